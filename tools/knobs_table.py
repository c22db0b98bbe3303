"""The switch table of DESIGN.md section 10, printed from the library's own table (pips_hip_knobs; csrc/knobs.h).  No GPU needed.

    python tools/knobs_table.py          # the markdown rows; paste them over the table of section 10

tests/test_knobs_cpu.py compares section 10 with the library row by row, so a row changed in csrc/knobs.h fails there until this
output is pasted again."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pips_ipmpp_amd as pa  # noqa: E402


def rows():
    yield "| switch | kind | default | read at | effect |"
    yield "|---|---|---|---|---|"
    for name, r in pa.knobs().items():
        yield f"| `{name}` | {r['kind']} | {r['default']} | {r['when']} | {r['effect']} |"


if __name__ == "__main__":
    print("\n".join(rows()))
