"""The environment switches of libpipship.so go through one table (csrc/knobs.h): what each kind of switch parses to, that nothing in
csrc/ reads the environment behind the table's back, that every PIPS_HIP_* / PIPS_IPM_* name the tests, tools and documents use is a
switch the library reads, and that DESIGN.md section 10 is the library's table.  No GPU."""
import os
import re

import pytest

import pips_ipmpp_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = [None, "", "0", "1", "7", "abc"]

# What the parsing rules of the read sites give for VALUES, written out from those rules (atoi / atoll / atof, presence, the three-way
# flag), not computed by the library: (name, kind, [expected number per value]).
PARSE = [
    ("PIPS_HIP_ROOT_LAUNCHES", "set", [0, 1, 1, 1, 1, 1]),          # getenv(...) != nullptr: an empty value and "0" count as set
    ("PIPS_HIP_ROOT_DIAG_BARRIERS", "int", [0, 0, 0, 1, 7, 0]),     # v ? atoi(v) : 0 - "0" is off for the dense root as for the tails
    ("PIPS_HIP_MF", "int", [1, 0, 0, 1, 7, 0]),                     # v ? atoi(v) : 1
    ("PIPS_HIP_ROOT_POLL_LIMIT", "int", [400000, 0, 0, 1, 7, 0]),   # v ? atoll(v) : 400000
    ("PIPS_HIP_TAIL_SINGLE", "tri", [-1, 0, 0, 1, 1, 0]),           # v ? (atoi(v) != 0) : -1
    ("PIPS_HIP_RELAX_ZEROS", "real", [0.4, 0.0, 0.0, 1.0, 7.0, 0.0]),   # v ? atof(v) : 0.4
    ("PIPS_HIP_SC_REDUCE", "text", [0, 1, 1, 1, 1, 1]),             # the number of a text switch: whether it is there
    ("PIPS_IPM_ROOT_INEQ_ELIMINATE", "tri", [-1, 0, 0, 1, 1, 0]),
]


@pytest.mark.parametrize("name,kind,expected", PARSE, ids=[p[0] for p in PARSE])
def test_parse_rules(monkeypatch, name, kind, expected):
    assert pa.knobs()[name]["kind"] == kind
    for value, want in zip(VALUES, expected):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
        number, text = pa.knob_value(name)
        assert number == want, (name, value, number, want)
        assert text == (value if kind == "text" and value is not None else ""), (name, value, text)


def test_parse_rules_beyond_the_common_values(monkeypatch):
    monkeypatch.setenv("PIPS_HIP_ROOT_POLL_LIMIT", "5000000000")   # 64-bit: atoll
    assert pa.knob_value("PIPS_HIP_ROOT_POLL_LIMIT")[0] == 5000000000
    monkeypatch.setenv("PIPS_HIP_RELAX_ZEROS", "0.25")
    assert pa.knob_value("PIPS_HIP_RELAX_ZEROS")[0] == 0.25
    monkeypatch.setenv("PIPS_HIP_ROOT_DIAG_BARRIERS", "-3x")       # atoi: the leading number
    assert pa.knob_value("PIPS_HIP_ROOT_DIAG_BARRIERS")[0] == -3
    monkeypatch.setenv("PIPS_HIP_ROOT_TRACE", "a trace file.txt")
    assert pa.knob_value("PIPS_HIP_ROOT_TRACE") == (1, "a trace file.txt")


def test_values_are_read_live(monkeypatch):
    """nothing is kept between two calls: set, read, remove, read again (the pattern of test_layout_cpu.py)"""
    monkeypatch.setenv("PIPS_HIP_SN_WIDTH", "4")
    assert pa.knob_value("PIPS_HIP_SN_WIDTH")[0] == 4
    monkeypatch.delenv("PIPS_HIP_SN_WIDTH")
    assert pa.knob_value("PIPS_HIP_SN_WIDTH")[0] == 16


def test_unknown_name_is_an_error():
    retired = "PIPS_HIP_" + "HEAD_SLOTS"   # (in two pieces: test_no_dead_switch_names reads this file too)
    for name in (retired, "PIPS_HIP_MF ", "pips_hip_mf", ""):
        with pytest.raises(pa.capi.PipsHipError, match="not a switch"):
            pa.knob_value(name)


def test_table_is_well_formed():
    knobs = pa.knobs()
    assert len(knobs) >= 41
    for name, r in knobs.items():
        assert re.fullmatch(r"PIPS_(HIP|IPM)_[A-Z0-9_]+", name), name
        assert r["kind"] in ("set", "int", "tri", "real", "text"), name
        assert set(r["when"].split("+")) <= {"create", "analyze", "call", "process"}, name
        assert (r["default"] == "-") == (r["kind"] in ("set", "text")), name
        assert r["effect"] and "|" not in r["effect"], name
        if r["kind"] == "set":   # presence switches say so: "=0" does not switch them off
            assert "set to any value" in r["effect"], name


def test_only_knobs_cpp_reads_the_environment():
    csrc = os.path.join(ROOT, "pips-ipmpp_amd", "csrc")
    readers = []
    for dirpath, _, files in os.walk(csrc):
        for f in files:
            if f.endswith((".o", ".so")):
                continue
            with open(os.path.join(dirpath, f), errors="replace") as fh:
                if "getenv" in fh.read():
                    readers.append(f)
    assert readers == ["knobs.cpp"], readers
    assert open(os.path.join(csrc, "knobs.cpp")).read().count("getenv(") == 1


# Names of that shape that are no switch of the library, each with its reason.  None of them may be a name csrc/ reads.
NOT_LIBRARY_SWITCHES = {
    "PIPS_HIP_LIBRARY": "read by python/capi.py: the path of the shared library to load (experiment builds)",
    "PIPS_HIP_H": "the include guard of include/pips_hip.h",
    "PIPS_HIP_ROOT_": "a prefix in prose: 'the PIPS_HIP_ROOT_* switches'",
}
SCANNED = ["tests", "tools", "bench.py", "README.md", "INTEGRATION.md", os.path.join("profiles", "README.md"), os.path.join("include", "pips_hip.h")]
TOKEN = re.compile(r"PIPS_(?:HIP|IPM)_[A-Z0-9_]+")


def scanned_files():
    for entry in SCANNED:
        path = os.path.join(ROOT, entry)
        if os.path.isfile(path):
            yield path
        for dirpath, dirs, files in os.walk(path):
            dirs[:] = [d for d in dirs if d != "__pycache__"]
            for f in files:
                if not f.endswith(".pyc"):
                    yield os.path.join(dirpath, f)


def test_no_dead_switch_names():
    """A test or tool that sets a name the library does not read runs the default path and says nothing: every name must be in the table."""
    knobs = set(pa.knobs())
    allowed = set(NOT_LIBRARY_SWITCHES)
    assert not (allowed & knobs)
    csrc = os.path.join(ROOT, "pips-ipmpp_amd", "csrc")
    csrc_text = "".join(open(os.path.join(csrc, f), errors="replace").read() for f in os.listdir(csrc) if not f.endswith(".o"))
    assert not [a for a in allowed if f'"{a}"' in csrc_text]
    dead = {}
    n_files = 0
    for path in scanned_files():
        n_files += 1
        with open(path, errors="replace") as fh:
            text = fh.read()
        for tok in set(TOKEN.findall(text)) - knobs - allowed:
            dead.setdefault(tok, []).append(os.path.relpath(path, ROOT))
    assert n_files > 50
    assert not dead, dead


def section10_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("\n## 10. Environment switches"):]
    nxt = sec.find("\n## ", 1)
    sec = sec if nxt < 0 else sec[:nxt]
    rows = {}
    for ln in sec.splitlines():
        m = re.fullmatch(r"\| `(PIPS_(?:HIP|IPM)_[A-Z0-9_]+)` \| (\S+) \| (\S+) \| (\S+) \| (.*) \|", ln)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = {"kind": m.group(2), "default": m.group(3), "when": m.group(4), "effect": m.group(5)}
        else:
            assert not ln.startswith("| `PIPS_"), ln   # a table row that names a switch has exactly that form
    return rows


def test_design_section_10_is_the_librarys_table():
    rows, knobs = section10_rows(), pa.knobs()
    assert sorted(rows) == sorted(knobs), (sorted(set(rows) - set(knobs)), sorted(set(knobs) - set(rows)))
    assert rows == knobs, [n for n in knobs if rows[n] != knobs[n]]   # tools/knobs_table.py prints the rows
