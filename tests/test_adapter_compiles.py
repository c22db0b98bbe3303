"""The reference-side bindings of INTEGRATION.md (examples/adapter/HipLdlSolver.h, HipDenseLdlSolver.h: the DoubleLinearSolver
subclasses a PIPS-IPM++ maintainer adds): the class body INTEGRATION.md quotes is the one in the file."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_integration_md_shows_the_same_adapter():
    """INTEGRATION.md quotes the leaf adapter: the quoted class body and the file must not drift apart."""
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = open(os.path.join(ROOT, "examples", "adapter", "HipLdlSolver.h")).read()
    start = md.index("class HipLdlSolver : public DoubleLinearSolver {")
    body = md[start:md.index("```", start)].strip()
    assert body in src
