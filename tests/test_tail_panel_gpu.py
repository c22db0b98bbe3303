"""The leaf tails group by group (csrc/engine.hip tail_panels, kernels.hip.h k_tile_panel): per group of four tile columns
the diagonal block is finished on the side stream and ONE launch runs trsm and short updates of every tile row below it, a workgroup per
row.  Every tile takes the products of the column launches in their order, so the same factorisation in a fresh process with
PIPS_HIP_TAIL_PANEL=0 gives the same entries, not merely close ones: tail panel, U = L D, pivots, inertia, SC and a solution, compared
with np.array_equal on what a factorisation defines, for two consecutive factorisations with different values on one handle.  That
the two sides took the two paths shows in what each handle's timer booked as diagonal tiles and trsm launches.
Shapes (tests/tail_panel_cases.py; tests/test_tail_panel_plan_cpu.py checks that they are what it says): a full group and a short one
with a padded last column and one padded border tile row; three groups under a sparse head, the last a single column, with two border
tile rows and with none; a banded block whose strips start at different columns; blocks of six and nine tile columns in one batch.
Two blocks each, PIPS_HIP_TAIL_SINGLE=0 on both sides (batches this small would take the single launch)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tail_panel_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{c}-{'deterministic' if d else 'default'}" for c, d in pc.RUNS]


@pytest.fixture(scope="module")
def grouped():
    """every run of tail_panel_cases.RUNS factorised once in this process (the groups: the default), shared and read-only"""
    names = ("PIPS_HIP_TAIL_SINGLE", "PIPS_HIP_TAIL_PANEL", "PIPS_HIP_TRSM_DENSE")
    old = {k: os.environ.get(k) for k in names}
    os.environ["PIPS_HIP_TAIL_SINGLE"] = "0"
    os.environ.pop("PIPS_HIP_TAIL_PANEL", None)
    os.environ.pop("PIPS_HIP_TRSM_DENSE", None)
    try:
        res = {run: pc.factor_case(*run) for run in pc.RUNS}
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    for out in res.values():
        for a in out.values():
            a.setflags(write=False)
    return res


@pytest.fixture(scope="module")
def columns(tmp_path_factory):
    """the same runs in ONE fresh process with the column launches"""
    path = str(tmp_path_factory.mktemp("tail_panel") / "columns.npz")
    env = dict(os.environ, PIPS_HIP_TAIL_SINGLE="0", PIPS_HIP_TAIL_PANEL="0")
    env.pop("PIPS_HIP_TRSM_DENSE", None)
    done = subprocess.run([sys.executable, "-m", "tests.tail_panel_cases", path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("run", pc.RUNS, ids=IDS)
def test_the_factorisation_is_sound(run, grouped):
    """inertia, finite entries, and a solution whose residual is small: the comparison below is between two sound factorisations"""
    case, _ = run
    blocks, _, _ = pc.batch(case)
    out = grouped[run]
    off = 0
    for b, (K, n_i, _) in enumerate(blocks):
        assert tuple(out[f"inertia{b}"]) == (n_i, K.nrows - n_i, 0)
        Kl = pc.scipy_lower(K)
        Kf = Kl + Kl.T - pc.scipy_diag(Kl)
        x, r = out["x"][off:off + K.nrows], out["rhs"][off:off + K.nrows]
        res = np.linalg.norm(Kf @ x - r) / np.linalg.norm(r)
        print(f"{case} block {b}: residual {res:.2e}")
        assert res < 1e-10
        off += K.nrows
    assert np.isfinite(out["SC"]).all() and np.isfinite(out["first_SC"]).all()


@pytest.mark.parametrize("run", pc.RUNS, ids=IDS)
def test_the_column_launches_give_the_same_entries(run, grouped, columns):
    case, det = run
    out = grouped[run]
    ref = {k: columns[f"{case}|{int(det)}|{k}"] for k in out}
    # the two sides took the two paths: what the handle's timer booked in the second factorisation
    ntc = max(int(out[f"dims{b}"][1]) // pc.TILE for b in range(len(pc.batch(case)[0])))
    assert ntc > 4
    upd, diag, trsm = (int(v) for v in out["tail_launches"])
    print(f"{case}: {ntc} tile columns; launches booked (update, diagonal, trsm) {(upd, diag, trsm)} group by group")
    upd_c, diag_c, trsm_c = (int(v) for v in ref["tail_launches"])
    print(f"{case}: {(upd_c, diag_c, trsm_c)} column by column")
    # group by group the first group's four diagonal tiles (and those of a group with no tile row below it) are booked on the main stream;
    # the trsm of column 3 has no tile inside the first group's block: it lies in a panel launch, booked as an update, where the column
    # path books a trsm launch (that path books a diagonal tile on the main stream only where the tile takes no update)
    assert diag >= 4 and trsm < trsm_c, ((upd, diag, trsm), (upd_c, diag_c, trsm_c))
    assert np.array_equal(out["SC"], ref["SC"]) and np.array_equal(out["first_SC"], ref["first_SC"])
    assert np.array_equal(out["x"], ref["x"]) and np.isfinite(out["x"]).all()
    for b in range(len(pc.batch(case)[0])):
        assert np.array_equal(out[f"dims{b}"], ref[f"dims{b}"]) and np.array_equal(out[f"inertia{b}"], ref[f"inertia{b}"])
        got, want = pc.defined_entries(out, b), pc.defined_entries(ref, b)
        for name in ("panel", "U", "d"):
            assert got[name].size > 0 and np.isfinite(got[name]).all(), (b, name)
            assert np.array_equal(got[name], want[name]), (b, name, int((got[name] != want[name]).sum()))
        # the first factorisation on the handle: its panel (U and the pivots were overwritten by the second)
        got, want = pc.first_panel(out, b), pc.first_panel(ref, b)
        assert np.isfinite(got).all() and np.array_equal(got, want), (b, "first panel", int((got != want).sum()))
        assert not np.array_equal(got, pc.defined_entries(out, b)["panel"])   # (the two factorisations had different values)
