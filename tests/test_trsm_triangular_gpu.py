"""The triangular trsm of the leaf tails (k_tile_gemm<5>: with static pivots Winv = D^-1 L^-1 is lower triangular, the products with its
zeros are skipped) and the Schur SYRK whose waves above the diagonal of a diagonal tile pair only stage (kernels.hip.h):
 (a) factors (through a solve), inertia and Schur contribution against the oracle, at the tolerances of tests/test_leaf_gpu.py;
 (b) the same factorisation in a fresh process with PIPS_HIP_TRSM_DENSE=1, the dense product: tail panel, U = L D, pivots and SC agree
     entry for entry (a skipped product is +-0, the sums keep their order; +0 and -0 compare equal);
 (c) Bunch-Kaufman pivoting, whose Winv = Lambda^-1 G is dense, still takes the dense product and still matches LAPACK.
Shapes (tests/trsm_cases.py): the smallest where the predicates can go wrong - three tile columns with a padded last one, border rows
below one tile and across two (Schur tiles ti == tj and ti != tj), an all-tail block; two blocks each, column launches forced."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import trsm_cases as tc
from tests.test_leaf_gpu import RTOL_SC, RTOL_SOLVE
from tests.test_root_pivoting_gpu import hip_solve, lapack_solve_and_inertia

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def triangular():
    """every run of trsm_cases.RUNS factorised once in this process (triangular trsm), shared and read-only"""
    old = {k: os.environ.get(k) for k in ("PIPS_HIP_TAIL_SINGLE", "PIPS_HIP_TRSM_DENSE")}
    os.environ["PIPS_HIP_TAIL_SINGLE"] = "0"
    os.environ.pop("PIPS_HIP_TRSM_DENSE", None)
    try:
        res = {run: tc.factor_case(*run) for run in tc.RUNS}
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    for out in res.values():
        for a in out.values():
            a.setflags(write=False)
    return res


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    """the same runs in ONE fresh process with the dense product"""
    path = str(tmp_path_factory.mktemp("trsm_dense") / "dense.npz")
    env = dict(os.environ, PIPS_HIP_TAIL_SINGLE="0", PIPS_HIP_TRSM_DENSE="1")
    done = subprocess.run([sys.executable, "-m", "tests.trsm_cases", path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("run", tc.RUNS, ids=lambda r: f"{r[0]}-{'deterministic' if r[1] else 'default'}")
def test_shapes_are_what_the_cases_say_and_match_the_oracle(run, triangular):
    case, _ = run
    prob, out = tc.problem(case), triangular[run]
    tail = tc.CASES[case][6] or prob.n_leaf
    for b in range(prob.N):
        m, m_pad, nb, ldT = (int(v) for v in out[f"dims{b}"])
        assert m == tail and m % tc.TILE != 0 and m_pad == -(-m // tc.TILE) * tc.TILE
        assert nb % tc.TILE != 0 and (nb < tc.TILE) == (case != "A_border200") and (case != "A_border200" or tc.TILE < nb < 2 * tc.TILE)
        assert tuple(out[f"inertia{b}"]) == (prob.n_i, prob.my_i, 0)
    want = np.tril(prob.oracle_schur())
    err_sc = np.abs(out["SC"] - want).max() / np.abs(want).max()
    print(f"{case}: SC rel err {err_sc:.2e}")
    assert err_sc < RTOL_SC
    for b in range(prob.N):
        sl = slice(b * prob.n_leaf, (b + 1) * prob.n_leaf)
        xo = out["rhs"][sl].copy()
        prob.oracle_leaf(b).solve(xo)
        err = np.linalg.norm(out["x"][sl] - xo) / np.linalg.norm(xo)
        res = np.linalg.norm(prob.K_full(b) @ out["x"][sl] - out["rhs"][sl]) / np.linalg.norm(out["rhs"][sl])
        print(f"{case} block {b}: solve rel err {err:.2e}, residual {res:.2e}")
        assert err < RTOL_SOLVE and res < 1e-10


@pytest.mark.parametrize("run", tc.RUNS, ids=lambda r: f"{r[0]}-{'deterministic' if r[1] else 'default'}")
def test_dense_product_gives_the_same_entries(run, triangular, dense):
    case, det = run
    out = triangular[run]
    ref = {k: dense[f"{case}|{int(det)}|{k}"] for k in out}
    assert np.array_equal(out["SC"], ref["SC"]) and np.isfinite(out["SC"]).all()
    for b in range(tc.problem(case).N):
        assert np.array_equal(out[f"dims{b}"], ref[f"dims{b}"]) and np.array_equal(out[f"inertia{b}"], ref[f"inertia{b}"])
        got, want = tc.defined_entries(out, b), tc.defined_entries(ref, b)
        for name in ("panel", "U", "d"):
            assert got[name].size > 0 and np.isfinite(got[name]).all(), (b, name)
            assert np.array_equal(got[name], want[name]), (b, name, int((got[name] != want[name]).sum()))


def test_bunch_kaufman_keeps_the_dense_product():
    """test_root_pivoting_gpu.py's zero-diagonal matrix at three tile columns: no 1 x 1 pivot at the start of any tile, Winv is dense"""
    n = 300
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    M = M + M.T
    np.fill_diagonal(M, 0.0)
    B = rng.standard_normal((n, 3))
    Xl, inl = lapack_solve_and_inertia(M, B)
    Xh, inh = hip_solve(M, B)
    assert inh == (inl[0], inl[1], 0), (inh, inl)
    assert np.linalg.norm(M @ Xh - B) / np.linalg.norm(B) < 1e-11
    assert np.linalg.norm(Xh - Xl) / np.linalg.norm(Xl) < 1e-8
