"""The references of tests/test_dense_root_multi_gpu.py (tests/dense_root_multi_cases.py: 70 right-hand sides per case, three interleaved panels of
32, the last with 6 columns), validated with numpy and LAPACK alone (no GPU).  For every case:
  * the right-hand sides are what the recipe says: row 5 zero, row 40 e_0, row 69 e_{n-1};
  * the refinement that gives X* converged (a correction below 2^-58 max|x| within five steps);
  * static order: the unblocked FP64 LDL^T in the given order has the hinted signs and no pivot the device's rule would replace;
  * the predicate accepts x_ref0 itself at M = 1;
  * at the largest margin it may ever be given (M = 64) the predicate rejects what a wrong transposing copy would deliver: two columns swapped
    inside a panel (3 <-> 4) and across panels (2 <-> 34) - each of the swapped columns is rejected, the others stay accepted - and column 69
    left at its right-hand side (an out-copy that skips the last, partial panel).
And the C ABI: pips_hip_dense_ldl_solve_multi_dev is exported and returns PIPS_ERR_ARG for nrhs < 0 and for ld < n without touching a device
(a null handle has no n: every ld is too short for it)."""
import ctypes as C

import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import dense_root_multi_cases as mc
from tests import util as u

M_CAP = u.UNREFINED_M_CAP
_ALL = [(c, True) for c in mc.STATIC_CASES] + [(c, False) for c in mc.BK_CASES + [mc.ZERO_LEADING_TILE]]
_IDS = [("static-" if st else "bk-") + mc.case_id(c) for c, st in _ALL]


@pytest.mark.parametrize("case,static", _ALL, ids=_IDS)
def test_reference(case, static):
    ref = mc.reference(case, static)
    n, mode = ref.n, 0 if static else 1
    B = ref.B
    assert B.shape == (mc.NRHS, n) and ref.M.shape == (n, n) and np.array_equal(ref.M, ref.M.T)
    assert not B[5].any() and B[40, 0] == 1.0 and B[69, n - 1] == 1.0 and np.count_nonzero(B[40]) == 1 and np.count_nonzero(B[69]) == 1
    assert ref.converged and 1 <= ref.refinement_steps <= 4, ref.refinement_steps
    print(f"dense-root-multi-reference case={mc.case_id(case)} static={static} steps={ref.refinement_steps}")
    x0 = ref.X_static if static else ref.X_lapack
    assert np.isfinite(ref.X_star).all() and np.isfinite(x0).all() and not x0[5].any()
    if static:
        n_primal, d = case[1], ref.d
        assert np.all(d[:n_primal] > 0.0) and np.all(d[n_primal:] < 0.0)
        assert np.abs(d).min() >= 1e-8 * np.abs(np.diag(ref.M)).max()
        assert ref.inertia == (n_primal, n - n_primal, 0)
    else:
        assert ref.X_static is None and sum(ref.inertia) == n and ref.inertia[2] == 0
    assert ref.accepts(x0, 1, mode).all()
    for a, b in ((3, 4), (2, 34)):
        X = x0.copy()
        X[[a, b]] = X[[b, a]]
        ok = ref.accepts(X, M_CAP, mode)
        assert not ok[a] and not ok[b] and ok.sum() == mc.NRHS - 2, (a, b, ref.ratios(X, mode))
    X = x0.copy()
    X[69] = B[69]
    ok = ref.accepts(X, M_CAP, mode)
    assert not ok[69] and ok.sum() == mc.NRHS - 1, ref.ratios(X, mode)


def test_zero_leading_tile_is_the_matrix_of_the_pivoting_test():
    M = mc.zero_leading_tile_matrix()
    assert M.shape == (288, 288) and not M[:128, :128].any() and np.array_equal(M, M.T)
    assert np.linalg.matrix_rank(M[128:, :128]) == 128


def test_multi_dev_entry_is_exported_and_checks_its_arguments():
    assert "pips_hip_dense_ldl_solve_multi_dev" in pa.capi.SYMBOLS
    f = pa.capi.lib.pips_hip_dense_ldl_solve_multi_dev
    f.restype = C.c_int
    err_arg = 1                                      # PIPS_ERR_ARG (csrc/common.h)
    assert f(None, C.c_int(-1), None, C.c_longlong(4)) == err_arg
    assert b"pips_hip_dense_ldl_solve_multi_dev" in pa.capi.lib.pips_hip_last_error()
    assert f(None, C.c_int(3), None, C.c_longlong(-1)) == err_arg
    assert f(None, C.c_int(0), None, C.c_longlong(0)) == err_arg      # (a null handle is an error before nrhs == 0 is a no-op)
    assert hasattr(pa.HipDenseLdlSolver, "solve_multi_dev")
