"""The inputs of tests/test_unrefined_sweeps_gpu.py, validated with the oracle alone (no GPU): for every case and every right-hand side
  * the oracle's static-pivot LDL^T perturbs no pivot - its inertia is (n_i, my_i, 0) - so its unrefined solution is that of K itself and
    eta_ref measures two triangular sweeps in FP64, nothing else;
  * the predicate  eta(x) <= M max(eta_ref, 2^-53)  and  ||x - x*||inf <= M max(||x_ref0 - x*||inf, 2^-53 ||x*||inf)  has teeth at the
    largest margin it may ever be given (M = 64): it rejects the oracle's own unrefined solution rounded to float32 and back, and the same
    solution with one randomly chosen entry set to zero - both through the backward error alone;
  * it accepts what it must: the oracle's unrefined solution at M = 1.
The all-zero right-hand side has no such perturbation (its solution is the zero vector, which float32 holds exactly): what is asked of it
on the device is exact zeros, and here that the oracle returns them and that the predicate rejects a single entry of 1e-300."""
import numpy as np
import pytest

from tests import util as u

M_CAP = u.UNREFINED_M_CAP


def _check_reference(ref, seed):
    prob = ref.prob
    assert ref.inertia == (prob.n_i, prob.my_i, 0), ref.inertia          # no perturbed pivot
    assert np.isfinite(ref.X0).all() and np.isfinite(ref.XS).all()
    assert ref.accepts(ref.X0, 1).all()
    if prob.n_leaf <= 700:      # the helper's measure against a dense restatement of the formula (long double residual, last right-hand side)
        Kf = prob.K_full(ref.b).toarray()
        k = ref.B.shape[0] - 1
        r = ref.B[k].astype(np.longdouble) - Kf.astype(np.longdouble) @ ref.X0[k].astype(np.longdouble)
        eta = float(np.abs(r).max()) / (np.abs(Kf).sum(axis=1).max() * np.abs(ref.X0[k]).max() + np.abs(ref.B[k]).max())
        # (two summation orders of a long double residual: each within (row length) * 2^-64 of the exact one, relative to the denominator)
        assert abs(eta - ref.eta_ref[k]) <= 2 * (np.count_nonzero(Kf, axis=1).max() + 1) * 2.0 ** -64
    rng = np.random.default_rng(seed)
    zero_rows = [q for q in range(ref.B.shape[0]) if not ref.B[q].any()]
    assert zero_rows == ([ref.what["zero"]] if "zero" in getattr(ref, "what", {}) else [])
    rounded = ref.X0.astype(np.float32).astype(np.float64)
    holed = ref.X0.copy()
    for q in range(ref.B.shape[0]):
        holed[q, rng.integers(ref.X0.shape[1])] = 0.0 if q not in zero_rows else 1e-300
    bw_rounded, bw_holed = ref.backward_ratios(rounded), ref.backward_ratios(holed)
    for q in range(ref.B.shape[0]):
        if q in zero_rows:
            assert not ref.X0[q].any() and not ref.XS[q].any() and ref.eta_ref[q] == 0.0
            assert bw_holed[q] > M_CAP
            continue
        assert ref.eta_ref[q] > 0.0
        assert bw_rounded[q] > M_CAP, (q, bw_rounded[q], ref.eta_ref[q])
        assert bw_holed[q] > M_CAP, (q, bw_holed[q], ref.eta_ref[q])
    real = np.array([q not in zero_rows for q in range(ref.B.shape[0])])
    assert not ref.accepts(rounded, M_CAP)[real].any() and not ref.accepts(holed, M_CAP).any()


@pytest.mark.parametrize("shape", list(u.UNREFINED_SINGLE_SHAPES))
def test_single_right_hand_side_inputs(shape):
    _check_reference(u.unrefined_reference("single", shape), 1)


@pytest.mark.parametrize("nrhs", u.UNREFINED_MULTI_NRHS)
def test_many_right_hand_sides_inputs(nrhs):
    ref = u.unrefined_reference("multi", nrhs)
    assert ref.B.shape == (nrhs, ref.prob.n_leaf)
    what = ref.what
    assert np.abs(ref.B[what["scaled"]]).max() > 1e5 and np.count_nonzero(ref.B[what["scaled"]]) == ref.prob.n_leaf
    if nrhs >= 7:
        for name in ("unit_head", "unit_tail"):
            row = ref.B[what[name]]
            assert np.count_nonzero(row) == 1 and row.max() == 1.0
        assert len({what[k] for k in what}) == 4 and nrhs - len(what) >= 3      # the rest are Gaussian rows
    _check_reference(ref, nrhs)


@pytest.mark.parametrize("shape", list(u.UNREFINED_BATCH_SHAPES))
def test_batch_inputs(shape):
    prob = u._unrefined_cached_problem("batch", shape)
    for b in range(prob.N):
        _check_reference(u.unrefined_reference("batch", (shape, b)), b)     # a row per repetition of the solve
    ref = u.unrefined_reference("batch_multi", shape)
    assert ref.B.shape[0] == u.UNREFINED_BATCH_NRHS
    _check_reference(ref, 99)
