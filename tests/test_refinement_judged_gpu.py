"""The refinement layer judged row by row: the residual r = b - K x (k_full_spmv_sub, k_full_spmv_sub_long, launch_residual), the per-block
norms (k_vec_block_absmax), the measure (worst_from_norms, k_mrefine_measure) and the choice of columns in solve_multi with its compaction
and scatter-back (k_maxpy_idx, k_maxpy).

A correct factor leaves a residual at rounding level, where nothing can be compared tightly.  Here the handle is factorised with K1 and then
handed the values K2 = K1 + E (LeafBatch.set_values / HipLdlSolver.set_values_only only copy the values; no solve sweep reads them): x0 =
K1^-1 b, the refinement's residual is -E x0 plus rounding, and after one correction K1 x1 = b - E x0 holds row by row.  The predicates of
util.RefinementReference, all sums in long double, per right-hand side, per block, over every row, noise_b = 2^-53 (||K1_b||inf ||x_b||inf +
||b_b||inf):

    uncorrected      |K1 x - b|_i             <= M noise_b
    corrected_once   |K1 x - (b - E x*)|_i    <= M noise_b        x* the oracle's twice refined solution of K1 x = b
    corrected_twice  |K1 x - (b - E x1*)|_i   <= M noise_b        x1* = x* - K1^-1 E x*
    measure_close    |dev - eta*(x)| <= max_b gamma_b / den_b + 4 2^-53 eta*,  gamma_b = max_i (nnz_i + 2) 2^-53 (|K2| |x| + |b|)_i  (derived)

tests/test_refinement_reference_cpu.py proves for every case that every row carries a signal of 2^14 noise_b, that the reference passes at
M = 4 and that a skipped or shifted row, a stale upper-triangle value, a missing long row, a correction in the wrong column or at the wrong
stride and a measure without its worst block are rejected at M = 64 (the weakest mutant stands at 6.6e5 noise_b); its docstring says what
was chosen about the inputs and why.

Cases:
  1. one right-hand side on a LeafBatch of six blocks - Problem blocks of 127, 256, 257 and 2049 rows, a time-coupled one of 900, and a leaf
     whose primal column 0 sits in 530 equality rows (a full row of 531 entries: k_full_spmv_sub_long, and the copy branch of launch_residual) -
     E = 2^-10 (+-1) K_ij in the block meant to be worst (first, middle, last, the long-row block) and 2^-13 in the others; atomics and
     deterministic mode; set_refinement (mode 0) and set_refinement_backward_error (mode 1).  tol = 1 with two steps allowed: no step, the
     result `uncorrected`, the measure close, deterministic mode bit-equal to refine_steps = 0; one unconditional step: `corrected_once`;
     tol = 1e-9 with two steps: two steps, `corrected_twice`.  The same on one time-coupled block of 16 500 rows (absmax_chunks() = 2).
  2. nrhs in {2, 8, 33, 257} on a HipLdlSolver, one step, backward error, tol = tau, E on J x J (J a random half of the rows): every column
     passes the predicate its host measure dictates and fails the other (util.refine_multi_judge); ld = n and n + 5 (the padding untouched),
     PIPS_HIP_MULTI unset and "0", deterministic mode at 33; dirty sets all (k_maxpy), none, exactly one (the solve_once branch), mixed with
     the first and last column of a chunk, column 256 alone (the second chunk), and E on every entry with all columns dirty (every row of
     every column: the grid.y / vec_stride indexing).
  3. last_refinement_steps over chunks is "the steps of the last chunk that took any": 257 dirty columns with one allowed step report 1
     (the engine used to add the chunks up and report 2, and 9 with PIPS_HIP_MULTI=0), and a clean last chunk does not reset it.

Measured on an MI355X, largest ratio deviation / noise_b over the cases of a path:

    path                                                              uncorrected    once    twice
    1. batch of six, atomics (mode 0 and 1 alike to 3 digits)          0.974          1.04    1.16
       batch of six, deterministic                                     0.909          1.11    1.15
       one block of 16 500 rows, atomics                               0.875          0.817   0.870
       one block of 16 500 rows, deterministic                         0.859          0.818   0.934
    (the device's measure stands within 0.004 of the derived slack of eta* in every case)

    path (the figure of the predicate each column has to pass)         all     mixed   one     none    first / second chunk
    2. one sweep per right-hand side (2 columns)                       0.744   0.757   0.774   0.473
       interleaved panels (8, 33, 257 columns)                         1.33    2.22    2.35    1.98    2.09 / 2.34
       PIPS_HIP_MULTI=0 (chunks of 32)                                 1.23    1.16                    - / 0.867
       deterministic panels (33 columns)                               0.980   1.26    1.26
       E on every entry: panels 1.10, PIPS_HIP_MULTI=0 1.00, deterministic 1.03

Largest ratio 2.35 (an uncorrected column beside the one dirty column of 257): M = 16, the smallest power of two that is at least 4 x 2.35 = 9.4.
"""
import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import util as u

pytestmark = pytest.mark.gpu

M = 16       # the smallest power of two >= 4 x the largest measured ratio (2.35), see above; never above 64


def _report(path, ratio):
    print(f"refine-ratio path={path} ratio={ratio:.4g}")
    assert M <= u.UNREFINED_M_CAP


# ---- 1. one right-hand side on a LeafBatch ----------------------------------------------------------------------------------------------
def _judged_batch(names, refs, mode, det, path):
    import torch   # noqa: F401  (the device runtime)
    N = len(refs)
    mats = [u.refine_block_matrix(name) for name in names]
    bt = pa.LeafBatch(N, 0)
    for b, (K, n_i) in enumerate(mats):
        bt.set_block(b, K, n_i)
    if det:
        bt.set_deterministic()
    set_refinement = bt.set_refinement_backward_error if mode == 1 else bt.set_refinement
    set_refinement(2, 1.0)
    bt.analyze(4)
    for b, ref in enumerate(refs):
        bt.set_values(b, ref.val1)
    bt.factor()
    for b, (K, n_i) in enumerate(mats):
        assert bt.inertia(b) == (n_i, K.nrows - n_i, 0)            # the device perturbs no pivot either: its factors are those of K1
    for b, ref in enumerate(refs):
        bt.set_values(b, ref.val2)                                 # the factors stay, the refinement sees K2
    rhs = np.concatenate([ref.B[0] for ref in refs])
    cut = np.cumsum([ref.n for ref in refs])[:-1]

    def solve():
        x = rhs.copy()
        bt.solve(x)
        return np.split(x, cut)

    # tol = 1, two steps allowed: the measure is taken and no step follows
    xs = solve()
    assert bt.last_refinement_steps() == 0
    dev = bt.last_refinement_measure()
    eta, slack = u.refine_batch_measure(refs, xs, mode)
    q0 = max(ref.ratios_uncorrected(x)[0] for ref, x in zip(refs, xs))
    _report(f"{path}/uncorrected", q0)
    print(f"refine-measure path={path} dev={dev:.17g} eta={eta:.17g} |dev-eta|/slack={abs(dev - eta) / slack:.3g}")
    assert q0 <= M, [ref.ratios_uncorrected(x)[0] for ref, x in zip(refs, xs)]
    assert abs(dev - eta) <= slack, (dev, eta, slack)
    if det:
        bt.set_refinement(0, 0.0)
        plain = solve()
        assert bt.last_refinement_steps() == 0 and all(np.array_equal(a, b) for a, b in zip(plain, xs))
    # one unconditional step
    set_refinement(1, 0.0)
    xs = solve()
    assert bt.last_refinement_steps() == 1
    q1 = [ref.ratios_once(x)[0] for ref, x in zip(refs, xs)]
    _report(f"{path}/once", max(q1))
    assert max(q1) <= M, q1
    # tol = 1e-9, two steps: the measure after the first step still exceeds it
    set_refinement(2, 1e-9)
    xs = solve()
    assert bt.last_refinement_steps() == 2
    q2 = [ref.ratios_twice(x)[0] for ref, x in zip(refs, xs)]
    _report(f"{path}/twice", max(q2))
    assert max(q2) <= M, q2
    bt.close()


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("mode", [0, 1], ids=["rhs_norm", "backward_error"])
@pytest.mark.parametrize("worst", u.REFINE_BATCH_WORST, ids=[f"worst{w}" for w in u.REFINE_BATCH_WORST])
def test_one_right_hand_side_on_a_batch(worst, mode, det):
    refs = u.refine_batch_references(worst)
    assert refs[2].row_len.max() > u.REFINE_FULL_LONG_ROW        # a long row exists: layout.cpp sends it to k_full_spmv_sub_long by this count
    _judged_batch(u.REFINE_BATCH_BLOCKS, refs, mode, det, f"batch/worst{worst}/mode{mode}/{'det' if det else 'atomics'}")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("mode", [0, 1], ids=["rhs_norm", "backward_error"])
def test_one_block_of_two_norm_chunks(mode, det):
    ref = u.refine_block_reference("big", u.REFINE_EPS_WORST)
    assert ref.n >= 16384                                         # absmax_chunks() = n_total / nblk / 16384 + 1 = 2
    _judged_batch(("big",), [ref], mode, det, f"big/mode{mode}/{'det' if det else 'atomics'}")


# ---- 2. several right-hand sides on a handle, through set_values_only -------------------------------------------------------------------
# (nrhs, dirty set, row length beyond n, PIPS_HIP_MULTI, deterministic)
_MULTI = [(nrhs, s, 0, None, False) for nrhs in u.REFINE_MULTI_NRHS for s in ("all", "none", "one", "mixed")] + \
         [(257, "first_chunk", 0, None, False), (257, "second_chunk", 0, None, False), (257, "second_chunk", 5, "0", False)] + \
         [(nrhs, s, 5, None, False) for nrhs in (33, 257) for s in ("all", "mixed")] + \
         [(8, "mixed", 0, "0", False), (33, "mixed", 5, "0", False), (33, "all", 0, "0", False), (257, "mixed", 0, "0", False), (257, "all", 5, "0", False)] + \
         [(33, s, pad, None, True) for s, pad in (("all", 0), ("one", 0), ("mixed", 5))] + \
         [(33, "all_entries", 5, None, False), (33, "all_entries", 0, "0", False), (33, "all_entries", 0, None, True)]


def _multi_id(c):
    nrhs, s, pad, multi, det = c
    return f"{nrhs}-{s}-ld_n{'+5' if pad else ''}-multi{'_unset' if multi is None else multi}{'-deterministic' if det else ''}"


@pytest.mark.parametrize("case", _MULTI, ids=[_multi_id(c) for c in _MULTI])
def test_several_right_hand_sides_column_choice(case, monkeypatch):
    import torch
    nrhs, dirty_set, pad, multi, det = case
    for k, v in (("PIPS_HIP_MULTI", multi), ("PIPS_HIP_DETERMINISTIC", None), ("PIPS_HIP_SWEEP_LAUNCHES", None)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    ref = u.refine_multi_reference(nrhs, dirty_set)
    prob = u.refine_multi_problem()
    K, n = prob.blocks[0]["K"], prob.n_leaf
    ld = n + pad
    s = pa.HipLdlSolver(K, n_primal=prob.n_i, refine_steps=1, refine_tol=ref.tau, backward_error=True)
    if det:
        s.set_deterministic()
    s.matrixChanged()
    assert s.get_inertia() == (prob.n_i, prob.my_i, 0)
    s.set_values_only(ref.val2)
    Xd = torch.full((nrhs, ld), 7.5, dtype=torch.float64, device="cuda")
    Xd[:, :n] = torch.tensor(ref.B, device="cuda")
    s.solve_dev(Xd, nrhs=nrhs, ld=ld)
    torch.cuda.synchronize()
    X = Xd.cpu().numpy()
    info = s.info()
    s.close()
    interleaved = nrhs >= 8 if multi is None else multi != "0"
    assert info["last_multi_path"] == (2 if det else 1 if interleaved else 0), info
    assert np.all(X[:, n:] == 7.5)                                 # the padding untouched
    ok, ratio = u.refine_multi_judge(ref, X[:, :n], M)
    _report(f"multi/{dirty_set}/{'det' if det else 'multi0' if multi == '0' else 'panels' if interleaved else 'per_rhs'}", ratio.max())
    assert ok.all(), (np.nonzero(~ok)[0], [ref.kinds[c] for c in np.nonzero(~ok)[0]], ratio[~ok])
    # 3. the steps of the last chunk that took any: one step was allowed, so 1 wherever a column is dirty - however many chunks took it
    assert info["last_refinement_steps"] == (1 if "dirty" in ref.kinds else 0), info


# ---- the seam itself ----------------------------------------------------------------------------------------------------------------------
def test_set_values_only_states():
    prob = u.Problem(77, 2, 400, 200, 10, 10, 0.03, diag_lo=-2.0, diag_hi=2.0)
    K = prob.blocks[0]["K"]
    s = pa.HipLdlSolver(K, n_primal=prob.n_i)
    with pytest.raises(pa.capi.PipsHipError, match="factor first"):
        s.set_values_only(K.val)                                   # before the first factorisation
    s.analyze()
    with pytest.raises(pa.capi.PipsHipError, match="factor first"):
        s.set_values_only(K.val)
    s.matrixChanged()
    s.set_values_only(K.val)
    s.close()
    solvers = [pa.HipLdlSolver(prob.blocks[b]["K"], n_primal=prob.n_i) for b in range(2)]
    pa.HipLdlSolver.factor_schur_batch(solvers)
    with pytest.raises(pa.capi.PipsHipError, match="batch"):
        solvers[0].set_values_only(K.val)                          # the newest factors are the group's
    solvers[0].matrixChanged()                                     # its own factors are the newest again
    solvers[0].set_values_only(K.val)
    for h in solvers:
        h.close()
