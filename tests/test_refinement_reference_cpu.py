"""The inputs and the reference of tests/test_refinement_judged_gpu.py, validated with the oracle alone (no GPU).

The lever (tests/util.py, RefinementReference): factor K1, hand the refinement the values K2 = K1 + E.  The residual of x0 = K1^-1 b is then
-E x0 plus rounding, and one correction leaves K1 x1 = b - E x0 row by row.  For every case of the GPU table this module checks that
  * the oracle perturbs no pivot of K1 (inertia (n_i, my_i, 0)): x0 is the solution of K1 itself;
  * input condition 1: with E on every stored entry every row of every right-hand side carries |(E x*)_i| >= 2^14 noise_b,
    noise_b = 2^-53 (||K1_b||inf ||x_b||inf + ||b_b||inf) - 256 times the largest margin M = 64, no row left out;
    input condition 2: in the column-choice cases eta* of the dirty columns lies 2^20 above that of every other, tau between them;
  * replacing x0 by x* in the target costs far less than noise_b (measured on x0_ref: below 1 / 4);
  * the reference passes its own predicates at M = 4: x0_ref `uncorrected`, x1_ref `corrected_once`, x2_ref `corrected_twice` - and each of
    them fails the other two at M = 64;
  * every mutant of the host emulation refine_fp64 / refine_multi_fp64 / refine_measure_fp64 is rejected at M = 64: a residual row skipped
    (first row, last row of the block, a row of more than 8 entries, the long row), the copies above the diagonal left unperturbed (a stale
    fsrc), a block's rows shifted by one, the long row's product missing, a correction added to the neighbouring column or at distance n in
    an array of rows of n + 5, the worst block dropped from the measure, ||x|| missing from the denominator of mode 1, and a measure that is
    off by the second-largest row.

Choices about the inputs, and the figures that decided them (the oracle alone, this module):
  * all primal diagonals span 1e-1 .. 1e2 (util.refine_block_matrix): with 1e-2 .. 1e2 the oracle's own x0 stands 7 .. 15 x noise_b on the
    blocks of 256 and 2049 rows and on the long-row leaf (the factors grow like 1 / smallest diagonal) and would miss `uncorrected` at M = 4.
    The block of the column-choice cases is unrefined_multi_problem() with its diagonal redrawn the same way: under its default
    1e-4 .. 1e4 x0_ref stands at 13 .. 24 x noise_b;
  * the all-entries case of several right-hand sides takes E = 2^-10 |K1| against positive xs: with random signs the weakest of 33 x 2250
    rows cancels down to 3.8e3 x noise_b, and 2^-8 would not lift it to 2^14 either;
  * E confined to J x J leaves rows without any signal by construction, so condition 1 is asked of the all-entries cases and the column-choice
    cases are held to condition 2 and to the two-sided verdict of util.refine_multi_judge.  A clean column (xs = 0 on J) cannot fail
    `corrected_once` - E x* is zero to rounding there, both targets coincide - so every third column that is not dirty is "faint": xs on J
    scaled by 2^-24, eta* 1e7 below the dirty ones and below tau, and yet 2e5 x noise_b apart between "corrected" and "left alone";
  * tol = 1e-9 with two steps: eta* after one step stands 8e2 .. 1e5 above tol in every rotation and mode, which is what makes the device take
    the second step.  After two steps it is 4.5e-10 .. 6.5e-8: the contraction per step is 2^-10 only where K1^-1 E has no large direction
    (the long-row leaf contracts by 1 / 12 in its first step), and 2^-30 = 9.3e-10 leaves mode 0 no room.  The engine takes no measure after
    the last allowed step, so this decides nothing on the device; the module asserts the contraction and prints the figure.
"""
import os
import re

import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import util as u

M_OWN, M_CAP = 4, u.UNREFINED_M_CAP
_BLOCK_CASES = [(name, eps) for name in u.REFINE_BATCH_BLOCKS for eps in (u.REFINE_EPS_WORST, u.REFINE_EPS_OTHER)] + [("big", u.REFINE_EPS_WORST)]


def test_long_row_constant_and_leaf():
    src = open(os.path.join(os.path.dirname(os.path.abspath(pa.__file__)), "..", "pips-ipmpp_amd", "csrc", "records.h")).read()
    assert int(re.search(r"constexpr int FULL_LONG_ROW = (\d+);", src).group(1)) == u.REFINE_FULL_LONG_ROW
    K, n_i, my_i, long_row = u.refine_long_row_leaf()
    probe = pa.symbolic_probe(K, n_i)
    assert (probe["n_head"], probe["m"]) == (620, 640), probe                  # the host symbolic pass accepts it
    ref = u.refine_block_reference("long_row", u.REFINE_EPS_WORST)
    assert ref.row_len[long_row] == 531 > u.REFINE_FULL_LONG_ROW and np.sum(ref.row_len > u.REFINE_FULL_LONG_ROW) == 1
    for name in u.REFINE_BATCH_BLOCKS:                  # rows beyond the eight lanes of a lane group in every block but the banded one
        assert (u.refine_block_reference(name, u.REFINE_EPS_WORST).row_len.max() > 8) == (name != "tc900"), name


@pytest.mark.parametrize("name,eps", _BLOCK_CASES, ids=[f"{n}-2^{int(np.log2(e))}" for n, e in _BLOCK_CASES])
def test_block_reference_and_residual_mutants(name, eps):
    ref = u.refine_block_reference(name, eps)
    K, n_i = u.refine_block_matrix(name)
    assert ref.inertia == (n_i, K.nrows - n_i, 0), ref.inertia                   # no perturbed pivot
    assert np.count_nonzero(ref.E) >= len(ref.E) - 2 * np.sum(np.abs(ref.val1) == ref.amax1)      # E on every stored entry but the largest
    sig, swap = ref.signal_over_noise(), ref.target_swap_over_noise()
    print(f"refine-input block={name} eps=2^{int(np.log2(eps))} signal/noise={sig.min():.3g} swap/noise={swap.max():.3g}")
    assert (sig >= u.REFINE_SIGNAL).all(), sig                                   # condition 1: every row
    assert (swap <= 0.25).all(), swap
    own = (ref.ratios_uncorrected(ref.X0_ref), ref.ratios_once(ref.X1_ref), ref.ratios_twice(ref.X2_ref))
    print(f"refine-own block={name} uncorrected={own[0].max():.3g} once={own[1].max():.3g} twice={own[2].max():.3g}")
    assert ref.uncorrected(ref.X0_ref, M_OWN).all() and ref.corrected_once(ref.X1_ref, M_OWN).all() and ref.corrected_twice(ref.X2_ref, M_OWN).all(), own
    assert not ref.corrected_once(ref.X0_ref, M_CAP).any() and not ref.corrected_twice(ref.X0_ref, M_CAP).any()
    assert not ref.uncorrected(ref.X1_ref, M_CAP).any() and not ref.corrected_twice(ref.X1_ref, M_CAP).any()
    assert not ref.uncorrected(ref.X2_ref, M_CAP).any() and not ref.corrected_once(ref.X2_ref, M_CAP).any()
    # the emulation without a mutant is the reference itself
    assert np.array_equal(u.refine_fp64(ref, ref.X0_ref, 1), ref.X1_ref)
    weakest = int(np.argmin(np.abs(ref.EXS[0])))
    rows = {"first": 0, "last": ref.n - 1, "weakest": weakest}
    if ref.row_len.max() > 8:
        rows["more_than_8"] = int(np.argmax((ref.row_len > 8) & (ref.row_len <= u.REFINE_FULL_LONG_ROW)))
    mutants = [("skip_row", r, k) for k, r in rows.items()] + [("stale_upper", None, ""), ("shift_rows", None, "")]
    if name == "long_row":
        long_row = int(np.argmax(ref.row_len))
        mutants += [("skip_row", long_row, "long"), ("long_row_missing", long_row, "")]
    for mutant, row, what in mutants:
        X1 = u.refine_fp64(ref, ref.X0_ref, 1, mutant, row)
        q1 = ref.ratios_once(X1)
        q2 = ref.ratios_twice(u.refine_fp64(ref, X1, 1, mutant, row))
        print(f"refine-mutant block={name} {mutant} {what} once={q1.min():.3g} twice={q2.min():.3g}")
        assert not ref.corrected_once(X1, M_CAP).any(), (mutant, what, q1)
        assert (q2 > M_CAP).all(), (mutant, what, q2)


@pytest.mark.parametrize("mode", [0, 1], ids=["rhs_norm", "backward_error"])
@pytest.mark.parametrize("worst", u.REFINE_BATCH_WORST)
def test_batch_measure_and_its_mutants(worst, mode):
    refs = u.refine_batch_references(worst)
    its = [[getattr(r, k)[0] for r in refs] for k in ("X0_ref", "X1_ref", "X2_ref")]
    (eta0, s0), (eta1, s1), (eta2, s2) = (u.refine_batch_measure(refs, xs, mode) for xs in its)
    per_block = [r.measures(r.X0_ref, mode)[0] for r in refs]
    print(f"refine-measure worst={worst} mode={mode} eta0={eta0:.4g} eta1={eta1:.4g} eta2={eta2:.4g} slack={s0:.3g}")
    assert int(np.argmax(per_block)) == worst and per_block[worst] > 4 * sorted(per_block)[-2]        # the rotation puts the worst block where it says
    assert eta0 + s0 < 1.0                                    # tol = 1: no step
    assert eta1 - s1 > 1e-9 and eta2 < eta1 / 8 < eta0 / 64   # tol = 1e-9: the second step is taken (the docstring on eta2)
    for xs in its[:2]:
        assert u.refine_measure_close(u.refine_measure_fp64(refs, xs, mode), refs, xs, mode)
    for mutant in ("worst_block_dropped", "second_largest_row") + (("x_norm_missing",) if mode == 1 else ()):
        dev = u.refine_measure_fp64(refs, its[0], mode, mutant)
        assert not u.refine_measure_close(dev, refs, its[0], mode), (mutant, dev, eta0, s0)


def test_big_block_measure():
    ref = u.refine_block_reference("big", u.REFINE_EPS_WORST)
    assert ref.n >= 16384
    for mode in (0, 1):
        etas = [u.refine_batch_measure([ref], [X[0]], mode) for X in (ref.X0_ref, ref.X1_ref, ref.X2_ref)]
        print(f"refine-measure big mode={mode} " + " ".join(f"{e:.4g}" for e, _ in etas))
        assert etas[0][0] + etas[0][1] < 1.0 and etas[1][0] - etas[1][1] > 1e-9 and etas[2][0] < etas[1][0] / 8
        assert not u.refine_measure_close(u.refine_measure_fp64([ref], [ref.X0_ref[0]], mode, "second_largest_row"), [ref], [ref.X0_ref[0]], mode)


_MULTI_CASES = [(nrhs, s) for nrhs in u.REFINE_MULTI_NRHS for s in ("all", "none", "one", "mixed")] + \
               [(257, "first_chunk"), (257, "second_chunk"), (33, "all_entries")]


@pytest.mark.parametrize("nrhs,dirty_set", _MULTI_CASES, ids=[f"{n}-{s}" for n, s in _MULTI_CASES])
def test_column_choice_inputs_and_mutants(nrhs, dirty_set):
    ref = u.refine_multi_reference(nrhs, dirty_set)
    prob = u.refine_multi_problem()
    n = prob.n_leaf
    assert ref.inertia == (prob.n_i, prob.my_i, 0)
    kinds = np.array(ref.kinds)
    dirty = kinds == "dirty"
    assert np.array_equal(ref.eta0 > ref.tau, dirty)
    if dirty.any() and (~dirty).any():                          # condition 2
        assert ref.eta0[dirty].min() >= u.REFINE_COLUMN_GAP * ref.eta0[~dirty].max(), (ref.eta0[dirty].min(), ref.eta0[~dirty].max())
    if dirty_set == "all_entries":                              # condition 1, every row of every column
        sig = ref.signal_over_noise()
        print(f"refine-input multi all_entries signal/noise={sig.min():.3g}")
        assert (sig >= u.REFINE_SIGNAL).all(), sig.min()
        assert np.count_nonzero(ref.E) >= len(ref.E) - 2
    else:                                                       # E lives on J x J
        inJ = np.zeros(n, bool)
        inJ[ref.J] = True
        assert len(ref.J) == n // 2 and not np.any(ref.E[~(inJ[ref.row_of] & inJ[ref.indices])]) and np.count_nonzero(ref.E) > 0
    assert (ref.target_swap_over_noise() <= 0.25).all()
    for c in np.nonzero(kinds == "zero")[0]:
        assert not ref.B[c].any() and not ref.X0_ref[c].any() and not ref.X1_ref[c].any()
    # the reference's own verdict at M = 4: dirty columns corrected once, the others left as the first solve gave them
    want = np.where(dirty[:, None], ref.X1_ref, ref.X0_ref)
    ok, ratio = u.refine_multi_judge(ref, want, M_OWN)
    print(f"refine-own multi nrhs={nrhs} set={dirty_set} ratio={ratio.max():.3g} tau={ref.tau:.3g}")
    assert ok.all(), (np.nonzero(~ok)[0], ratio)
    # ... and the wrong choice, column by column: a dirty one left alone, a faint one corrected
    for X in (ref.X0_ref, ref.X1_ref):
        bad, _ = u.refine_multi_judge(ref, X, M_CAP)
        wrong = dirty if X is ref.X0_ref else kinds == "faint"
        assert not bad[wrong].any()
    ld = n + 5
    fix = list(np.nonzero(dirty)[0])
    X = u.refine_multi_fp64(ref, fix, ld)
    assert np.array_equal(X[:, :n], want) and np.all(X[:, n:] == 7.5)
    if fix:
        for mutant in ("neighbour_column", "stride_n"):
            Xm = u.refine_multi_fp64(ref, fix, ld, mutant)
            ok, _ = u.refine_multi_judge(ref, Xm[:, :n], M_CAP)
            hit = fix if mutant == "neighbour_column" else [c for c in fix if c > 0]      # (at distance n column 0 is still in its place)
            assert not ok[hit].any(), (mutant, ok[hit])
