"""The references of tests/test_schur_judged_gpu.py, validated with the oracle alone (no GPU).  For every problem of util.SCHUR_PROBLEMS
(and the finalised variants the sparse-root cases use):
  * the oracle's static-pivot LDL^T perturbs no pivot in any block - inertia (n_i, my_i, 0) - so SC_ref0 is the unrefined Schur contribution
    of K itself, and err_ref0 = max|SC_ref0 - SC*| measures the plain FP64 algorithm and nothing else;
  * SC_ref0 is what Problem.oracle_schur gives (one refinement step) to 1e-9: the sign convention; SC* is SC_ref0 to the same bound, and
    the per-block terms add up to the whole;
  * the predicate  max|SC - SC*| <= M max(err_ref0, 2^-53 max|SC*|)  over the lower triangle accepts SC_ref0 at M = 1 and has teeth at the
    largest margin it may ever be given (M = 64).  It rejects SC_ref0 rounded to float32 and back, and SC_ref0 with
      - one block's term left out,
      - the term of one border column of one block left out - the last column of the block's bmap, and the first column of its last chunk of
        32 (what a chunk or tile off-by-one produces),
      - one block's term scaled by 1 + 1e-6,
      - the last row zeroed where it lies past a 128-row boundary (S > 128),
      - one off-diagonal square transposed (rows 32 .. 63 against columns 0 .. 31; S < 64: the square of side S // 2 below the diagonal;
        none at S = 1) - a block whose la >= lb order is taken the wrong way;
    and 2 SC_ref0 is accepted as a contribution accumulated twice while SC_ref0 is not;
  * the per-block quotient accepts the block's own unrefined term at M = 1, and rejects it at M = 64 with a border column left out, scaled by
    1 + 1e-6, or with an entry outside the block's bmap."""
import numpy as np
import pytest

from tests import util as u

M_CAP = u.UNREFINED_M_CAP
_CASES = [(key, False) for key in u.SCHUR_PROBLEMS] + [(key, True) for key in u.SCHUR_PROBLEMS if key[1:3] == (129, 3)]


def _without_column(SC, term, c):
    """SC with block's term taken out of row c and column c (lower triangle)"""
    out = SC.copy()
    out[c, :] -= term[c, :]
    out[c + 1:, c] -= term[c + 1:, c]
    return out


@pytest.mark.parametrize("key,finalized", _CASES, ids=[f"{k[0]}-S{k[1]}-N{k[2]}-{k[3]}{'-finalized' if f else ''}" for k, f in _CASES])
def test_schur_reference(key, finalized):
    n_i, S, N, borders = key
    ref = u.schur_reference(key, finalized)
    prob = ref.prob
    assert (prob.n_i, prob.my_i, prob.S, prob.N) == (n_i, n_i // 2, S, N) and prob.n0 == S // 2
    assert ref.inertia == [(prob.n_i, prob.my_i, 0)] * N, ref.inertia                     # no perturbed pivot
    # bmaps: every column in every block, or (hetero) proper subsets that differ
    full = np.arange(S)
    want_maps = [full, full[:prob.n0], full[prob.n0:]] if borders == "hetero" else [full] * N
    assert all(np.array_equal(a, b) for a, b in zip(ref.bmaps, want_maps))
    assert np.isfinite(ref.SC_star).all() and np.isfinite(ref.SC_ref0).all() and ref.scale > 0.0 and ref.err_ref0 > 0.0
    want = prob.oracle_schur()
    if finalized:
        want = prob.oracle_finalize(want)
    want = np.tril(want)
    assert np.abs(ref.SC_ref0 - want).max() <= 1e-9 * np.abs(want).max()
    assert np.abs(ref.SC_star - want).max() <= 1e-9 * np.abs(want).max()
    if not finalized:
        assert np.abs(sum(ref.block_star) - ref.SC_star).max() <= 4 * N * u.UNIT_ROUNDOFF * ref.scale
        assert np.abs(sum(ref.block_ref0) - ref.SC_ref0).max() <= 4 * N * u.UNIT_ROUNDOFF * ref.scale
    R0 = ref.SC_ref0
    assert ref.accepts(R0, 1) and ref.ratio(ref.SC_star) == 0.0
    assert ref.ratio(np.full((S, S), np.nan)) == np.inf
    # float32 rounding is visible
    r32 = ref.ratio(R0.astype(np.float32).astype(np.float64))
    assert r32 > M_CAP, (r32, ref.err_ref0 / ref.scale)
    wrong = {}
    for b in range(N):
        term, cols = ref.block_ref0[b], ref.bmaps[b]
        wrong[f"block {b} left out"] = R0 - term
        wrong[f"block {b} scaled"] = R0 + 1e-6 * term
        for c in {int(cols[-1]), int(cols[(len(cols) - 1) // 32 * 32])}:
            wrong[f"block {b} without column {c}"] = _without_column(R0, term, c)
    if S > 128:
        last = R0.copy()
        last[S - 1, :] = 0.0
        assert (S - 1) // 128 * 128 in (128, 256) and S - 1 >= 128
        wrong["last row zeroed"] = last
    k = 32 if S >= 64 else S // 2
    if k:
        sq = R0.copy()
        sq[k:2 * k, :k] = R0[k:2 * k, :k].T
        wrong["square transposed"] = sq
    for what, SC in wrong.items():
        assert not ref.accepts(SC, M_CAP), (what, ref.ratio(SC))
    assert ref.accepts(2.0 * R0, 1, times=2) and not ref.accepts(R0, M_CAP, times=2) and not ref.accepts(2.0 * R0, M_CAP)
    # the per-block quotient
    if finalized:
        return
    for b in range(N):
        term, cols = ref.block_ref0[b], ref.bmaps[b]
        assert ref.block_accepts(b, term, 1), ref.block_ratio(b, term)
        assert not ref.block_accepts(b, (1.0 + 1e-6) * term, M_CAP)
        assert not ref.block_accepts(b, _without_column(term, term, int(cols[-1])), M_CAP)
        if len(cols) < S:
            out = term.copy()
            outside = np.setdiff1d(full, cols)
            out[max(outside[0], cols[0]), min(outside[0], cols[0])] = 1e-300
            assert ref.block_ratio(b, out) == np.inf
