"""The case table of tests/test_pivot_rule_gpu.py and its reference (util.PivotRuleReference), proved on the host: no GPU.

For every case of the table (util.PIVOT_LEAF_TABLE at each of its cuts, util.PIVOT_ROOT_CASES):
  (a) exactness - where solves are judged, no pattern neighbour of a rejected row is eliminated before it (read from the probe's perm: the
      device's order), the pivot the reference sees there is the matrix entry bit for bit, and K' carries d' bit for bit; the rows the
      construction meant to have rejected are the rows the reference rejects (duplicate_rows: the wanted in-tile columns, through the probe);
  (b) decision margins - accepted pivots have s d >= 64 thr_rel pref, rejected ones s d <= thr_rel pref / 64, in the long-double reference and
      in a plain FP64 restatement that sums every pivot in the reverse order and multiplies by the rounded reciprocal: no decision hangs on a
      rounding, whatever order a kernel sums in;
  (c) the oracle (OracleLdl, and the static FP64 LDL^T of the dense root) perturbs nothing on K', its refined solve has converged - one more
      step moves it by less than a quarter of the yardstick it serves in - and agrees with the long-double factors' own solve within it;
  (d) discrimination - each mutant of util.PIVOT_MUTANTS changes a triple or K', or has its unrefined solution rejected at M = 64, somewhere.
"""
import numpy as np
import pytest

from tests import util as u

_LEAF = [(name, shape, kind, block, cut) for name, shape, kind, block, cuts in u.PIVOT_LEAF_TABLE for cut in cuts]


def _leaf_id(c):
    name, shape, kind, block, cut = c
    return f"{name}-{kind}{shape[0]}-b{block}-{cut}"


def _root_id(c):
    return f"{c[0]}-n{c[1]}" + ("" if c[2] is None else f"-p{c[2]}")


def _assert_margins(ref, tag):
    acc = ref.accepted
    lo = ref.ratio[acc].min() if acc.any() else np.inf
    hi = ref.ratio[~acc].max() if (~acc).any() else -np.inf
    print(f"pivot-margin {tag}: smallest accepted s d / pref = {lo:.3g}, largest rejected = {hi:.3g}")
    assert lo >= 64 * u.PIVOT_THR_REL, (tag, lo)
    assert hi <= u.PIVOT_THR_REL / 64, (tag, hi)


@pytest.mark.parametrize("c", _LEAF, ids=[_leaf_id(c) for c in _LEAF])
def test_leaf_case(c):
    name, shape, kind, block, cut = c
    case = u.pivot_leaf_case(name, shape, kind, cut, block)
    ref = u.pivot_leaf_reference(case, cut)
    n_i, my_i, n = case.n_i, case.my_i, case.n
    perm, pos = ref.perm, np.empty(n, np.int64)
    pos[ref.perm] = np.arange(n)
    assert ref.probe["n_head"] + ref.probe["m"] == n and sorted(perm) == list(range(n))
    # the rows the construction means are the rows the rule rejects, and the triple follows from them
    assert np.array_equal(np.sort(ref.rejected_rows), case.meant_rows), (ref.rejected_rows, case.meant_rows)
    if name == "wrong_sign_primal_unhinted":       # accepted and counted as it stands: the triple is the eigenvalue count of K
        Kd = ref.K_lower.toarray()
        ev = np.linalg.eigvalsh(np.tril(Kd) + np.tril(Kd, -1).T)
        assert np.abs(ev).min() > 1e-8 * np.abs(ev).max()
        assert ref.triple == (int((ev > 0).sum()), int((ev < 0).sum()), 0)
    else:
        k = len(case.meant_rows)
        primal = int((case.meant_rows < n_i).sum())
        assert ref.triple == (n_i - primal, my_i - (k - primal), k)
    if name.startswith("duplicate_rows"):          # which positions were hit: every wanted in-tile column where there is a tail, three head pivots otherwise
        tail = ref.rejected_positions[ref.rejected_positions >= ref.n_head] - ref.n_head
        if ref.probe["m"] > 0:
            assert set(tail % u.DENSE_ROOT_TILE) >= set(u.PIVOT_WANTED_TILE_COLUMNS), tail
            assert len(set(tail // u.DENSE_ROOT_TILE)) >= 2 and (tail // u.DENSE_ROOT_TILE > 0).any(), tail          # a tile other than the first
            assert ((tail % u.DENSE_ROOT_TILE == 0) & (tail > 0)).any()
        else:
            assert len(ref.rejected_positions) >= 3 and (case.meant_rows >= n_i).all()
    # (a)
    if case.solve_judged:
        Kf = ref.K_lower + ref.K_lower.T
        for k, row in zip(ref.rejected_positions, ref.rejected_rows):
            nb = Kf[row].indices
            # no neighbour in the pattern is eliminated earlier - or (dead_dual) those that are hold a stored zero in this row: their updates are exact zeros
            assert all(pos[j] > k or Kf[row, j] == 0.0 for j in nb if j != row), (row, k)
            assert ref.stood[k] == ref.exact_entry[k] == ref.K_lower[row, row]
            assert ref.Kp_lower[row, row] == ref.dprime[k]
            want = ref.repl_abs if ref.pref[k] == 0.0 else u.PIVOT_REPL_REL * ref.pref[k]
            assert want > 0.0 and ref.dprime[k] == (want if row < n_i else -want)         # s: the hint's sign
        assert ref.repl_abs == u.PIVOT_REPL_REL * np.abs(case.K.val).max()
    # (b)
    _assert_margins(ref, _leaf_id(c) + "/long double")
    plain = u.pivot_leaf_reference(case, cut, variant="left_reverse")
    _assert_margins(plain, _leaf_id(c) + "/FP64 reversed")
    assert np.array_equal(plain.accepted, ref.accepted) and plain.triple == ref.triple
    # (c)
    if case.solve_judged and case.hint >= 0:
        j = u.pivot_leaf_judge(case, cut)
        npos = int((ref.dprime[~ref.accepted] > 0).sum())
        assert j.inertia == (ref.triple[0] + npos, ref.triple[1] + ref.triple[2] - npos, 0)
        yard = np.maximum(j.fwd_ref, u.UNIT_ROUNDOFF * j.xs_norm)
        X3 = j.prob.oracle_leaf(0, refine_steps=3).solve(j.B.copy())
        Xld = ref.solve(j.B)
        print(f"pivot-oracle {_leaf_id(c)}: third step / yardstick {(np.abs(X3 - j.XS).max(axis=1) / yard).max():.3g}, "
              f"long double / yardstick {(np.abs(Xld - j.XS).max(axis=1) / yard).max():.3g}, eta_ref {j.eta_ref.max():.3g}")
        assert (np.abs(X3 - j.XS).max(axis=1) <= 0.25 * yard).all()
        assert (np.abs(Xld - j.XS).max(axis=1) <= yard).all()
        assert j.accepts(j.X0, 1).all()


@pytest.mark.parametrize("c", u.PIVOT_ROOT_CASES, ids=[_root_id(c) for c in u.PIVOT_ROOT_CASES])
def test_root_case(c):
    ref, j = u.pivot_root_reference(c)
    n, n_primal = ref.n, ref.n_primal
    assert np.array_equal(ref.rejected_rows, ref.meant_rows)
    k, primal = len(ref.meant_rows), int((ref.meant_rows < n_primal).sum())
    assert ref.triple == (n_primal - primal, n - n_primal - (k - primal), k)
    if c[0] == "dead":       # every sub-block of the blocked diagonal tile fails once, at its edge and inside, and a tile other than the first restarts
        assert set(ref.rejected_positions % 128 // 32) == {0, 1, 3} | ({0} if n > 128 else set()) and (ref.rejected_positions >= 128).any()
    dmax = np.abs(np.diag(ref.M)).max()
    assert dmax > 1.0 and ref.repl_abs == u.PIVOT_REPL_REL * dmax          # (above the 1 on the padding's diagonal, which the maximum also sees)
    # (a)
    for kk in ref.rejected_positions:
        assert not ref.M[kk, :kk].any()                                  # nothing eliminated earlier reaches the row
        assert ref.stood[kk] == ref.M[kk, kk]
        s = 1.0 if kk < n_primal else -1.0
        want = s * (ref.repl_abs if ref.pref[kk] == 0.0 else u.PIVOT_REPL_REL * ref.pref[kk])
        assert ref.dprime[kk] == want == ref.Kp_dense[kk, kk]
    # (b)
    _assert_margins(ref, _root_id(c) + "/long double")
    plain, _ = u.pivot_root_reference(c, variant="left_reverse")
    _assert_margins(plain, _root_id(c) + "/FP64 reversed")
    assert np.array_equal(plain.accepted, ref.accepted)
    # (c) the static FP64 LDL^T of K' in the given order meets no pivot the rule would reject, and x* has converged
    pref = np.abs(np.diag(ref.Kp_dense))
    sd = np.where(np.arange(n) < n_primal, 1.0, -1.0) * j.d
    assert (sd >= 64 * u.PIVOT_THR_REL * pref).all()
    assert j.converged
    Xld = ref.solve(j.B)
    yard = np.maximum(j.fwd_ref[0], u.UNIT_ROUNDOFF * j.xs_norm)
    print(f"pivot-oracle {_root_id(c)}: long double / yardstick {(np.abs(Xld - j.X_star).max(axis=1) / yard).max():.3g}, eta_ref {j.eta_ref[0].max():.3g}")
    assert (np.abs(Xld - j.X_star).max(axis=1) <= yard).all()
    assert j.accepts(j.X_static, 1, mode=0).all()


# (d): where each mutant is looked for - the model's cut of the leaf cases (the tail's refresh happens there), the all-head cut of duplicate_rows
# (dual rows in the head), one dense root of each kind
_DISCRIMINATION_LEAF = [("dead_primal", "model"), ("free_primal", "model"), ("wrong_sign_primal", "model"), ("duplicate_rows", "model"),
                        ("duplicate_rows", "all_head"), ("duplicate_rows_wrong_sign", "model")]
_DISCRIMINATION_ROOT = [("dead", 129, None), ("wrong_sign", 129, 32)]


@pytest.mark.parametrize("mutant", u.PIVOT_MUTANTS)
def test_the_table_tells_a_mutant_rule_from_the_right_one(mutant):
    caught = []
    np.seterr(all="ignore")          # (a mutant may divide by a zero pivot: its solution is then non-finite, which the predicate rejects)
    for name, cut in _DISCRIMINATION_LEAF:
        case = u.pivot_leaf_case(name, cut=cut)
        ref = u.pivot_leaf_reference(case, cut)
        mut = u.pivot_leaf_reference(case, cut, rule=u.PivotRule(mutant=mutant))
        how = []
        if mut.triple != ref.triple:
            how.append("triple")
        if (mut.Kp_lower != ref.Kp_lower).nnz:
            how.append("K'")
        if case.solve_judged:
            j = u.pivot_leaf_judge(case, cut)
            if not j.accepts(mut.solve(j.B), u.UNREFINED_M_CAP).all():
                how.append("solve")
        if how:
            caught.append((name, cut, how))
    for c in _DISCRIMINATION_ROOT:
        ref, j = u.pivot_root_reference(c)
        mut, _ = u.pivot_root_reference(c, rule=u.PivotRule(mutant=mutant))
        how = []
        if mut.triple != ref.triple:
            how.append("triple")
        if not np.array_equal(mut.Kp_dense, ref.Kp_dense):
            how.append("K'")
        if not j.accepts(mut.solve(j.B), u.UNREFINED_M_CAP, mode=0).all():
            how.append("solve")
        if how:
            caught.append((_root_id(c), how))
    print(f"pivot-mutant {mutant}: {caught}")
    assert caught, mutant
    # tail_pref_not_refreshed and dual_pref_without_sum show in K' alone, on pivots that cancel to rounding noise: there the device's K' is known to
    # about 1e-8 only, so the GPU module cannot judge a solve on them - it pins their counts and decisions; every other mutant changes a triple
    # or fails a judged solve
    if mutant not in ("tail_pref_not_refreshed", "dual_pref_without_sum"):
        assert any("triple" in how or "solve" in how for *_, how in caught), (mutant, caught)


def test_the_right_rule_is_not_a_mutant_of_itself():
    """the reference's own unrefined solve passes the predicate it rejects the mutants with (M = 1: it is the long-double solution of K')"""
    for name, cut in _DISCRIMINATION_LEAF:
        case = u.pivot_leaf_case(name, cut=cut)
        if case.solve_judged:
            j = u.pivot_leaf_judge(case, cut)
            assert j.accepts(j.rule_ref.solve(j.B), 1).all(), (name, cut)
    for c in _DISCRIMINATION_ROOT:
        ref, j = u.pivot_root_reference(c)
        assert j.accepts(ref.solve(j.B), 1, mode=0).all(), c
