"""The references of tests/test_solve_compressed_judged_gpu.py, validated with the oracle, scipy and the generator alone (no GPU).  For every case
of util.ARROWHEAD_CASES:
  * the system A = [[diag(K_i), Br_i], [Br_i^T, K_0]] on [x_1 .. x_N | x0 y0 z0 ylink zlink] is symmetric, and it is the system the oracle's
    solve_compressed solves: x_ref0 lies within 1e-9 of x*, which comes from scipy's LU of A and knows nothing of Schur complements;
  * the refinement that gives x* converged: a correction below 2^-58 max|x| within eight steps;
  * the oracle's unrefined leaves have the inertia (n_primal, n_leaf - n_primal, 0) - no pivot perturbed - and the root (n0, S - n0, 0);
  * the predicate (util.ArrowheadReference.accepts: backward, root rows, forward root, forward leaf, per right-hand side) accepts x_ref0 at M = 1
    and x* with forward ratios 0; the all-zero right-hand side gives exact zeros in both, and a solution of it that is not exactly zero, or
    anything non-finite, is rejected;
  * util.solve_compressed_fp64 without a mutant returns the bits of oracle.solve_compressed.
The predicate has teeth at the largest margin it may ever be given (M = 64): on both Gaussian right-hand sides of every case it rejects the
solution of x_ref0's algorithm with
  (a) every leaf solution rounded to float32,
  (b) the root right-hand side without one block's Br_i^T z_i,
  (c) the same term without that block's last non-empty border row,
  (d) the largest entry of the root right-hand side off by a relative 1e-11,
  (e) the Ltsolve reading x0 with its first and last entry swapped,
  (f) where mz0 > 0, z0 recovered without the C0 x0 term.
The cases with the generator's default diagonals (1e-4 .. 1e4) did not reject (d); their primal diagonals are narrowed to 1e-2 .. 1e2
(util._arrowhead_narrow_diagonals says why).  Two (case, mutant) pairs remain that cannot be rejected on both right-hand sides
(util.ARROWHEAD_NOT_DISTINGUISHABLE): at most one per case and none on a case whose followers go way 2 on trust, which is asserted.
One solve of the GPU module lies beyond every admissible margin (one Schur row, b0 = 0: forward_root); test_one_schur_row_exceeds_the_margin_on_its_own
restates the algorithm in plain FP64 with densely factorised leaves in three elimination orders and shows that each of them does too."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import util as u

M_CAP = u.UNREFINED_M_CAP
_GAUSSIAN = (0, 1)


def _applies(case, mutant):
    ref_free = {"z0_without_C0_x0": case == "general_mz0", "x0_entries_swapped": case != "width1"}
    return ref_free.get(mutant, True)


_PAIRS = [(c, m) for c in u.ARROWHEAD_CASES for m in u.SOLVE_COMPRESSED_MUTANTS if _applies(c, m)]


def test_the_case_table():
    assert len(set(u.ARROWHEAD_CASES)) == len(u.ARROWHEAD_CASES) and set(u.ARROWHEAD_WAY2_CASES) <= set(u.ARROWHEAD_CASES)
    assert set(u.ARROWHEAD_NOT_DISTINGUISHABLE) <= set(u.ARROWHEAD_CASES) - set(u.ARROWHEAD_WAY2_CASES)       # (a dict: at most one mutant per case)
    assert set(u.ARROWHEAD_NOT_DISTINGUISHABLE.values()) <= set(u.SOLVE_COMPRESSED_MUTANTS)
    # every mutant that has something to act on is run on every case: (f) needs z0 rows, (e) two Schur rows - the latter is width1's one exception
    for c in u.ARROWHEAD_CASES:
        left_out = [m for m in u.SOLVE_COMPRESSED_MUTANTS if (c, m) not in _PAIRS]
        sysm = u.ArrowheadSystem(*u.arrowhead_problem(c))
        assert left_out == [m for m in u.SOLVE_COMPRESSED_MUTANTS if (m == "z0_without_C0_x0" and sysm.mz0 == 0) or (m == "x0_entries_swapped" and sysm.S < 2)]
        assert "x0_entries_swapped" not in left_out or u.ARROWHEAD_NOT_DISTINGUISHABLE.get(c) == "x0_entries_swapped"


@pytest.mark.parametrize("case", u.ARROWHEAD_CASES)
def test_arrowhead_reference(case):
    ref = u.arrowhead_reference(case)
    sysm, nl = ref.sys, ref.n_leaves
    n = nl + sysm.S_full
    assert ref.A.shape == (n, n) and abs(ref.A - ref.A.T).max() == 0.0
    assert ref.B.shape == (len(u.ARROWHEAD_RHS), n)
    what = dict(zip(u.ARROWHEAD_RHS, range(len(u.ARROWHEAD_RHS))))
    assert not ref.B0[what["b0_zero"]].any() and ref.BL[what["b0_zero"]].all()
    assert not ref.BL[what["b_leaf_zero"]].any() and ref.B0[what["b_leaf_zero"]].all()
    k = what["unit_b0_last"]
    assert ref.B[k, -1] == 1.0 and np.count_nonzero(ref.B[k]) == 1 and sysm.red[-1] == sysm.S_full - 1       # the last Schur index
    assert list(ref.is_zero_rhs) == [name == "zero" for name in u.ARROWHEAD_RHS]
    # x*
    assert ref.converged and ref.refinement_steps <= ref.MAX_STEPS, ref.refinement_steps
    assert np.isfinite(ref.X_star).all() and np.isfinite(ref.X_ref0).all()
    # x_ref0: no pivot perturbed, the expected inertia, and the same system
    assert ref.leaf_inertia == [(sysm.n_primal, sysm.n_leaf - sysm.n_primal, 0)] * sysm.N
    assert ref.root_inertia == (sysm.n0, sysm.S - sysm.n0, 0)
    for part in (slice(0, nl), slice(nl, None)):
        err = np.abs(ref.X_ref0[:, part] - ref.X_star[:, part]).max(axis=1)
        assert np.all(err <= 1e-9 * np.abs(ref.X_star[:, part]).max(axis=1)), err
    z = what["zero"]
    assert not ref.X_star[z].any() and not ref.X_ref0[z].any()
    # the predicate on what it must accept ...
    assert ref.accepts(ref.X_ref0[:, nl:], ref.X_ref0[:, :nl], 1).all()
    r = ref.ratios(ref.X_star[:, nl:], ref.X_star[:, :nl])
    print(f"solve-compressed-reference case={case} n={n} steps={ref.refinement_steps} x* backward={r['backward'].max():.3g} root_rows={r['root_rows'].max():.3g}")
    assert not r["forward_root"].any() and not r["forward_leaf"].any()
    assert np.all(r["backward"] <= 1.0) and np.all(r["root_rows"] <= 1.0)
    # ... and on what it must not: a solution of the zero right-hand side that is not zero, anything non-finite
    bad = ref.X_ref0.copy()
    bad[z, nl] = 1e-300
    bad[0, nl // 2] = np.nan
    bad[1, -1] = np.inf
    assert list(ref.accepts(bad[:, nl:], bad[:, :nl], M_CAP)) == [False, False, True, True, True, False]
    assert not ref.accepts(bad[z, nl:], bad[z, :nl], M_CAP, k=z)[0] and ref.accepts(ref.X_ref0[z, nl:], ref.X_ref0[z, :nl], 1, k=z)[0]
    # the restatement the mutants are made from is the oracle's algorithm to the bit
    for k in range(len(ref.B)):
        x0, xl = ref.mutant(k, None)
        assert np.array_equal(x0, ref.X_ref0[k, nl:]) and np.array_equal(xl, ref.X_ref0[k, :nl])


def test_second_factorisation_is_another_system():
    """group 9 of the GPU module factorises with 1.3 x the leaf diagonals: its reference is rebuilt, and the first one does not hold for it"""
    first, second = u.arrowhead_reference("small"), u.arrowhead_reference("small_scaled")
    assert first.sys.prob is second.sys.prob and second.sys.diag_scale == u.ARROWHEAD_SECOND_DIAG_SCALE
    d1, d2 = first.A.diagonal(), second.A.diagonal()
    nl = first.n_leaves
    assert np.array_equal(d2[:nl], u.ARROWHEAD_SECOND_DIAG_SCALE * d1[:nl]) and np.array_equal(d2[nl:], d1[nl:])
    assert abs((first.A - second.A)).max() == np.abs(d2 - d1).max()                       # (nothing but the leaf diagonals differs)
    X = second.X_ref0
    assert not first.accepts(X[:, nl:], X[:, :nl], M_CAP)[:5].any()


@pytest.mark.parametrize("case,mutant", _PAIRS, ids=[f"{c}-{m}" for c, m in _PAIRS])
def test_the_predicate_rejects_the_mutants(case, mutant):
    ref = u.arrowhead_reference(case)
    rejected = []
    for k in _GAUSSIAN:
        x0, xl = ref.mutant(k, mutant)
        r = ref.ratios(x0, xl, k)
        print(f"solve-compressed-mutant case={case} {mutant} rhs={u.ARROWHEAD_RHS[k]}: " + " ".join(f"{name}={float(v[0]):.3g}" for name, v in r.items()))
        rejected.append(not ref.accepts(x0, xl, M_CAP, k)[0])
    if u.ARROWHEAD_NOT_DISTINGUISHABLE.get(case) == mutant:
        assert any(rejected) and case not in u.ARROWHEAD_WAY2_CASES, rejected
    else:
        assert all(rejected), rejected


class _DenseLeaf:
    """K_i x = b by the unblocked FP64 LDL^T of the dense K_i in a given elimination order (util.dense_root_ldl_static): the leaf solver the
    oracle's Schur assembly and solve_compressed_fp64 ask for, with nothing of the device in it"""

    def __init__(self, K_full, perm):
        self.perm = np.asarray(perm)
        self.L, self.d = u.dense_root_ldl_static(K_full[np.ix_(self.perm, self.perm)])

    def solve(self, x):
        X = np.atleast_2d(x)
        X[:, self.perm] = u.dense_root_ldl_solve(self.L, self.d, X[:, self.perm])
        return x


def test_one_schur_row_exceeds_the_margin_on_its_own():
    """tests/test_solve_compressed_judged_gpu.py keeps width1 / all_tail / b0 = 0 as a strict expected failure: the device measures forward_root
    41.6 there.  That lies in the measure, not in a kernel.  With one Schur row the root part is one number, and x_ref0's error in it on that
    right-hand side happens to be 2.4e-15 of it, where it is 1e-14 .. 1e-13 on the other four.  The same algorithm in plain FP64 on the CPU with
    the leaves factorised densely - in the given order, in the reverse order, and in the order of the device's all-tail cut - misses every
    admissible margin on that number too (4 x the ratio is above 64), and stays within 8 on everything else."""
    import pips_ipmpp_amd as pa
    ref = u.arrowhead_reference("width1")
    s, nl = ref.sys, ref.n_leaves
    assert s.S == 1 and s.N == 1
    k_bad = u.ARROWHEAD_RHS.index("b0_zero")
    rel = np.abs(ref.X_ref0[:5, nl:] - ref.X_star[:5, nl:]).max(axis=1) / np.abs(ref.X_star[:5, nl:]).max(axis=1)
    assert rel[k_bad] == rel.min() and rel[k_bad] < 2.0 ** -48 and np.median(rel) > 4.0 * rel[k_bad], rel
    Kl = s.K_lower(0)
    Kf = (Kl + u.sp.tril(Kl, -1).T).toarray()
    n = Kf.shape[0]
    orders = {"given": np.arange(n), "reverse": np.concatenate([np.arange(s.n_primal)[::-1], np.arange(s.n_primal, n)[::-1]]),
              "all_tail": pa.symbolic_probe(s.prob.blocks[0]["K"], s.n_primal, force_n_head=0, want_perm=True)["perm"]}
    for name, perm in orders.items():
        assert sorted(perm) == list(range(n))
        leaf = _DenseLeaf(Kf, perm)
        root = orc.DenseRootSolver(1)
        root.matrixChanged(np.tril(s.finalize(orc.add_term_to_schur_compl_blocked(np.zeros((1, 1)), leaf, ref.Bts[0]), with_C0=True)))
        for k in range(len(ref.B)):
            x0, xl = u.solve_compressed_fp64(s, [leaf], ref.Bts, root, ref.B0[k], ref.BL[k])
            r = {key: float(v[0]) for key, v in ref.ratios(x0, xl, k).items()}
            print(f"solve-compressed-dense-leaf order={name} rhs={u.ARROWHEAD_RHS[k]} " + " ".join(f"{key}={v:.3g}" for key, v in r.items()))
            if k == k_bad:
                assert r["forward_root"] > 16.0 and max(r["backward"], r["root_rows"], r["forward_leaf"]) <= 8.0, (name, r)
            else:
                assert max(r.values()) <= 8.0, (name, k, r)


def test_the_mutants_are_defects_of_one_step_each():
    """what each mutant changes, on the small case: (b) and (c) leave the leaf right-hand sides' own solves alone and change x0; with b_leaf = 0
    they change nothing (z_i = 0); (d) moves x0 by a relative 1e-11 at most times the root's condition; (e) leaves x0 as it is"""
    ref = u.arrowhead_reference("small")
    nl = ref.n_leaves
    k = u.ARROWHEAD_RHS.index("b_leaf_zero")
    for mutant in ("block_term_left_out", "border_row_dropped"):
        x0, xl = ref.mutant(k, mutant)
        assert np.array_equal(x0, ref.X_ref0[k, nl:]) and np.array_equal(xl, ref.X_ref0[k, :nl])
        x0, xl = ref.mutant(0, mutant)
        assert not np.array_equal(x0, ref.X_ref0[0, nl:])
    x0, xl = ref.mutant(0, "x0_entries_swapped")
    assert np.array_equal(x0, ref.X_ref0[0, nl:]) and not np.array_equal(xl, ref.X_ref0[0, :nl])
    x0, xl = ref.mutant(0, "root_rhs_entry_off")
    rel = np.abs(x0 - ref.X_ref0[0, nl:]).max() / np.abs(ref.X_ref0[0, nl:]).max()
    assert 0.0 < rel <= 1e-11 * np.linalg.cond(ref.SC_ref0 + np.tril(ref.SC_ref0, -1).T)
    x0, xl = ref.mutant(0, "float32_leaves")
    assert np.array_equal(x0, ref.X_ref0[0, nl:]) and np.array_equal(xl, ref.X_ref0[0, :nl].astype(np.float32).astype(np.float64))
    z = u.arrowhead_reference("general_mz0")
    x0, xl = z.mutant(0, "z0_without_C0_x0")
    same = np.ones(z.sys.S_full, bool)
    same[z.sys.z0_rows] = False
    assert np.array_equal(x0[same], z.X_ref0[0, z.n_leaves:][same]) and not np.array_equal(x0, z.X_ref0[0, z.n_leaves:])
    assert isinstance(z.root0, orc.DenseRootSolver)
