"""The static pivot rule when it rejects a pivot: replaced pivots, counts, and the factors they leave.

Every other judged module runs cases in which no pivot is rejected.  Here every case rejects some, and two facts carry the checks:
  1. a right-looking LDL^T whose pivot k is replaced by d'_k is the exact factorisation of K' = K + (d'_k - d_k) e_k e_k^T, d_k the pivot as it
     stood - so the device's factors, used WITHOUT refinement, must solve K' x = b, and the predicates of UnrefinedReference / DenseRootReference
     apply with K' in place of K;
  2. K' is known exactly only where d_k is: solves are judged on cases whose rejected rows have no pattern neighbour eliminated earlier (the
     pivot stands as the matrix entry; proved from the probe's perm in tests/test_pivot_rule_reference_cpu.py), cancellation cases
     (duplicate rows of W) on counts and decisions only.
The reference is util.PivotRuleReference: a long-double LDL^T of P K P^T in the device's order under the rule restated from the kernels.  The CPU
module proves for every case the exactness, decision margins of 64 either way, that the oracle perturbs nothing on K', and that the table tells
eight mutant rules from the right one.

Cases (util.PIVOT_LEAF_TABLE, util.PIVOT_ROOT_CASES; n <= 600 everywhere):
  leaf 400 / 200, random W (head 344 of simple leaves + tail 256) and banded W (fronts): dead_primal (zero diagonal, zero column of W: K'_jj = repl_abs,
  x_j = b_j / repl_abs), dead_dual (a dual row with a zero diagonal and stored zeros in W: K'_jj = -repl_abs), free_primal (zero diagonal, coupled), wrong_sign_primal (-2^-3: hinted K'_jj = +repl_rel 2^-3; unhinted accepted, the triple
  is the eigenvalue count), duplicate_rows (equal rows of W, zero dual diagonal: the later row of a pair lands inside the head, and in the tail on
  in-tile columns 0, 31, 32, 127 with one of them in a tile other than the first), duplicate_rows_wrong_sign (the same with a replaced head pivot
  whose update makes the tail's refreshed reference magnitude the one that counts); two_blocks: three leaves of 170 / 85 (all head) in one batch,
  dead_primal in block 0, nothing in block 1, duplicate_rows in block 2 - workgroups of k_head_factor_simple straddle the blocks.
  dense root, quasi-definite, n in {129, 300, 513}: dead rows at 0, 31, 32, 96, 127, 128 (every 32-wide sub-block of the blocked diagonal tile fails
  once, tile 1 restarts too); one wrong-sign primal row p in {0, 32, 128} coupled to dual rows only.
Paths: cuts model / all head / all tail x head variants PIPS_HIP_MF=0 (k_head_factor / k_head_factor_simple by scatter), default (fronts, k_front),
PIPS_HIP_MF_KONLY=1 x tail forms PIPS_HIP_TAIL_SINGLE=0 (k_tile_diag) and =1 (k_tail_ldl: blocked tile, restart, careful kernel; asserted from the
phase timers) x PIPS_HIP_DETERMINISTIC=1 (two fresh handles agree to the bit); the dense root's single launch, PIPS_HIP_ROOT_LAUNCHES=1,
PIPS_HIP_ROOT_DIAG_BARRIERS=1 and the column-major device entry with lda > n.  Triples are asserted exactly, per block, through LeafBatch.inertia,
HipLdlSolver.get_inertia and inertia_batch.

Measured on an MI355X, largest ratio over the cases, cuts, variants and right-hand sides of a path (backward = eta_dev / max(eta_ref, 2^-53),
forward = ||x_dev - x*|| / max(||x_ref0 - x*||, 2^-53 ||x*||), both against the plain FP64 algorithm on K'):

    path                                                              backward    forward    M
    dead_primal (batch of one, handle, two_blocks, refined)           0.0033      2.0        8
    dead_dual                                                         0.0059      2.0        8
    free_primal                                                       1.31        2.14       16
    wrong_sign_primal, hinted                                         3.29        7.74       32
    dense root, dead rows (all four entries and drivers)              1.3e-7      1.62       8
    dense root, wrong-sign row                                        2.68        3.21       16

M per path: the smallest power of two >= 4 x the larger of the two ratios.  The forward 2.0 of the dead rows is x_j = b_j / d' one ulp from the oracle's
(the yardstick there is the floor 2^-53 ||x*||); the 7.74 of wrong_sign_primal (banded W, model cut, scatter head / launch-per-step tail) comes with
multipliers near 1e9 and stays within a factor 2 of that on every path that solves the case.  Nothing lies beyond 64: no expected failure.
Default refinement on free_primal: measure 0 after 1 step (printed, not asserted).
Seeded defect (fix_pivot returning repl in place of s * repl, built apart): 34 of 220 fail - every cut and variant of dead_dual (30), its two
handle tests, and dead-n129 of the dense root on all four variants (its dead rows 96, 127, 128 are dual)."""
import numpy as np
import pytest
import scipy.sparse as sp

import pips_ipmpp_amd as pa
from tests import util as u

pytestmark = pytest.mark.gpu

# per path: the smallest power of two >= 4 x the largest measured ratio (see the table above); never above 64
M = {"dead_primal": 8, "dead_dual": 8, "free_primal": 16, "wrong_sign_primal": 32, "root_dead": 8, "root_wrong_sign": 16}
_KNOBS = ("PIPS_HIP_MF", "PIPS_HIP_MF_KONLY", "PIPS_HIP_MF_SPLIT", "PIPS_HIP_TAIL_SINGLE", "PIPS_HIP_DETERMINISTIC", "PIPS_HIP_ROOT_LAUNCHES",
          "PIPS_HIP_ROOT_DIAG_BARRIERS", "PIPS_HIP_ND_DEPTH")
_VARIANTS = {"default": {}, "scatter_head": {"PIPS_HIP_MF": "0"}, "k_only_fronts": {"PIPS_HIP_MF_KONLY": "1"},
             "tail_launches": {"PIPS_HIP_TAIL_SINGLE": "0"}, "tail_single": {"PIPS_HIP_TAIL_SINGLE": "1"}, "deterministic": {"PIPS_HIP_DETERMINISTIC": "1"}}


def _env(monkeypatch, variant):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in _VARIANTS.get(variant, {}).items():
        monkeypatch.setenv(k, v)


def _applies(variant, cut):
    if variant in ("scatter_head", "k_only_fronts"):
        return cut != "all_tail"
    if variant in ("tail_launches", "tail_single"):
        return cut != "all_head"
    return True


_BIG = [(name, shape, kind, block, cut) for name, shape, kind, block, cuts in u.PIVOT_LEAF_TABLE if shape == u.PIVOT_LEAF_SHAPE for cut in cuts]
_LEAF = [(c, v) for c in _BIG for v in _VARIANTS if _applies(v, c[4])]


def _leaf_id(c):
    name, shape, kind, block, cut = c
    return f"{name}-{kind}-{cut}"


def _case(c):
    name, shape, kind, block, cut = c
    case = u.pivot_leaf_case(name, shape, kind, cut, block)
    return case, u.pivot_leaf_reference(case, cut)


def _batch_of_one(case, cut, refine_steps=0):
    f = u.PIVOT_CUTS[cut]
    bt = pa.LeafBatch(1, 0)
    bt.set_block(0, case.K, case.hint)
    bt.set_options(force_n_head=case.n if f is None else f, refine_steps=refine_steps)
    bt.analyze(1)
    bt.set_values(0, case.K.val)
    bt.set_timing(True)
    bt.factor()
    return bt


def _solve_rows(bt, B):
    X = np.empty_like(B)
    for i in range(B.shape[0]):
        x = B[i].copy()
        bt.solve(x)
        assert bt.last_refinement_steps() == 0
        X[i] = x
    return X


def _judge_leaf(j, X, path, name):
    bw, fw = j.backward_ratios(X), j.forward_ratios(X)
    print(f"pivot-ratio path={path} backward={bw.max():.4g} forward={fw.max():.4g}")
    assert M[name] <= u.UNREFINED_M_CAP
    assert (bw <= M[name]).all(), (path, bw, j.eta_ref)
    assert (fw <= M[name]).all(), (path, fw)


def _assert_decoupled(X, B, rows, dprime, path):
    """x_j = b_j / d' within 2 ulp on rows that nothing couples"""
    for row, d in zip(rows, dprime):
        want = B[:, row] / d
        assert (np.abs(X[:, row] - want) <= 2 * np.spacing(np.abs(want))).all(), (path, row, X[:, row], want)


# ---- leaves: triples on every path, solves without refinement ----------------------------------------------------------------------------
@pytest.mark.parametrize("c,variant", _LEAF, ids=[f"{_leaf_id(c)}-{v}" for c, v in _LEAF])
def test_leaf_triple_and_unrefined_solves(c, variant, monkeypatch):
    _env(monkeypatch, variant)
    case, ref = _case(c)
    cut = c[4]
    bt = _batch_of_one(case, cut)
    info, tm = bt.info(), bt.get_timing()
    assert info["n_head"] == ref.probe["n_head"] and info["m"] == ref.probe["m"] and info["ntc"] == -(-info["m"] // 128), (info, ref.probe)
    if cut == "model":
        assert 0 < info["n_head"] < case.n and info["ntc"] == 2, info
    if cut != "all_tail":
        assert info["multifrontal_head"] == (0 if variant == "scatter_head" else 1), info
    if variant == "tail_single":        # info() does not say which tail form ran, the phase timers do
        assert tm["tail_update"][1] == 1 and tm["tail_diag"][1] == 0 and tm["tail_trsm"][1] == 0, tm
    elif variant == "tail_launches":
        assert tm["tail_diag"][1] >= 1 and tm["tail_trsm"][1] >= 1, tm
    assert bt.inertia(0) == ref.triple, (bt.inertia(0), ref.triple, ref.rejected_positions)
    path = f"leaf/{_leaf_id(c)}/{variant}"
    X = None
    if case.solve_judged:
        j = u.pivot_leaf_judge(case, cut)
        X = _solve_rows(bt, j.B)
        _judge_leaf(j, X, path, case.name)
        if case.decoupled:
            _assert_decoupled(X, j.B, ref.rejected_rows, ref.dprime[ref.rejected_positions], path)
    if variant == "deterministic":      # two fresh handles agree to the bit: triple and solution
        B = u.pivot_rhs(case.n, ref.rejected_rows)
        X = _solve_rows(bt, B) if X is None else X
        bt2 = _batch_of_one(case, cut)
        assert bt2.inertia(0) == ref.triple
        assert np.array_equal(_solve_rows(bt2, B), X, equal_nan=True)
        bt2.close()
    bt.close()


_HANDLE = [c for c in _BIG if c[4] == "model"]


@pytest.mark.parametrize("c", _HANDLE, ids=[_leaf_id(c) for c in _HANDLE])
def test_handle_order_is_the_probes_and_its_triple_the_references(c, monkeypatch):
    """HipLdlSolver: get_perm() is the perm of symbolic_probe for the same K and hint - the reference's order is the device's - and get_inertia()
    the reference's triple; the unrefined solve is judged like the batch's."""
    _env(monkeypatch, "default")
    case, ref = _case(c)
    s = pa.HipLdlSolver(case.K, n_primal=case.hint, refine_steps=0)
    s.matrixChanged()
    info = s.info()
    assert np.array_equal(s.get_perm(), ref.probe["perm"])
    assert info["n_head"] == ref.probe["n_head"] and info["m"] == ref.probe["m"], info
    assert s.get_inertia() == ref.triple
    if case.solve_judged:
        j = u.pivot_leaf_judge(case, "model")
        X = j.B.copy()
        s.solve(X)
        assert s.info()["last_refinement_steps"] == 0
        _judge_leaf(j, X, f"handle/{_leaf_id(c)}", case.name)
    s.close()


# ---- two_blocks: per-block counts in a batch whose simple-leaf workgroups straddle the blocks -------------------------------------------
@pytest.mark.parametrize("variant", ["default", "scatter_head", "deterministic"])
def test_three_block_batch_counts_per_block(variant, monkeypatch):
    _env(monkeypatch, variant)
    cases = [u.pivot_leaf_case(name, shape, kind, cut, block) for name, shape, kind, block, (cut,) in u.PIVOT_TWO_BLOCKS]
    refs = [u.pivot_leaf_reference(case, "model") for case in cases]
    want = [r.triple for r in refs]
    assert want[0][2] == 3 and want[1] == (170, 85, 0) and want[2][2] >= 3 and want[2][0] == 170       # dead primal rows / nothing / duplicate dual rows
    bt = pa.LeafBatch(3, 0)
    for b, case in enumerate(cases):
        bt.set_block(b, case.K, case.hint)
    bt.set_options(refine_steps=0)
    bt.analyze(2)
    for b, case in enumerate(cases):
        bt.set_values(b, case.K.val)
    bt.factor()
    info = bt.info()
    assert info["n_head"] == sum(r.probe["n_head"] for r in refs) == 3 * 255 and info["m"] == 0, info
    assert [bt.inertia(b) for b in range(3)] == want
    # block 0 alone is judged: its rows of the batch's solution solve K'_0 x = b
    j = u.pivot_leaf_judge(cases[0], "model")
    X = np.zeros((j.B.shape[0], 3, 255))
    for i in range(j.B.shape[0]):
        x = np.concatenate([j.B[i], np.zeros(2 * 255)])
        bt.solve(x)
        assert bt.last_refinement_steps() == 0
        X[i] = x.reshape(3, 255)
    bt.close()
    assert not X[:, 1:].any()
    _judge_leaf(j, X[:, 0], f"two_blocks/{variant}", "dead_primal")
    _assert_decoupled(X[:, 0], j.B, refs[0].rejected_rows, refs[0].dprime[refs[0].rejected_positions], "two_blocks")
    if variant == "default":           # the array of handles: the same engine behind factor_schur_batch, counts through inertia_batch
        solvers = [pa.HipLdlSolver(case.K, n_primal=case.hint, refine_steps=0) for case in cases]
        pa.HipLdlSolver.factor_schur_batch(solvers)
        assert pa.HipLdlSolver.inertia_batch(solvers) == want
        for s in solvers:
            s.close()


# ---- a second factorisation on the same handle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dead_primal", "dead_dual", "free_primal", "wrong_sign_primal"])
@pytest.mark.parametrize("kind", ["random", "time_coupled"])
def test_counts_follow_the_values_from_factorisation_to_factorisation(name, kind, monkeypatch):
    """perturbed values, values that perturb nothing, perturbed again: the counters and the cached count start over each time"""
    _env(monkeypatch, "default")
    case, ref = _case((name, u.PIVOT_LEAF_SHAPE, kind, 0, "model"))
    clean = u.pivot_leaf_case("clean", u.PIVOT_LEAF_SHAPE, kind, "model", 0)
    assert np.array_equal(clean.K.colidx, case.K.colidx) and np.array_equal(clean.K.rowptr, case.K.rowptr)
    bt = _batch_of_one(case, "model")
    assert bt.inertia(0) == ref.triple and ref.triple[2] > 0
    for K, want in ((clean.K, (case.n_i, case.my_i, 0)), (case.K, ref.triple), (clean.K, (case.n_i, case.my_i, 0))):
        bt.set_values(0, K.val)
        bt.factor()
        assert bt.inertia(0) == want
    bt.close()


@pytest.mark.parametrize("name", ["duplicate_rows", "free_primal"])
def test_regularisation_restores_the_inertia_at_the_first_try(name, monkeypatch):
    """add_regularization(1e-6, 1e-6): the reference on the regularised values rejects nothing (margins of 64), and the device agrees"""
    _env(monkeypatch, "default")
    case, ref = _case((name, u.PIVOT_LEAF_SHAPE, "random", 0, "model"))
    reg = sp.diags(np.concatenate([np.full(case.n_i, 1e-6), np.full(case.my_i, -1e-6)]))
    ref_reg = u.PivotRuleReference((case.K_scipy() + reg).tocsr(), case.hint, ref.probe["perm"], ref.probe["n_head"])
    assert ref_reg.triple == (case.n_i, case.my_i, 0) and ref_reg.ratio.min() >= 64 * u.PIVOT_THR_REL
    bt = _batch_of_one(case, "model")
    assert bt.inertia(0) == ref.triple and ref.triple[2] > 0
    bt.add_regularization(1e-6, 1e-6)
    bt.factor()
    assert bt.inertia(0) == (case.n_i, case.my_i, 0)
    bt.close()


# ---- the dense root ---------------------------------------------------------------------------------------------------------------------
_ROOT_VARIANTS = {"single_launch": {}, "launches": {"PIPS_HIP_ROOT_LAUNCHES": "1"}, "diag_barriers": {"PIPS_HIP_ROOT_DIAG_BARRIERS": "1"},
                  "device_column_major": {}}


def _root_id(c):
    return f"{c[0]}-n{c[1]}" + ("" if c[2] is None else f"-p{c[2]}")


@pytest.mark.parametrize("variant", list(_ROOT_VARIANTS))
@pytest.mark.parametrize("c", u.PIVOT_ROOT_CASES, ids=[_root_id(c) for c in u.PIVOT_ROOT_CASES])
def test_root_triple_and_solves(c, variant, monkeypatch):
    import torch
    _env(monkeypatch, None)
    for k, v in _ROOT_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    ref, j = u.pivot_root_reference(c)
    n = ref.n
    s = pa.HipDenseLdlSolver(n, n_primal=ref.n_primal)
    if variant == "device_column_major":       # entry (r, c) at r + c lda, lower triangle authoritative, other finite numbers above it and behind a column
        lda = n + 3
        A = torch.full((n, lda), 7.5, dtype=torch.float64, device="cuda")
        A[:, :n] = torch.tensor(np.ascontiguousarray(u.dense_root_with_garbage_above(ref.M, 11).T), device="cuda")
        s.matrixChanged_dev(A, lda)
        torch.cuda.synchronize()
    else:
        s.matrixChanged(np.ascontiguousarray(np.tril(ref.M)))
    assert s.get_inertia() == ref.triple, (s.get_inertia(), ref.triple)
    assert s.info()["single_launch"] == (0 if variant == "launches" else 1), s.info()
    X = j.B.copy()
    s.solve(X)
    s.close()
    fw, bw = j.ratios(X, mode=0)
    path = f"root/{_root_id(c)}/{variant}"
    print(f"pivot-ratio path={path} backward={bw.max():.4g} forward={fw.max():.4g}")
    m = M["root_" + c[0]]
    assert m <= u.UNREFINED_M_CAP
    assert (bw <= m).all() and (fw <= m).all(), (path, bw, fw)
    if c[0] == "dead":
        _assert_decoupled(X, j.B, ref.rejected_rows, ref.dprime[ref.rejected_positions], path)


# ---- solves with the default refinement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "time_coupled"])
def test_refined_solve_of_dead_rows_is_that_of_the_matrix_without_them(kind, monkeypatch):
    """A right-hand side that is zero on the rejected (decoupled) rows: x is exactly zero there, and elsewhere the handle's answer under its
    default refinement is judged against the refined oracle on K with those rows and columns deleted."""
    _env(monkeypatch, "default")
    case, ref = _case(("dead_primal", u.PIVOT_LEAF_SHAPE, kind, 0, "model"))
    keep = np.setdiff1d(np.arange(case.n), ref.rejected_rows)
    Kl = case.K_scipy()
    Kf = (Kl + sp.tril(Kl, -1).T).tocsr()
    Kred = sp.tril(Kf[keep][:, keep]).tocsr()
    B = np.random.default_rng(8).standard_normal((1, case.n))
    B[:, ref.rejected_rows] = 0.0
    j = u.UnrefinedReference(u._OneLeafMatrix(Kred, case.n_i - len(ref.rejected_rows)), 0, B[:, keep])
    assert j.inertia == (case.n_i - len(ref.rejected_rows), case.my_i, 0)
    s = pa.HipLdlSolver(case.K, n_primal=case.hint)
    s.matrixChanged()
    assert s.get_inertia() == ref.triple
    x = B[0].copy()
    s.solve(x)
    steps = s.info()["last_refinement_steps"]
    s.close()
    assert not x[ref.rejected_rows].any()
    _judge_leaf(j, x[keep][None, :], f"refined/dead_primal/{kind}/steps{steps}", "dead_primal")


def test_refined_solve_of_free_rows_reports_its_measure(monkeypatch):
    """free_primal under the default refinement: the measure and the steps are printed, nothing about what refinement recovers from the factors of K'
    is asserted (the harness's outer solve owns that) beyond a finite answer and an exact triple"""
    _env(monkeypatch, "default")
    case, ref = _case(("free_primal", u.PIVOT_LEAF_SHAPE, "random", 0, "model"))
    bt = _batch_of_one(case, "model", refine_steps=-1)
    assert bt.inertia(0) == ref.triple
    x = u.pivot_rhs(case.n, ref.rejected_rows)[0].copy()
    x[ref.rejected_rows] = 0.0
    bt.solve(x)
    print(f"pivot-refined free_primal: measure {bt.last_refinement_measure():.3g}, steps {bt.last_refinement_steps()}")
    bt.close()
    assert np.isfinite(x).all()
