"""What tests/test_solve_multi_judged_gpu.py and tests/test_solve_multi_two_rank_gpu.py rest on, shown without a GPU.

The column sets (tests/solve_multi_cases.py): column j of a case is 2^((j // 6) mod 11) times base column j mod 6 of the case's shared
util.ArrowheadReference.  On `small` and `general_mz0`, for twelve columns spread over 257 (every base, every scale, both ends):
  * the oracle's solve_compressed run directly on the scaled right-hand side gives scale x X_ref0[base] bit for bit, and references built
    directly on those columns (six at a time, in the order of the bases) have that X_ref0 and scale x X_star[base] bit for bit - so judging a
    column by scaling it back and asking the shared reference is judging it against its own reference;
  * the set is what the docstring says: the seed of util.arrowhead_reference, every sixth column zero.
The predicate at M = 64 (util.UNREFINED_M_CAP) on a Gaussian column with j >= 32 (column 36, scale 2^6; its neighbour 37 is the other
Gaussian base): it rejects the six mutants of tests/test_solve_compressed_reference_cpu.py made on the scaled right-hand side, the solution
set with the two columns swapped (both columns are rejected), and the column solved with its neighbour's b0.
The planner (pips_kkt_multi_plan_probe, csrc/multiplan.h - the function KktSystem::solve_compressed_multi cuts its chunks with): the chunks
of nrhs in {0, 1, 7, 8, 31, 32, 33, 256, 257, 600}; n_total x chunk doubles within 2 GiB at n_total = 2 000 000; never fewer than 32 columns
per chunk however long the leaf vector; from = 0 means never panels."""
import numpy as np
import pytest

import pips_ipmpp_amd as pa
from oracle import oracle as orc
from tests import solve_multi_cases as smc
from tests import util as u

M_CAP = u.UNREFINED_M_CAP
CASES = ("small", "general_mz0")
J, NEIGHBOUR = 36, 37


def test_the_column_set():
    assert len(smc.SPREAD) == 12 and {smc.base(j) for j in smc.SPREAD} == set(range(6)) and min(smc.SPREAD) == 0 and max(smc.SPREAD) == smc.WIDEST - 1
    assert {(j // 6) % 11 for j in smc.SPREAD} == set(range(11))
    assert smc.base(J) == 0 and smc.base(NEIGHBOUR) == 1 and J >= 32 and smc.scale(J) == smc.scale(NEIGHBOUR) == 64.0
    assert smc.scale(65) == 2.0 ** 10 and smc.scale(66) == 1.0 and smc.scale(5) != smc.scale(6)
    for case in CASES:
        ref = u.arrowhead_reference(case)
        B0, BL = u.arrowhead_rhs(ref.sys, smc.seed(case))
        assert np.array_equal(B0, ref.B0) and np.array_equal(BL, ref.BL)
        C0, CL = smc.columns(ref, smc.WIDEST)
        assert C0.shape == (257, ref.sys.S_full) and CL.shape == (257, ref.n_leaves)
        for j in range(smc.WIDEST):
            assert np.array_equal(C0[j], 2.0 ** ((j // 6) % 11) * B0[j % 6]) and np.array_equal(CL[j], 2.0 ** ((j // 6) % 11) * BL[j % 6])
        zero = ~np.hstack([C0, CL]).any(axis=1)
        assert list(np.nonzero(zero)[0]) == list(range(5, 257, 6))
        D0, DL = smc.columns(ref, 5, first=30)
        assert np.array_equal(D0, C0[30:35]) and np.array_equal(DL, CL[30:35])


@pytest.mark.parametrize("case", CASES)
def test_scaled_columns_have_the_scaled_references(case):
    ref = u.arrowhead_reference(case)
    s, nl = ref.sys, ref.n_leaves
    C0, CL = smc.columns(ref, smc.WIDEST)
    cols = list(smc.SPREAD)
    for j in cols:      # the oracle itself on the scaled right-hand side
        b0, bs = C0[j].copy(), [v.copy() for v in CL[j].reshape(s.N, -1)]
        orc.solve_compressed(b0, bs, ref.leaves0, ref.Bts, ref.root0, s.n0, s.my0, s.mz0, s.myl, s.mzl, C0=s.C0, z_diag_reg=s.z_diag0)
        assert np.array_equal(np.concatenate(bs + [b0]), smc.scaled(ref, ref.X_ref0, j)), j
    # (six columns in the order of the bases, as the shared reference holds them: the LU solve of x* takes its right-hand sides as one block,
    # and the last bits of a blocked product may depend on the block's shape - not on a column's scale)
    assert [smc.base(j) for j in cols] == list(range(6)) * 2
    halves = [u.ArrowheadReference(s, C0[cols[h:h + 6]], CL[cols[h:h + 6]]) for h in (0, 6)]
    for h, direct in zip((0, 6), halves):
        assert direct.converged and direct.refinement_steps == ref.refinement_steps
        for i, j in enumerate(cols[h:h + 6]):
            assert np.array_equal(direct.X_ref0[i], smc.scaled(ref, ref.X_ref0, j)), j
            assert np.array_equal(direct.X_star[i], smc.scaled(ref, ref.X_star, j)), j
    # ... and so are the ratios: the direct reference on a solution, the shared one on the solution scaled back
    X = np.array([smc.scaled(ref, ref.X_ref0, j) for j in cols])
    X[:, ::7] *= 1.0 + 2.0 ** -40
    for h, direct in zip((0, 6), halves):
        want = direct.ratios(X[h:h + 6, nl:], X[h:h + 6, :nl])
        for i, j in enumerate(cols[h:h + 6]):
            got = smc.ratios(ref, X[h + i:h + i + 1, nl:], X[h + i:h + i + 1, :nl], first=j)
            assert all(got[name][0] == want[name][i] for name in want), (j, got, {k: v[i] for k, v in want.items()})
    zero = [i for i, j in enumerate(cols) if smc.base(j) == 5]
    assert zero and all(not X[i].any() for i in zero)
    # all columns of x_ref0 scaled are accepted at M = 1; a zero column that is not exactly zero is rejected
    X = np.array([smc.scaled(ref, ref.X_ref0, j) for j in range(40)])
    assert smc.accepts(ref, X[:, nl:], X[:, :nl], 1).all()
    X[5, 3] = 1e-300
    assert list(np.nonzero(~smc.accepts(ref, X[:, nl:], X[:, :nl], M_CAP))[0]) == [5]


def _mutants(case):
    return [m for m in u.SOLVE_COMPRESSED_MUTANTS if m != "z0_without_C0_x0" or case == "general_mz0"]


@pytest.mark.parametrize("case", CASES)
def test_the_predicate_rejects_the_mutants_on_a_scaled_column(case):
    ref = u.arrowhead_reference(case)
    nl = ref.n_leaves
    C0, CL = smc.columns(ref, NEIGHBOUR + 1)
    x0, xl = u.solve_compressed_fp64(ref.sys, ref.leaves0, ref.Bts, ref.root0, C0[J], CL[J])
    assert np.array_equal(np.concatenate([xl, x0]), smc.scaled(ref, ref.X_ref0, J))
    assert smc.accepts(ref, x0[None], xl[None], 1, first=J)[0]
    assert len(_mutants(case)) == (6 if case == "general_mz0" else 5)
    for mutant in _mutants(case):
        x0, xl = u.solve_compressed_fp64(ref.sys, ref.leaves0, ref.Bts, ref.root0, C0[J], CL[J], mutant)
        r = smc.ratios(ref, x0[None], xl[None], first=J)
        print(f"solve-multi-mutant case={case} {mutant} column={J}: " + " ".join(f"{name}={v[0]:.3g}" for name, v in r.items()))
        assert not smc.accepts(ref, x0[None], xl[None], M_CAP, first=J)[0], mutant
        # the same mutant of the base column, scaled: the same bits, so the proofs of the six base columns are the proofs of every column
        y0, yl = ref.mutant(smc.base(J), mutant)
        assert np.array_equal(x0, smc.scale(J) * y0) and np.array_equal(xl, smc.scale(J) * yl), mutant


@pytest.mark.parametrize("case", CASES)
def test_the_predicate_rejects_columns_that_got_mixed_up(case):
    ref = u.arrowhead_reference(case)
    nl = ref.n_leaves
    n = NEIGHBOUR + 3
    X = np.array([smc.scaled(ref, ref.X_ref0, j) for j in range(n)])
    assert smc.accepts(ref, X[:, nl:], X[:, :nl], 1).all()
    X[[J, NEIGHBOUR]] = X[[NEIGHBOUR, J]]
    ok = smc.accepts(ref, X[:, nl:], X[:, :nl], M_CAP)
    assert list(np.nonzero(~ok)[0]) == [J, NEIGHBOUR]
    # the column's leaf part with its neighbour's b0
    C0, CL = smc.columns(ref, n)
    x0, xl = u.solve_compressed_fp64(ref.sys, ref.leaves0, ref.Bts, ref.root0, C0[NEIGHBOUR], CL[J])
    assert not smc.accepts(ref, x0[None], xl[None], M_CAP, first=J)[0]
    # ... and the same base at another scale: column 30 is column 36 halved
    assert np.array_equal(2.0 * X[30], X[NEIGHBOUR]) and not smc.accepts(ref, X[30:31, nl:], X[30:31, :nl], M_CAP, first=J)[0]


# ---- the planner -------------------------------------------------------------------------------------------------------------------------
GIB2 = 2 << 30


def _plan(nrhs, from_=8, chunk_max=256, n_total=1000, budget=GIB2):
    return pa.capi.kkt_multi_plan_probe(nrhs, from_, chunk_max, n_total, budget)


@pytest.mark.parametrize("nrhs,want", [
    (0, []), (1, [(0, 1, 0)]), (7, [(q, 1, 0) for q in range(7)]), (8, [(0, 8, 1)]), (31, [(0, 31, 1)]), (32, [(0, 32, 1)]), (33, [(0, 33, 1)]),
    (256, [(0, 256, 1)]), (257, [(0, 256, 1), (256, 1, 1)]), (600, [(0, 256, 1), (256, 256, 1), (512, 88, 1)])])
def test_the_documented_chunks(nrhs, want):
    assert _plan(nrhs) == want


def test_the_chunks_respect_the_budget_and_never_go_below_a_panel():
    n_total = 2_000_000
    plan = _plan(600, n_total=n_total)
    assert plan == [(0, 128, 1), (128, 128, 1), (256, 128, 1), (384, 128, 1), (512, 88, 1)]
    assert all(c * n_total * 8 <= GIB2 for _, c, _ in plan) and (128 + 32) * n_total * 8 > GIB2
    for n_total in (1, 1000, 1 << 20, 2_000_000, 8_388_608, 8_388_609, 50_000_000, 1 << 40):
        for nrhs in (8, 100, 257, 600):
            plan = _plan(nrhs, n_total=n_total)
            assert [f for f, _, _ in plan] == list(np.cumsum([0] + [c for _, c, _ in plan[:-1]])) and sum(c for _, c, _ in plan) == nrhs
            assert all(p == 1 for _, _, p in plan) and all(c == plan[0][1] for _, c, _ in plan[:-1]) and plan[-1][1] <= plan[0][1]
            full = plan[0][1] if len(plan) > 1 else None
            if full is not None:
                assert full % 32 == 0 and 32 <= full <= 256
                assert full * n_total * 8 <= GIB2 or full == 32          # (one panel is the least, whatever it takes)
    assert _plan(100, n_total=8_388_608)[0] == (0, 32, 1) and _plan(100, n_total=8_388_609)[0] == (0, 32, 1) and _plan(100, n_total=4_194_304)[0] == (0, 64, 1)
    assert _plan(100, chunk_max=16) == [(0, 32, 1), (32, 32, 1), (64, 32, 1), (96, 4, 1)]
    assert _plan(100, chunk_max=64) == [(0, 64, 1), (64, 36, 1)]


def test_the_threshold():
    assert _plan(40, from_=0) == [(q, 1, 0) for q in range(40)]         # never panels
    assert _plan(2, from_=2) == [(0, 2, 1)] and _plan(1, from_=2) == [(0, 1, 0)]
    assert _plan(40, from_=41) == [(q, 1, 0) for q in range(40)] and _plan(41, from_=41) == [(0, 41, 1)]


def test_bad_arguments():
    for args in ((-1, 8, 256, 10, GIB2), (4, -1, 256, 10, GIB2), (4, 8, 0, 10, GIB2), (4, 8, 256, -1, GIB2), (4, 8, 256, 10, -1)):
        with pytest.raises(pa.capi.PipsHipError, match="pips_kkt_multi_plan_probe"):
            pa.capi.kkt_multi_plan_probe(*args)
