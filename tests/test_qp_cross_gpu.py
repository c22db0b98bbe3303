"""Convex QPs with cross Hessians between x0 and the blocks on the device harness (pips_ipm_create_qp_cross): the Hessian product
against the global scipy matrix, the solve against the numpy restatement of tests/qp_ref.py and the optimality conditions of the
original problem, long x0 rows, the sparse root, Schur mode 2, the scalers (Ruiz bit for bit against tests/qp_scaling_ref.ruiz on the
global Q, badly scaled twins), handles without R unchanged, deterministic mode."""
import numpy as np
import pytest
import scipy.sparse as sp

import pips_ipmpp_amd as pa
from tests import qp_cross_ref as qc
from tests import qp_scaling_ref as qs
from tests import scaling_ref as sr
from tests.qp_ref import kkt_check_qp

pytestmark = pytest.mark.gpu
INFO = ("applied", "row_ratio_before", "col_ratio_before", "row_ratio_after", "col_ratio_after", "geometric_passes", "geometric_kept", "host_waits")


def _check_product(ipm, Q, seed):
    x = np.random.default_rng(seed).standard_normal(Q.shape[0])
    got, want = ipm.hessian_mult(x), Q @ x
    err = np.abs(got - want).max()
    print(f"hessian_mult: max error {err:.3e}, bar {1e-13 * np.abs(want).max():.3e}")
    assert err <= 1e-13 * np.abs(want).max()


def _check_solve(ipm, d, Q, ref, trace=None):
    """tests/test_qp_gpu.py::_check_solve: the bars the LP test holds against HiGHS and the oracle, against the restatement"""
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    f = ref["objective"]
    print(f"status {res['status']}, iterations {res['iterations']} (restatement {ref['iterations']}), objective {res['objective']!r} "
          f"(restatement {f!r}), gap {abs(res['objective'] - res['dual_objective']):.3e}")
    assert ref["status"] == 0
    assert res["status"] == 0, res
    assert abs(res["objective"] - f) < 1e-6 * max(1.0, abs(f)), (res, f)
    assert abs(res["objective"] - res["dual_objective"]) < 1e-5 * max(1.0, abs(f))
    kkt_check_qp(d, Q, ipm.iterate(), 1e-5)
    T = ipm.trace()
    assert abs(res["iterations"] - ref["iterations"]) <= 1
    assert np.array_equal(T[:, 5], T[:, 6])   # one step length
    if trace is not None:
        assert abs(len(T) - len(trace)) <= 1
        early = min(len(T), len(trace)) - 4
        for k in range(max(early, 1)):
            want = np.array(trace[k][1:8] if len(trace[k]) == 8 else list(trace[k][1:5]) + [0, 0, 0])
            scale = np.maximum(np.abs(want), [1e-12, 1e-9 * ref["dnorm"], 1.0, 1.0, 1e-3, 1e-3, 1e-3])
            assert (np.abs(T[k] - want) / scale).max() < 1e-4, (k, T[k], want)
    return res


# ---- product ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,kind", [(0, "pd"), (1, "psd"), (4, "pd"), (7, "psd")])
def test_hessian_product_against_scipy(seed, kind):
    c = qc.case(seed, kind)
    ipm = pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], cross_hessians=c["rs"])
    _check_product(ipm, c["Q"], seed)
    ipm.close()
    # R alone: a QP handle
    ipm = pa.GeneralIpmSolver(c["blocks"], cross_hessians=c["rs"])
    _check_product(ipm, qc.global_hessian(None, c["rs"], c["blocks"]), seed)
    ipm.close()


def test_hessian_product_on_long_x0_rows():
    """541 entries in every x0 row: k_spmv_long_part / _finish carry the cross part"""
    c = qc.long_case()
    ipm = pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], cross_hessians=c["rs"])
    _check_product(ipm, c["Q"], 0)
    ipm.close()


# ---- solve -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("seed", range(8))
def test_qp_against_the_restatement_and_the_optimality_conditions(seed, kind):
    c = qc.case(seed, kind)
    ipm = pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], cross_hessians=c["rs"])
    _check_solve(ipm, c["d"], c["Q"], c["ref"], c["trace"])
    ipm.close()


def test_solve_with_long_x0_rows():
    c = qc.long_case()
    ipm = pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], cross_hessians=c["rs"])
    _check_solve(ipm, c["d"], c["Q"], c["ref"], c["trace"])
    ipm.close()


@pytest.mark.parametrize("seed", range(4))
def test_with_the_sparse_root(seed, monkeypatch):
    """the root inequality rows are kept as rows of the root system there, so the path differs: no trace comparison"""
    monkeypatch.setenv("PIPS_IPM_SPARSE_ROOT", "1")
    c = qc.case(seed, "pd")
    ipm = pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], cross_hessians=c["rs"])
    _check_solve(ipm, c["d"], c["Q"], c["ref"])
    ipm.close()


def test_with_blocked_schur_solves(monkeypatch):
    monkeypatch.setenv("PIPS_IPM_SCHUR_MODE", "2")
    c = qc.case(2, "pd")
    ipm = pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], cross_hessians=c["rs"])
    _check_solve(ipm, c["d"], c["Q"], c["ref"], c["trace"])
    ipm.close()


def test_outer_solve_runs_on_the_operator_with_the_cross_terms():
    from oracle import ipm_oracle as io
    c = qc.case(0, "pd")
    d, Q = c["d"], c["Q"]
    ipm = pa.GeneralIpmSolver(c["blocks"], dual_reg=3e-2, hessians=c["hs"], cross_hessians=c["rs"])
    ipm.set_option("REGULARIZATION", 0)
    rng = np.random.default_rng(5)
    mz, nx, my = ipm.nzr, ipm.nx, ipm.ny
    ncp = 2 * mz + 2 * nx
    G, L = 10 ** rng.uniform(-1, 1, ncp), 10 ** rng.uniform(-1, 1, ncp)
    rhs = rng.standard_normal(nx + my + mz)
    sol, info = ipm.outer_solve(G, L, rhs, tol=1e-10)
    M = np.concatenate([d["iclow"], d["icupp"], d["ixlow"], d["ixupp"]])
    ratio = np.where(M != 0, L / np.where(M != 0, G, 1.0), 0.0)
    dd = ratio[2 * mz:2 * mz + nx] + ratio[2 * mz + nx:]
    om = ratio[:mz] + ratio[mz:2 * mz]
    nom = np.where(om != 0, -1.0 / np.where(om != 0, om, 1.0), 0.0)
    J = sp.vstack([d["A"], d["C"]], format="csr")
    K = sp.bmat([[sp.diags(dd) + Q, J.T], [J, sp.diags(np.concatenate([np.zeros(my), nom]))]], format="csr")
    err = np.linalg.norm(K @ sol - rhs)
    print(f"outer solve: {info}, ||K sol - rhs|| = {err:.3e}, bar {1e-9 * np.linalg.norm(rhs):.3e}")
    assert io.BICG_STATUS[info["status"]] == "converged", info
    assert err <= 1e-9 * np.linalg.norm(rhs)
    ipm.close()


# ---- scaling ---------------------------------------------------------------------------------------------------------------------------
def _report(sc):
    return np.array([sc[k] for k in INFO], dtype=float)


def _check_factors(ipm, want, tag):
    col, re, ri, info = want
    got = ipm.scaling()
    assert np.array_equal(got["col"], col), tag
    assert np.array_equal(got["row_eq"], re) and np.array_equal(got["row_ineq"], ri), tag
    assert np.array_equal(_report(got), info), (tag, _report(got), info)


@pytest.mark.parametrize("seed,kind", [(0, "pd"), (1, "psd"), (4, "pd"), (7, "psd")])
def test_ruiz_factors_and_report_equal_the_restatement(seed, kind):
    """on the twin, whose cross entries span decades: Ruiz on [Q J^T; J 0] with the global arrow matrix, bit for bit"""
    t = qc.twin_case(seed, kind)
    ipm = pa.GeneralIpmSolver(t["tb"], hessians=t["th"], cross_hessians=t["tr"], scaler="ruiz")
    want = qs.ruiz(t["J"], t["Qt"], my=t["my"])
    _check_factors(ipm, want, (seed, kind))
    # the cross part moves the factors: without it Ruiz gives others
    assert not np.array_equal(want[0], qs.ruiz(t["J"], qs.global_hessian(t["th"], t["tb"]), my=t["my"])[0])
    # and the handle holds Q' = Cs Q Cs
    v = np.random.default_rng(seed).standard_normal(ipm.nx)
    got, wantp = ipm.hessian_mult(v), want[0] * (t["Qt"] @ (want[0] * v))
    assert np.abs(got - wantp).max() <= 1e-13 * np.abs(wantp).max()
    ipm.close()


def test_ruiz_factors_on_long_x0_rows():
    """the Q sweep of the x0 rows runs through k_scale_sweep_long"""
    c = qc.long_case()
    J, my, _ = qs.J_of(c["blocks"])
    ipm = pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], cross_hessians=c["rs"], scaler="ruiz")
    _check_factors(ipm, qs.ruiz(J, c["Q"], my=my), "long rows")
    ipm.close()


def test_j_only_scalers_take_their_factors_from_j():
    t = qc.twin_case(0, "pd")
    for name, kind in (("equilibrium", sr.EQUILIBRIUM), ("geometric_equilibrium", sr.GEOMETRIC_EQUILIBRIUM)):
        ipm = pa.GeneralIpmSolver(t["tb"], hessians=t["th"], cross_hessians=t["tr"], scaler=name)
        _check_factors(ipm, sr.scale(t["J"], t["my"], kind), name)
        sc = ipm.scaling()
        v = np.random.default_rng(3).standard_normal(ipm.nx)
        got, want = ipm.hessian_mult(v), sc["col"] * (t["Qt"] @ (sc["col"] * v))
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), name
        ipm.close()


@pytest.mark.parametrize("seed,kind", qc.TWINS)
def test_ruiz_solves_the_badly_scaled_twin(seed, kind):
    """Status 0, the objective of the restatement on the unscaled original, one step length, and the iterate mapped back to the problem
    before the twin transformation satisfies its optimality conditions (the bars of tests/test_qp_scaling_gpu.py).  The twins are
    those on which the restatement completes after Ruiz scaling (qc.TWINS)."""
    c, t = qc.case(seed, kind), qc.twin_case(seed, kind)
    assert qc.scaled_twin_ref(seed, kind)["status"] == 0
    cs, rq, rn = t["fac"]
    f = c["ref"]["objective"]
    ipm = pa.GeneralIpmSolver(t["tb"], hessians=t["th"], cross_hessians=t["tr"], scaler="ruiz")
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    print(f"status {res['status']}, iterations {res['iterations']} (restatement on the original {c['ref']['iterations']}), "
          f"objective error {abs(res['objective'] - f):.3e}, gap {abs(res['objective'] - res['dual_objective']):.3e}, bar unit {max(1.0, abs(f)):.3e}")
    assert res["status"] == 0, res
    assert abs(res["objective"] - f) < 1e-6 * max(1.0, abs(f)), (res, f)
    assert abs(res["objective"] - res["dual_objective"]) < 1e-5 * max(1.0, abs(f))
    T = ipm.trace()
    assert np.array_equal(T[:, 5], T[:, 6])
    it = ipm.iterate()
    orig_it = dict(x=it["x"] * cs, y=it["y"] * rq, z=it["z"] * rn, lam=it["lam"] * rn, pi=it["pi"] * rn, gamma=it["gamma"] / cs, phi=it["phi"] / cs)
    d = c["d"]
    mult = max(np.abs(orig_it[k]).max(initial=0.0) for k in ("lam", "pi", "gamma", "phi", "y", "z"))
    scale = max(1.0, np.abs(d["b"]).max(initial=0.0), np.abs(d["c"]).max(initial=0.0))
    kkt_check_qp(d, c["Q"], orig_it, 1e-5 * max(1.0, mult / scale))
    ipm.close()


# ---- unchanged paths, deterministic mode -----------------------------------------------------------------------------------------------
def _run(ipm):
    sc = ipm.scaling()
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    out = (res, ipm.trace(), ipm.iterate(), sc, ipm.stats2()["host_syncs"])
    ipm.close()
    return out


def _same(a, b):
    (ra, ta, ia, sa, wa), (rb, tb, ib, sb, wb) = a, b
    assert all(np.array_equal(ra[k], rb[k]) for k in ra), (ra, rb)
    assert np.array_equal(ta, tb)
    assert all(np.array_equal(ia[k], ib[k]) for k in ia)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert wa == wb


@pytest.mark.parametrize("scaler", [None, "ruiz"])
def test_a_handle_without_r_is_the_block_diagonal_one(scaler, monkeypatch):
    """through the new entry with no R, and with R_i that hold no entry: result, trace, solution, factors and host waits, to the bit"""
    from tests.qp_ref import block_hessians
    monkeypatch.setenv("PIPS_HIP_DETERMINISTIC", "1")
    blocks = qc.random_lp(1)
    hs, _ = block_hessians(1, blocks, "pd")
    n = qc.sizes(blocks)
    base = _run(pa.GeneralIpmSolver(blocks, hessians=hs, scaler=scaler))
    assert base[0]["status"] == 0
    _same(base, _run(pa.GeneralIpmSolver(blocks, hessians=hs, scaler=scaler, cross_hessians=[None] * len(blocks))))
    empty = [None] + [dict(rows=m, cols=n[0], rowptr=[0] * (m + 1), colidx=[], val=[]) for m in n[1:]]
    _same(base, _run(pa.GeneralIpmSolver(blocks, hessians=hs, scaler=scaler, cross_hessians=empty)))
    # an LP through it stays the LP handle
    lp = _run(pa.GeneralIpmSolver(blocks, scaler=scaler))
    _same(lp, _run(pa.GeneralIpmSolver(blocks, scaler=scaler, cross_hessians=[None] * len(blocks))))


@pytest.mark.parametrize("scaler", [None, "ruiz"])
def test_deterministic_cross_qp_repeats_to_the_bit(scaler, monkeypatch):
    monkeypatch.setenv("PIPS_HIP_DETERMINISTIC", "1")
    c = qc.case(1, "pd")
    a = _run(pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], cross_hessians=c["rs"], scaler=scaler))
    b = _run(pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], cross_hessians=c["rs"], scaler=scaler))
    assert a[0]["status"] == 0
    _same(a, b)


def test_stored_zero_cross_entries_do_not_move_the_objective():
    """R_i of stored zeros: a cross handle (border rows under x0, long way round) on the block-diagonal problem"""
    from tests.qp_ref import block_hessians
    blocks = qc.random_lp(1)
    hs, _ = block_hessians(1, blocks, "pd")
    n = qc.sizes(blocks)
    zeros = [None] + [dict(rows=m, cols=n[0], rowptr=list(range(m + 1)), colidx=[k % n[0] for k in range(m)], val=[0.0] * m) for m in n[1:]]
    a = pa.GeneralIpmSolver(blocks, hessians=hs)
    ra = a.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    a.close()
    b = pa.GeneralIpmSolver(blocks, hessians=hs, cross_hessians=zeros)
    rb = b.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    b.close()
    assert ra["status"] == 0 and rb["status"] == 0
    assert abs(ra["objective"] - rb["objective"]) <= 1e-8 * max(1.0, abs(ra["objective"]))
