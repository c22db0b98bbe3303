"""Scaling of convex QPs on the device harness (pips_ipm_create_qp_scaled): the Ruiz factors against the numpy restatement of
tests/qp_scaling_ref.py bit for bit, the J-only scalers with Hessians, the products of the scaled handle, the solve of badly scaled
twins against the restatement of tests/qp_ref.py and the optimality conditions of the problem before the twin transformation,
unscaled handles unchanged, deterministic mode, refusals, two ranks and device memory."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pips_ipmpp_amd as pa
from tests import qp_scaling_ref as qs
from tests import scaling_ref as sr
from tests.general_lp_gen import random_block_lp
from tests.qp_ref import block_hessians, kkt_check_qp, long_row_case, solve_qp
from tests.test_qp_ref_cpu import _random_lp

pytestmark = pytest.mark.gpu
KINDS = ["pd", "psd"]
J_ONLY = {"equilibrium": sr.EQUILIBRIUM, "geometric": sr.GEOMETRIC, "geometric_equilibrium": sr.GEOMETRIC_EQUILIBRIUM}
INFO = ("applied", "row_ratio_before", "col_ratio_before", "row_ratio_after", "col_ratio_after", "geometric_passes", "geometric_kept", "host_waits")


@functools.lru_cache(maxsize=None)
def _case(seed, kind):
    """the original QP with its assembled data and the restatement's result, its badly scaled twin with J, my, the global Q and the twin
    factors - computed once, shared, left unchanged"""
    from oracle import ipm_oracle as io
    blocks = _random_lp(seed, 0.0)
    hs, _ = block_hessians(seed, blocks, kind)
    Q = qs.global_hessian(hs, blocks)
    d = io.assemble(blocks)
    ref = solve_qp(d, Q, max_iter=100, mutol=1e-9, artol=1e-8)
    tb, th, fac = qs.twin(blocks, hs, seed)
    J, my, _ = qs.J_of(tb)
    return dict(blocks=blocks, hs=hs, Q=Q, d=d, ref=ref, tb=tb, th=th, fac=fac, J=J, my=my, Qt=qs.global_hessian(th, tb))


def _report(sc):
    return np.array([sc[k] for k in INFO], dtype=float)


def _check_factors(ipm, want, tag):
    col, re, ri, info = want
    got = ipm.scaling()
    assert np.array_equal(got["col"], col), tag
    assert np.array_equal(got["row_eq"], re) and np.array_equal(got["row_ineq"], ri), tag
    assert np.array_equal(_report(got), info), (tag, _report(got), info)


# ---- factors, bitwise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", range(8))
def test_ruiz_factors_and_report_equal_the_restatement(seed, kind):
    """Exact agreement: maxima do not depend on the order, sqrt and the division are correctly rounded on both sides, and the products
    are formed in the same order."""
    c = _case(seed, kind)
    ipm = pa.GeneralIpmSolver(c["tb"], hessians=c["th"], scaler="ruiz")
    _check_factors(ipm, qs.ruiz(c["J"], c["Qt"], my=c["my"]), (seed, kind))
    ipm.close()


@pytest.mark.parametrize("seed", range(4))
def test_ruiz_factors_without_a_hessian(seed):
    """Ruiz on [0 J^T; J 0]: an LP twin, created by pips_ipm_create_general_scaled, and the same through the QP entry with no Hessian
    present"""
    c = _case(seed, "pd")
    want = qs.ruiz(c["J"], None, my=c["my"])
    for kw in (dict(), dict(hessians=[None] * len(c["tb"]))):
        ipm = pa.GeneralIpmSolver(c["tb"], scaler="ruiz", **kw)
        _check_factors(ipm, want, (seed, kw))
        assert np.array_equal(ipm.hessian_mult(np.ones(ipm.nx)), np.zeros(ipm.nx))
        ipm.close()


def test_ruiz_factors_on_long_rows():
    """n0 = 520: every row of Q0 in full storage is longer than the long-row threshold (512), so the Q sweep runs through
    k_scale_sweep_long (J and J^T of this shape have short rows only: at most 11 and 5 entries)"""
    blocks, hs, _ = long_row_case()
    Q = qs.global_hessian(hs, blocks)
    assert np.diff(Q.indptr)[:520].min() == 520
    J, my, _ = qs.J_of(blocks)
    ipm = pa.GeneralIpmSolver(blocks, hessians=hs, scaler="ruiz")
    _check_factors(ipm, qs.ruiz(J, Q, my=my), "long rows")
    ipm.close()


@pytest.mark.parametrize("seed", range(4))
def test_j_only_scalers_with_hessians_take_their_factors_from_j(seed):
    c = _case(seed, KINDS[seed % 2])
    for name, kind in J_ONLY.items():
        ipm = pa.GeneralIpmSolver(c["tb"], hessians=c["th"], scaler=name)
        _check_factors(ipm, sr.scale(c["J"], c["my"], kind), (seed, name))
        ipm.close()


# ---- products on the scaled handle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_products_of_the_scaled_handle(seed):
    """hessian_mult is Q' v = Cs Q Cs v and mult the scaled operator R J Cs, with the factors the handle reports"""
    c = _case(seed, KINDS[seed % 2])
    J, Qt = c["J"], c["Qt"]
    rng = np.random.default_rng(seed)
    v, w = rng.standard_normal(J.shape[1]), rng.standard_normal(J.shape[0])
    for name in list(J_ONLY) + ["ruiz"]:
        ipm = pa.GeneralIpmSolver(c["tb"], hessians=c["th"], scaler=name)
        sc = ipm.scaling()
        if not sc["applied"]:   # (the geometric scaler may decline)
            assert name == "geometric"
            ipm.close()
            continue
        got, want = ipm.hessian_mult(v), sc["col"] * (Qt @ (sc["col"] * v))
        err = np.abs(got - want).max()
        print(f"{name}: hessian_mult max error {err:.3e}, bar {1e-13 * np.abs(want).max():.3e}")
        assert err <= 1e-13 * np.abs(want).max(), name
        S = sp.diags(np.concatenate([sc["row_eq"], sc["row_ineq"]])) @ J @ sp.diags(sc["col"])
        for g, wt in ((ipm.mult(v), S @ v), (ipm.mult(w, transposed=True), S.T @ w)):
            assert np.abs(g - wt).max() <= 1e-14 * max(1.0, np.abs(wt).max()) * 10, name
        ipm.close()


# ---- the solve ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", range(8))
def test_ruiz_solves_the_badly_scaled_twin(seed, kind):
    """Status 0, the objective of the restatement on the unscaled original, one step length, the iterate mapped back to the problem
    before the twin transformation satisfies its optimality conditions, and the early path is the restatement's on the
    restatement-scaled twin."""
    from oracle import ipm_oracle as io
    c = _case(seed, kind)
    cs, rq, rn = c["fac"]
    ref, f = c["ref"], c["ref"]["objective"]
    assert ref["status"] == 0
    col, re, ri, _ = qs.ruiz(c["J"], c["Qt"], my=c["my"])
    sb, sh = sr.transform_blocks(c["tb"], col, re, ri), qs.scale_hessians(c["th"], c["tb"], col)
    trace = []
    o = solve_qp(io.assemble(sb), qs.global_hessian(sh, sb), max_iter=100, mutol=1e-9, artol=1e-8, trace=trace)
    ipm = pa.GeneralIpmSolver(c["tb"], hessians=c["th"], scaler="ruiz")
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    print(f"status {res['status']}, iterations {res['iterations']} (restatement on the scaled twin {o['iterations']}, on the original {ref['iterations']}), "
          f"objective error {abs(res['objective'] - f):.3e}, gap {abs(res['objective'] - res['dual_objective']):.3e}, bar unit {max(1.0, abs(f)):.3e}")
    assert res["status"] == 0, res
    assert abs(res["objective"] - f) < 1e-6 * max(1.0, abs(f)), (res, f)
    assert abs(res["objective"] - res["dual_objective"]) < 1e-5 * max(1.0, abs(f))
    T = ipm.trace()
    assert np.array_equal(T[:, 5], T[:, 6])   # one step length
    it = ipm.iterate()   # of the twin; back to the problem before the twin transformation (the map of unscale_variables)
    orig_it = dict(x=it["x"] * cs, y=it["y"] * rq, z=it["z"] * rn, lam=it["lam"] * rn, pi=it["pi"] * rn, gamma=it["gamma"] / cs, phi=it["phi"] / cs)
    d = c["d"]
    mult = max(np.abs(orig_it[k]).max(initial=0.0) for k in ("lam", "pi", "gamma", "phi", "y", "z"))
    scale = max(1.0, np.abs(d["b"]).max(initial=0.0), np.abs(d["c"]).max(initial=0.0))
    kkt_check_qp(d, c["Q"], orig_it, 1e-5 * max(1.0, mult / scale))
    # The early path.  The number of iterations is not compared: the device stops on the unscaled residual against the twin's data
    # norm, the restatement on the scaled one against the scaled norm, and a step of length ~1 leaves mu ~ (1 - alpha) mu, which
    # moves with the last digits of alpha (`pd` 5: mu 0.32 -> 5.7e-8 in one step of the restatement, which ends after 10 iterations, the
    # device after 8; the other 15 twins end within one iteration of it)
    assert o["status"] == 0
    early = min(len(T), len(trace)) - 4
    for k in range(max(early, 1)):
        want = np.array(trace[k][1:8] if len(trace[k]) == 8 else list(trace[k][1:5]) + [0, 0, 0])
        cols = [0, 2, 3, 4, 5, 6]   # mu, pobj, dobj, sigma, alpha_p, alpha_d: the residual norm differs (the device reports the unscaled one)
        sc = np.maximum(np.abs(want), [1e-12, 1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3])
        assert (np.abs(T[k] - want) / sc)[cols].max() < 1e-4, (k, T[k], want)
    ipm.close()


# ---- unscaled handles unchanged, deterministic mode ---------------------------------------------------------------------------------------
class _Direct(pa.GeneralIpmSolver):
    """a handle from a direct call of pips_ipm_create_qp_scaled with the scaler given as a number"""

    def __init__(self, blocks, hessians, scaler):
        capi = pa.capi
        keep, cb, cq, tail = capi._ipm_input(blocks, hessians)
        self.n_blocks, self._keep, self._comm, self._h = len(blocks), (keep, cb, cq), None, C.c_void_p()
        capi._check(capi.lib.pips_ipm_create_qp_scaled(C.byref(self._h), C.c_int(len(blocks)), cb, cq, *tail, C.c_double(0.0), C.c_int(-1), None,
                                                       C.c_int(0), C.c_int(1), C.c_int(scaler)), "pips_ipm_create_qp_scaled")
        d = (C.c_longlong * 4)()
        capi._check(capi.lib.pips_ipm_get_dims(self._h, d), "pips_ipm_get_dims")
        self.nx, self.ny, self.nzr, self.n_pairs = int(d[0]), int(d[1]), int(d[2]), int(d[3])


def _run(ipm):
    sc = ipm.scaling()
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    out = (res, ipm.trace(), ipm.iterate(), sc)
    ipm.close()
    return out


def _same(a, b):
    (ra, ta, ia, sa), (rb, tb, ib, sb) = a, b
    assert all(np.array_equal(ra[k], rb[k]) for k in ra), (ra, rb)
    assert np.array_equal(ta, tb)
    assert all(np.array_equal(ia[k], ib[k]) for k in ia)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)


def test_unscaled_qp_handles_are_unchanged(monkeypatch):
    monkeypatch.setenv("PIPS_HIP_DETERMINISTIC", "1")
    c = _case(1, "pd")
    base = _run(pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"]))
    assert base[0]["status"] == 0 and not base[3]["applied"] and base[3]["host_waits"] == 0
    _same(base, _run(pa.GeneralIpmSolver(c["blocks"], hessians=c["hs"], scaler=None)))
    _same(base, _run(_Direct(c["blocks"], c["hs"], pa.capi.PIPS_SCALER_NONE)))


def test_deterministic_ruiz_scaled_qp_repeats_to_the_bit(monkeypatch):
    monkeypatch.setenv("PIPS_HIP_DETERMINISTIC", "1")
    c = _case(1, "pd")
    a = _run(pa.GeneralIpmSolver(c["tb"], hessians=c["th"], scaler="ruiz"))
    b = _run(pa.GeneralIpmSolver(c["tb"], hessians=c["th"], scaler="ruiz"))
    assert a[0]["status"] == 0 and a[3]["applied"]
    _same(a, b)
    _same(a, _run(_Direct(c["tb"], c["th"], pa.capi.PIPS_SCALER_RUIZ)))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refused_scalers_and_bad_hessians():
    c = _case(0, "pd")
    for bad in (4, 6, -1):
        with pytest.raises(pa.capi.PipsHipError, match="not supported"):
            _Direct(c["tb"], c["th"], bad)
        with pytest.raises(pa.capi.PipsHipError, match="not supported"):
            _Direct(c["tb"], None, bad)
    with pytest.raises(pa.capi.PipsHipError):
        pa.GeneralIpmSolver(c["tb"], hessians=c["th"], scaler="curtis_reid")
    n0 = int(c["tb"][0]["n0"])
    upper = dict(rows=n0, cols=n0, rowptr=[0, 2] + list(range(3, n0 + 2)), colidx=[0, 1] + list(range(1, n0)), val=[1.0] * (n0 + 1))
    for name in ("ruiz", "equilibrium"):
        with pytest.raises(pa.capi.PipsHipError, match="above the diagonal"):
            pa.GeneralIpmSolver(c["tb"], hessians=[upper] + [None] * (len(c["tb"]) - 1), scaler=name)


# ---- two ranks -------------------------------------------------------------------------------------------------------------------------
def _two_rank_problem():
    """"psd": the blocks with an odd index carry no Hessian"""
    b = random_block_lp(705, 5, 6, 14, 4, 3, 2, 2)
    hs, _ = block_hessians(5, b, "psd")
    tb, th, _ = qs.twin(b, hs, 31)
    return tb, th


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    blocks, hs = _two_rank_problem()
    mine = np.nonzero(pa.map_children_to_ranks(len(blocks) - 1, world) == rank)[0]

    def allreduce(ptr, n):
        t = torch.as_tensor(pa.capi._DeviceDoubles(ptr, n), device="cuda")
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)
        torch.cuda.synchronize()

    comm = pa.ExternalComm(allreduce)
    ipm = pa.GeneralIpmSolver([blocks[0]] + [blocks[1 + k] for k in mine], hessians=[hs[0]] + [hs[1 + k] for k in mine], comm=comm, rank=rank,
                              n_ranks=world, scaler="ruiz")
    sc = ipm.scaling()
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    np.savez(os.path.join(out, f"rank{rank}.npz"), res=np.array([res[k] for k in ("status", "iterations", "objective")]), col=sc["col"],
             re=sc["row_eq"], ri=sc["row_ineq"], info=_report(sc), mine=mine)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_scale_and_solve_like_one(tmp_path):
    world = 2
    port = 29500 + (os.getpid() % 2000) + 37
    mp.start_processes(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    blocks, hs = _two_rank_problem()
    one = pa.GeneralIpmSolver(blocks, hessians=hs, scaler="ruiz")
    sc = one.scaling()
    r1 = one.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    root = blocks[0]
    n0, my0, mz0, myl, mzl = root["n0"], root["mA"], root["mC"], root["mBL"], root["mDL"]
    xo, yo, zo = [n0], [my0 + myl], [mz0 + mzl]
    for b in blocks[1:]:
        xo.append(xo[-1] + b["ni"]); yo.append(yo[-1] + b["mA"]); zo.append(zo[-1] + b["mC"])
    for rank in range(world):
        z = np.load(os.path.join(tmp_path, f"rank{rank}.npz"))
        mine = z["mine"]
        col = np.concatenate([sc["col"][:n0]] + [sc["col"][xo[k]:xo[k + 1]] for k in mine])
        re = np.concatenate([sc["row_eq"][:my0 + myl]] + [sc["row_eq"][yo[k]:yo[k + 1]] for k in mine])
        ri = np.concatenate([sc["row_ineq"][:mz0 + mzl]] + [sc["row_ineq"][zo[k]:zo[k + 1]] for k in mine])
        assert np.array_equal(z["col"], col) and np.array_equal(z["re"], re) and np.array_equal(z["ri"], ri), rank
        assert np.array_equal(z["info"], _report(sc)), rank
        assert int(z["res"][0]) == r1["status"] and int(z["res"][1]) == r1["iterations"], (z["res"], r1)
        assert abs(z["res"][2] - r1["objective"]) <= 1e-9 * abs(r1["objective"])
    one.close()


# ---- memory ----------------------------------------------------------------------------------------------------------------------------
def test_a_ruiz_scaled_qp_handle_gives_back_what_it_took():
    c = _case(2, "pd")

    def cycle():
        ipm = pa.GeneralIpmSolver(c["tb"], hessians=c["th"], scaler="ruiz")
        assert ipm.scaling()["applied"]
        ipm.solve(max_iter=5)
        ipm.close()
        torch.cuda.synchronize()

    cycle()   # warm-up: what is allocated on first use and meant to stay
    want = (pa.device_allocs_live(), pa.device_bytes_live())
    cycle()
    assert (pa.device_allocs_live(), pa.device_bytes_live()) == want
