"""Problem scaling on the device (pips_ipm_create_general_scaled): the factors against the numpy restatement of the reference's
scalers (tests/scaling_ref.py), the scaled operator, the reference's known-answer LPs with the geometric-mean scaler
(t_pips.cpp:122-129 TestGamssmallPrimalDualStepScaleGeo), badly scaled LPs, the path against the CPU restatement on the scaled
data, a declining scaler that changes nothing, and two ranks."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pips_ipmpp_amd as pa
from tests import scaling_ref as sr
from tests.general_lp_gen import random_block_lp
from tests.test_native_general_gpu import _highs, _kkt_check, _random_lp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GAMSSMALL = json.load(open(os.path.join(HERE, "golden", "gamssmall.json")))["instances"]
KINDS = {"equilibrium": sr.EQUILIBRIUM, "geometric": sr.GEOMETRIC, "geometric_equilibrium": sr.GEOMETRIC_EQUILIBRIUM}
BAD_GAMS = [0, 7, 13, 20]   # GAMSsmall instances that get a badly scaled twin


def _bad(blocks, seed):
    col, re, ri = sr.random_factors(blocks, 9000 + seed)
    return sr.transform_blocks(blocks, col, re, ri), (col, re, ri)


def _cases():
    out = [(f"gams_{d['name']}", lambda d=d: d["blocks"]) for d in GAMSSMALL]
    out += [(f"random_{s}", lambda s=s: _random_lp(s, 0.0)) for s in range(8)]
    out += [(f"bad_random_{s}", lambda s=s: _bad(_random_lp(s, 0.0), s)[0]) for s in range(8)]
    out += [(f"bad_gams_{GAMSSMALL[k]['name']}", lambda k=k: _bad(GAMSSMALL[k]["blocks"], 100 + k)[0]) for k in BAD_GAMS]
    return out


CASES = _cases()


def _J(blocks):
    from oracle import ipm_oracle as io
    d = io.assemble(blocks)
    return sp.csr_matrix(sp.vstack([d["A"], d["C"]])), d["A"].shape[0], d


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_factors_and_report_equal_the_restatement(case):
    """Exact agreement: min / max do not depend on the order, sqrt and the division are correctly rounded on both sides, and the
    products |a s| are formed the same way."""
    blocks = case[1]()
    J, my, _ = _J(blocks)
    for name, kind in KINDS.items():
        col, re, ri, info = sr.scale(J, my, kind)
        ipm = pa.GeneralIpmSolver(blocks, dual_reg=1e-9, scaler=name)
        got = ipm.scaling()
        assert np.array_equal(got["col"], col), name
        assert np.array_equal(got["row_eq"], re) and np.array_equal(got["row_ineq"], ri), name
        g = [got["applied"], got["row_ratio_before"], got["col_ratio_before"], got["row_ratio_after"], got["col_ratio_after"],
             got["geometric_passes"], got["geometric_kept"], got["host_waits"]]
        assert np.array_equal(np.array(g, dtype=float), info), (name, g, info)
        ipm.close()


@pytest.mark.parametrize("seed", range(3))
def test_mult_is_the_scaled_operator(seed):
    blocks = _bad(_random_lp(seed, 0.0), seed)[0]
    J, my, _ = _J(blocks)
    ipm = pa.GeneralIpmSolver(blocks, scaler="geometric_equilibrium")
    sc = ipm.scaling()
    assert sc["applied"]
    S = sp.diags(np.concatenate([sc["row_eq"], sc["row_ineq"]])) @ J @ sp.diags(sc["col"])
    rng = np.random.default_rng(seed)
    v, w = rng.standard_normal(J.shape[1]), rng.standard_normal(J.shape[0])
    for got, want in ((ipm.mult(v), S @ v), (ipm.mult(w, transposed=True), S.T @ w)):
        assert np.abs(got - want).max() <= 1e-14 * max(1.0, np.abs(want).max()) * 10
    ipm.close()


# instances that miss only the iteration bound with the scaler: (name, scaler) -> measured iterations, reason
ITER_EXCEPTIONS = {}


@pytest.mark.parametrize("inst", GAMSSMALL, ids=[d["name"] for d in GAMSSMALL])
def test_gamssmall_scaled(inst):
    """TestGamssmallPrimalDualStepScaleGeo: all 26 with the geometric-mean scaler, every third one with the other two"""
    from oracle import ipm_oracle as io
    k = GAMSSMALL.index(inst)
    d = io.assemble(inst["blocks"])
    for name in (["geometric"] + (["equilibrium", "geometric_equilibrium"] if k % 3 == 0 else [])):
        ipm = pa.GeneralIpmSolver(inst["blocks"], dual_reg=1e-9, scaler=name)
        res = ipm.solve(max_iter=200, mutol=1e-8, artol=1e-8)
        assert res["status"] == 0, (name, res)
        assert abs(res["objective"] - inst["expected_objective"]) < 1e-4, (name, res)
        if (inst["name"], name) not in ITER_EXCEPTIONS:
            assert res["iterations"] <= 1.1 * inst["expected_iterations"] + 1, (name, res)
        _kkt_check(d, ipm.iterate(), 1e-5)
        ipm.close()


BAD = [(f"random_{s}", s, None) for s in range(8)] + [(f"gams_{GAMSSMALL[k]['name']}", 100 + k, k) for k in BAD_GAMS]


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_badly_scaled_lp(case):
    """A' = R A Cs with R, Cs from 10^U(-4, 4): geometric + equilibrium scaling solves it; x = Cs x' and the mapped multipliers
    satisfy the optimality conditions of the original problem"""
    from oracle import ipm_oracle as io
    _, seed, k = case
    orig = _random_lp(seed, 0.0) if k is None else GAMSSMALL[k]["blocks"]
    blocks, (cs, rq, rn) = _bad(orig, seed)
    d = io.assemble(orig)
    ref = _highs(d)
    assert ref.status == 0
    ipm = pa.GeneralIpmSolver(blocks, dual_reg=1e-9, scaler="geometric_equilibrium")
    res = ipm.solve(max_iter=200, mutol=1e-9, artol=1e-8)
    assert res["status"] == 0, res
    assert abs(res["objective"] - ref.fun) < 1e-6 * max(1.0, abs(ref.fun)), (res, ref.fun)
    it = ipm.iterate()   # of the badly scaled problem; back to the original one (the same map as unscale_variables)
    orig_it = dict(x=it["x"] * cs, y=it["y"] * rq, z=it["z"] * rn, lam=it["lam"] * rn, pi=it["pi"] * rn, gamma=it["gamma"] / cs, phi=it["phi"] / cs)
    # the stopping test is relative to the transformed problem: its multipliers map back with 1 / cs (up to 1e4), so the
    # stationarity and complementarity terms of the original carry that magnitude - the tolerance is relative to it
    mult = max(np.abs(orig_it[k]).max(initial=0.0) for k in ("lam", "pi", "gamma", "phi", "y", "z"))
    scale = max(1.0, np.abs(d["b"]).max(initial=0.0), np.abs(d["c"]).max(initial=0.0))
    _kkt_check(d, orig_it, 1e-5 * max(1.0, mult / scale))
    ipm.close()


@pytest.mark.parametrize("seed", range(4))
def test_path_matches_the_cpu_restatement_on_the_scaled_data(seed):
    from oracle import ipm_oracle as io
    blocks = _bad(_random_lp(seed, 0.0), seed)[0]
    J, my, _ = _J(blocks)
    col, re, ri, info = sr.scale(J, my, sr.GEOMETRIC)
    assert info[0] == 1.0
    ipm = pa.GeneralIpmSolver(blocks, scaler="geometric")
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    assert res["status"] == 0, res
    trace = []
    o = io.solve_blocks(sr.transform_blocks(blocks, col, re, ri), max_iter=100, mutol=1e-9, artol=1e-8, trace=trace)
    T = ipm.trace()
    assert abs(len(T) - len(trace)) <= 1
    early = min(len(T), len(trace)) - 4
    for k in range(max(early, 1)):
        want = np.array(trace[k][1:8] if len(trace[k]) == 8 else list(trace[k][1:5]) + [0, 0, 0])
        # mu, pobj, dobj, sigma, alpha_p, alpha_d: the residual norm differs (the device reports the unscaled one)
        cols = [0, 2, 3, 4, 5, 6]
        scale = np.maximum(np.abs(want), [1e-12, 1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3])
        assert (np.abs(T[k] - want) / scale)[cols].max() < 1e-4, (k, T[k], want)


def test_declining_scaler_changes_nothing(monkeypatch):
    """geometric on ratios <= 500: factors of exactly 1, applied 0, and the run is the unscaled one to the bit"""
    monkeypatch.setenv("PIPS_HIP_DETERMINISTIC", "1")
    blocks = next(d["blocks"] for d in GAMSSMALL if sr.scale(*_J(d["blocks"])[:2], sr.GEOMETRIC)[3][0] == 0.0 and d["blocks"][0]["mBL"] > 0)
    runs = []
    for scaler in (None, "geometric"):
        ipm = pa.GeneralIpmSolver(blocks, dual_reg=1e-9, scaler=scaler)
        sc = ipm.scaling()
        assert not sc["applied"] and (sc["col"] == 1).all() and (sc["row_eq"] == 1).all() and (sc["row_ineq"] == 1).all()
        res = ipm.solve(max_iter=200, mutol=1e-8, artol=1e-8)
        runs.append((res, ipm.trace(), ipm.solution(), ipm.stats2()["host_syncs"]))
        ipm.close()
    (r0, t0, s0, h0), (r1, t1, s1, h1) = runs
    assert r0 == r1 and np.array_equal(t0, t1) and h0 == h1
    assert all(np.array_equal(a, b) for a, b in zip(s0, s1))


def test_curtis_reid_and_unknown_names_raise_and_unscaled_handles_report_ones():
    blocks = _random_lp(0, 0.0)
    for bad in ("curtis_reid", "geo"):
        with pytest.raises(pa.capi.PipsHipError):
            pa.GeneralIpmSolver(blocks, scaler=bad)
    ipm = pa.GeneralIpmSolver(blocks)
    sc = ipm.scaling()
    assert not sc["applied"] and sc["host_waits"] == 0
    assert (sc["col"] == 1).all() and (sc["row_eq"] == 1).all() and (sc["row_ineq"] == 1).all()
    ipm.close()


# ---- two ranks --------------------------------------------------------------------------------------------------------------
TWO = dict(seed=5, nb=5, n0=6, ni=14, mA=4, mC=3, mBL=2, mDL=2)


def _two_rank_blocks():
    b = random_block_lp(700 + TWO["seed"], TWO["nb"], TWO["n0"], TWO["ni"], TWO["mA"], TWO["mC"], TWO["mBL"], TWO["mDL"], free_fraction=0.0)
    return _bad(b, 31)[0]


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    blocks = _two_rank_blocks()
    N = len(blocks) - 1
    mine = np.nonzero(pa.map_children_to_ranks(N, world) == rank)[0]

    def allreduce(ptr, n):
        t = torch.as_tensor(pa.capi._DeviceDoubles(ptr, n), device="cuda")
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)
        torch.cuda.synchronize()

    comm = pa.ExternalComm(allreduce)
    ipm = pa.GeneralIpmSolver([blocks[0]] + [blocks[1 + k] for k in mine], dual_reg=1e-9, comm=comm, rank=rank, n_ranks=world,
                              scaler="geometric_equilibrium")
    sc = ipm.scaling()
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    np.savez(os.path.join(out, f"rank{rank}.npz"), res=np.array([res[k] for k in ("status", "iterations", "objective")]), trace=ipm.trace(),
             col=sc["col"], re=sc["row_eq"], ri=sc["row_ineq"], mine=mine)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_scale_and_solve_like_one(tmp_path):
    world = 2
    port = 29500 + (os.getpid() % 2000) + 23
    mp.start_processes(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    blocks = _two_rank_blocks()
    one = pa.GeneralIpmSolver(blocks, dual_reg=1e-9, scaler="geometric_equilibrium")
    sc = one.scaling()
    r1 = one.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    T1 = one.trace()
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
        assert int(z["res"][0]) == r1["status"] == 0 and int(z["res"][1]) == r1["iterations"]
        assert abs(z["res"][2] - r1["objective"]) <= 1e-9 * max(1.0, abs(r1["objective"]))
        # the history as test_two_rank_ipm_gpu checks it: mu and both objectives (the residual norm is a maximum of rounding-level
        # entries late in the run, where the ranks' sums differ in their last bits)
        assert z["trace"].shape == T1.shape
        assert np.allclose(z["trace"][:, [0, 2, 3]], T1[:, [0, 2, 3]], rtol=1e-6, atol=0)
        assert np.allclose(z["trace"][:, 1], T1[:, 1], rtol=1e-6, atol=1e-9 * r1["dnorm"])
    one.close()
