"""A block QP with cross Hessians on two ranks: two processes share device 0 and reduce through an ExternalComm (gloo, staged through
host memory), each owns a part of the blocks with their R_i.  (Q x)_0 = Q0 x0 + sum_i R_i^T x_i is a sum over both ranks' blocks: rank 0
contributes Q0 x0, each rank its own blocks' terms, summed with the replicated rows of the J^T product.  Both ranks must return the same
scalars and trace, and what the one-process run returns; hessian_mult's x0 part is the full sum on both; the Ruiz factors are those
of one rank (the maxima of the x0 columns of Q are reduced over the ranks)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pips_ipmpp_amd as pa
from tests import qp_cross_ref as qc

pytestmark = pytest.mark.gpu

SEED = 2   # four blocks: two leaves on rank 0, one on rank 1


def _problem(which):
    """"all": every leaf block has Q_i and R_i, the root Q0.  "rank0_only": no Hessian on the root and none on the blocks of rank 1, whose
    own blocks then have neither Q_i nor R_i - that rank must still take the QP path with the cross epilogues and hold no Q0 block.
    "twin": the badly scaled twin of "all" for the Ruiz scaler.  "twin_rank0_r": that twin with R_i on the blocks of rank 0 only, Q0 and
    every Q_i kept - rank 1 learns of the cross Hessian from the other rank: its scaler reduces the x0 maxima nevertheless, and it gives
    up the Q0 block it held while scaling.  "twin_rank0_only": the twin of "rank0_only" - rank 1 holds no Hessian at all, so its scaler has
    no Q to sweep and must send zeros for the x0 maxima at every one of the passes."""
    blocks = qc.random_lp(SEED)
    hs, rs, _ = qc.arrow_hessians(SEED, blocks, "pd")
    owner = pa.map_children_to_ranks(len(blocks) - 1, 2)
    assert (owner == 0).any() and (owner == 1).any() and all(r is not None for r in rs[1:])
    if which in ("rank0_only", "twin_rank0_only"):
        hs = [None] + [h if owner[k] == 0 else None for k, h in enumerate(hs[1:])]
        rs = [None] + [r if owner[k] == 0 else None for k, r in enumerate(rs[1:])]
    if which == "twin_rank0_r":
        rs = [None] + [r if owner[k] == 0 else None for k, r in enumerate(rs[1:])]
    if which.startswith("twin"):
        blocks, hs, rs, _ = qc.twin(blocks, hs, rs, SEED)
    return blocks, hs, rs


def _probe_vector(nx_all):
    return np.random.default_rng(11).standard_normal(nx_all)


def _worker(rank, world, port, out, which):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    blocks, hs, rs = _problem(which)
    b, h, r, mine = qc.split(blocks, hs, rs, rank, world)

    def allreduce(ptr, n):
        t = torch.as_tensor(pa.capi._DeviceDoubles(ptr, n), device="cuda")
        hst = t.cpu()
        dist.all_reduce(hst)
        t.copy_(hst)
        torch.cuda.synchronize()

    comm = pa.ExternalComm(allreduce)
    ipm = pa.GeneralIpmSolver(b, hessians=h, cross_hessians=r, comm=comm, rank=rank, n_ranks=world, scaler="ruiz" if which.startswith("twin") else None)
    off = np.concatenate([[0], np.cumsum(qc.sizes(blocks))])
    v = _probe_vector(off[-1])
    qv = ipm.hessian_mult(np.concatenate([v[:off[1]]] + [v[off[1 + k]:off[2 + k]] for k in mine]))
    sc = ipm.scaling()
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    np.savez(os.path.join(out, f"xrank{rank}.npz"), res=np.array([res[k] for k in ("status", "iterations", "objective", "dual_objective", "mu", "rnorm", "dnorm")]),
             trace=ipm.trace(), mine=mine, x=ipm.iterate()["x"], qv=qv, col=sc["col"], re=sc["row_eq"], ri=sc["row_ineq"])
    ipm.close()
    dist.barrier()
    dist.destroy_process_group()


def _two(tmp_path, which, salt):
    world = 2
    port = 29500 + (os.getpid() % 2000) + salt
    mp.start_processes(_worker, args=(world, port, str(tmp_path), which), nprocs=world, join=True, start_method="spawn")
    return [np.load(os.path.join(str(tmp_path), f"xrank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("which", ["all", "rank0_only"])
def test_two_rank_cross_qp_matches_one_rank(tmp_path, which):
    got = _two(tmp_path, which, 41 if which == "all" else 43)
    blocks, hs, rs = _problem(which)
    Q = qc.global_hessian(hs, rs, blocks)
    off = np.concatenate([[0], np.cumsum(qc.sizes(blocks))])
    n0 = off[1]
    one = pa.GeneralIpmSolver(blocks, hessians=hs, cross_hessians=rs)
    r1 = one.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    x1 = one.iterate()["x"]
    one.close()
    assert r1["status"] == 0, r1
    assert np.array_equal(got[0]["res"], got[1]["res"]) and np.array_equal(got[0]["trace"], got[1]["trace"])
    # hessian_mult: the x0 part is the full sum, equal on both ranks and scipy's; the own blocks' rows are scipy's
    want = Q @ _probe_vector(off[-1])
    assert np.array_equal(got[0]["qv"][:n0], got[1]["qv"][:n0])
    for g in got:
        w = np.concatenate([want[:n0]] + [want[off[1 + k]:off[2 + k]] for k in g["mine"]])
        err = np.abs(g["qv"] - w).max()
        print(f"hessian_mult: max error {err:.3e}, bar {1e-13 * np.abs(want).max():.3e}")
        assert err <= 1e-13 * np.abs(want).max()
    for g in got:   # the bars of tests/test_qp_two_rank_gpu.py
        status, its, obj = int(g["res"][0]), int(g["res"][1]), g["res"][2]
        assert status == 0 and abs(its - r1["iterations"]) <= 1, (g["res"], r1)
        assert abs(obj - r1["objective"]) <= 1e-8 * max(1.0, abs(r1["objective"]))
        assert g["res"][6] == r1["dnorm"]
        assert np.abs(g["x"][:n0] - x1[:n0]).max() <= 1e-6 * max(1.0, np.abs(x1).max())
        assert np.array_equal(g["trace"][:, 5], g["trace"][:, 6])


@pytest.mark.parametrize("which", ["twin", "twin_rank0_r", "twin_rank0_only"])
def test_ruiz_on_two_ranks_equals_ruiz_on_one(tmp_path, which):
    """The maxima of the x0 columns of Q hold R_i^T of both ranks' blocks: reduced like those of the replicated rows of J^T.  Every case:
    the factors of both ranks equal the one-rank factors bit for bit, the handle's product is Q' v, and both ranks return the same
    scalars and trace.  The solve is held against the one-rank run on "twin" only, whose problem is one of qc.TWINS (the restatement
    completes on it); the other two are checked for the factors, the product and the ranks' agreement."""
    got = _two(tmp_path, which, {"twin": 47, "twin_rank0_r": 53, "twin_rank0_only": 59}[which])
    blocks, hs, rs = _problem(which)
    one = pa.GeneralIpmSolver(blocks, hessians=hs, cross_hessians=rs, scaler="ruiz")
    sc = one.scaling()
    r1 = one.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    one.close()
    root = blocks[0]
    xo = np.concatenate([[0], np.cumsum(qc.sizes(blocks))])
    yo = np.concatenate([[0], np.cumsum([root["mA"] + root["mBL"]] + [b["mA"] for b in blocks[1:]])])
    zo = np.concatenate([[0], np.cumsum([root["mC"] + root["mDL"]] + [b["mC"] for b in blocks[1:]])])
    for rank, g in enumerate(got):
        pick = lambda a, o: np.concatenate([a[:o[1]]] + [a[o[1 + k]:o[2 + k]] for k in g["mine"]])   # noqa: E731
        assert np.array_equal(g["col"], pick(sc["col"], xo)), rank
        assert np.array_equal(g["re"], pick(sc["row_eq"], yo)) and np.array_equal(g["ri"], pick(sc["row_ineq"], zo)), rank
        if which == "twin":
            assert r1["status"] == 0 and int(g["res"][0]) == 0 and abs(int(g["res"][1]) - r1["iterations"]) <= 1, (g["res"], r1)
            assert abs(g["res"][2] - r1["objective"]) <= 1e-8 * max(1.0, abs(r1["objective"]))
    assert np.array_equal(got[0]["res"], got[1]["res"]) and np.array_equal(got[0]["trace"], got[1]["trace"])
    # the handle holds Q' = Cs Q Cs on both ranks (rank 1 of "twin_rank0_r" in the pattern without the Q0 block, uploaded after the scaler ran)
    want = sc["col"] * (qc.global_hessian(hs, rs, blocks) @ (sc["col"] * _probe_vector(xo[-1])))
    for g in got:
        w = np.concatenate([want[:xo[1]]] + [want[xo[1 + k]:xo[2 + k]] for k in g["mine"]])
        assert np.abs(g["qv"] - w).max() <= 1e-13 * np.abs(want).max()
