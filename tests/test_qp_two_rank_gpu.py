"""A block QP on two ranks: two processes share device 0 and reduce through an ExternalComm (gloo, staged through host memory), each
owns a part of the blocks and both hold Q0.  Q0 x0 is replicated - every rank computes it, only rank 0 adds it to the replicated
rows that are summed - so both ranks must return the same scalars, and what the one-process run returns."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pips_ipmpp_amd as pa
from tests.general_lp_gen import random_block_lp
from tests.qp_ref import block_hessians

pytestmark = pytest.mark.gpu

SEED = 2


def _problem(which="all"):
    """which = "rank0_leaf_only": no Hessian on the root and none on the blocks of rank 1 - that rank must still take the QP path (the
    ranks agree on it at creation: the fused reductions are collectives and the step-length rule steers the replicated iterate)"""
    rng = np.random.default_rng(SEED)   # seed 2 of the family of tests/test_native_general_gpu.py
    nb = int(rng.integers(2, 5))
    blocks = random_block_lp(100 + SEED, nb, int(rng.integers(4, 9)), int(rng.integers(8, 20)), int(rng.integers(2, 6)), int(rng.integers(1, 5)),
                             int(rng.integers(1, 4)), int(rng.integers(1, 4)), free_fraction=0.0)
    hs, _ = block_hessians(SEED, blocks, "pd")
    if which == "rank0_leaf_only":
        owner = pa.map_children_to_ranks(len(blocks) - 1, 2)
        assert (owner == 0).any() and (owner == 1).any()
        hs = [None] + [h if owner[k] == 0 else None for k, h in enumerate(hs[1:])]
    return blocks, hs


def _worker(rank, world, port, out, which):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    blocks, hs = _problem(which)
    mine = np.nonzero(pa.map_children_to_ranks(len(blocks) - 1, world) == rank)[0]

    def allreduce(ptr, n):
        t = torch.as_tensor(pa.capi._DeviceDoubles(ptr, n), device="cuda")
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)
        torch.cuda.synchronize()

    comm = pa.ExternalComm(allreduce)
    ipm = pa.GeneralIpmSolver([blocks[0]] + [blocks[1 + k] for k in mine], hessians=[hs[0]] + [hs[1 + k] for k in mine], comm=comm, rank=rank,
                              n_ranks=world)
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    np.savez(os.path.join(out, f"qrank{rank}.npz"), res=np.array([res[k] for k in ("status", "iterations", "objective", "dual_objective", "mu", "rnorm", "dnorm")]),
             trace=ipm.trace(), mine=mine, x=ipm.iterate()["x"])
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("which", ["all", "rank0_leaf_only"])
def test_two_rank_qp_matches_one_rank(tmp_path, which):
    world = 2
    port = 29500 + (os.getpid() % 2000) + (29 if which == "all" else 31)
    mp.start_processes(_worker, args=(world, port, str(tmp_path), which), nprocs=world, join=True, start_method="spawn")
    blocks, hs = _problem(which)
    n0 = int(blocks[0]["n0"])
    one = pa.GeneralIpmSolver(blocks, hessians=hs)
    r1 = one.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    x1 = one.iterate()["x"]
    assert r1["status"] == 0, r1
    got = [np.load(os.path.join(str(tmp_path), f"qrank{r}.npz")) for r in range(world)]
    assert np.array_equal(got[0]["res"], got[1]["res"]) and np.array_equal(got[0]["trace"], got[1]["trace"])
    for g in got:
        status, its, obj = int(g["res"][0]), int(g["res"][1]), g["res"][2]
        assert status == 0 and abs(its - r1["iterations"]) <= 1, (g["res"], r1)
        assert abs(obj - r1["objective"]) <= 1e-8 * max(1.0, abs(r1["objective"]))
        assert g["res"][6] == r1["dnorm"]
        assert np.abs(g["x"][:n0] - x1[:n0]).max() <= 1e-6 * max(1.0, np.abs(x1).max())
        assert np.array_equal(g["trace"][:, 5], g["trace"][:, 6])
