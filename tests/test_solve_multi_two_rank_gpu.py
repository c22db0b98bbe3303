"""KktSystem.solve_compressed_multi over two ranks: two processes share device 0 and reduce through the gloo ExternalComm, started as
tests/test_two_rank_gpu.py starts its ranks.  Each rank owns its contiguous share of the blocks and passes the full root columns and its
own part of the leaf columns; the panel path ends its Lsolve with ONE all-reduce of S x nrhs doubles per chunk (deterministic mode with a
rank count that divides eight: one all-gather of the group panels instead), which the recorded collective sizes show.

`small` with the dense root and `two_link_6` with the sparse root, nrhs = 33 (one chunk, a panel and one column), default mode and
deterministic mode.  The columns are those of tests/solve_multi_cases.py and every one is judged against the long-double arrowhead
reference (root part of rank 0, leaf parts from their owners), as tests/test_solve_multi_judged_gpu.py judges them.  Both ranks hold the
same root part to the bit: T = -sum_i Br_i^T Z_i is summed over the ranks on its own and then added to the same panel on every rank.  In
deterministic mode a repeated call gives the same bits on both ranks.

Measured on an MI355X (the largest ratio over columns, cases and modes) and the margin by the rule of DESIGN.md section 6:

    group       backward                        root_rows                     forward_root                   forward_leaf                   M
    two_rank    3.92 (small, deterministic)     1.25 (small, deterministic)   2.04 (small, deterministic)    3.07 (small, deterministic)    16

The module is one group with one margin.  Its parts: small in default mode 1.39, 1.18, 1.09, 1.86; two_link_6 at most 0.33, 0.33, 0.51, 0.52.
"""
import os
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pips_ipmpp_amd as pa
from tests import solve_multi_cases as smc
from tests import util as u

pytestmark = pytest.mark.gpu

M = 16      # the smallest power of two >= 4 x the largest measured ratio (see above); never above 64
NRHS = 33
CASES = {"small": False, "two_link_6": True}        # case -> sparse root


def _worker(rank, world, port, out, case):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    for k in ("PIPS_HIP_MULTI", "PIPS_HIP_FORCE_REDUCE", "PIPS_HIP_AUG_SWEEPS"):
        os.environ.pop(k, None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sparse_root = CASES[case]
    prob, scale = u.arrowhead_problem(case)
    sysm = u.ArrowheadSystem(prob, scale)
    B0, BL = u.arrowhead_rhs(sysm, smc.seed(case))
    C0, CL = smc.columns(types.SimpleNamespace(B0=B0, BL=BL), NRHS)
    mine = np.nonzero(pa.map_children_to_ranks(sysm.N, world) == rank)[0]
    CLm = np.ascontiguousarray(CL.reshape(NRHS, sysm.N, sysm.n_leaf)[:, mine, :].reshape(NRHS, -1))
    calls = []

    def allreduce(ptr, n):
        t = torch.as_tensor(pa.capi._DeviceDoubles(ptr, n), device="cuda")
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)
        torch.cuda.synchronize()
        calls.append(n)

    comm = pa.ExternalComm(allreduce)
    cols = [np.nonzero(np.diff(prob.blocks[b]["Bt"].rowptr) > 0)[0] for b in range(sysm.N)] if sparse_root else None
    saved = {}
    for mode in ("default", "deterministic"):
        bt = pa.LeafBatch(len(mine), sysm.S, device=0)
        if mode == "deterministic":
            bt.set_deterministic(True)
        if sparse_root:
            bt.set_schur_mode(1)
        for i, b in enumerate(mine):
            bt.set_block(i, prob.blocks[b]["K"], sysm.n_primal, prob.blocks[b]["Bt"])
        bt.analyze(2)
        bt.set_refinement_backward_error(2, 1e-15)
        for i, b in enumerate(mine):
            bt.set_values(i, prob.blocks[b]["K"].val)
        kkt = pa.KktSystem(bt, sysm.n0, 0, sysm.myl, 0, F0=prob.F0, comm=comm, rank=rank, n_ranks=world, sparse_root=sparse_root, all_block_cols=cols)
        kkt.factorize(torch.tensor(np.concatenate([prob.blocks[b]["diag"] for b in mine]), device="cuda"), torch.tensor(sysm.x_diag0, device="cuda"))
        saved[f"{mode}_leaf_inertia"] = np.array([bt.inertia(i) for i in range(len(mine))])
        saved[f"{mode}_root_inertia"] = np.array(kkt.root_inertia())
        for rep in ("first", "repeated") if mode == "deterministic" else ("first",):
            X0, XL = torch.tensor(C0, device="cuda"), torch.tensor(CLm, device="cuda")
            del calls[:]
            kkt.solve_compressed_multi(X0, XL)
            bt.sync()
            saved[f"{mode}_{rep}_x0"], saved[f"{mode}_{rep}_xl"] = X0.cpu().numpy(), XL.cpu().numpy()
            saved[f"{mode}_{rep}_calls"] = np.array(calls)
            i = kkt.solve_multi_info()
            saved[f"{mode}_{rep}_info"] = np.array([i["path"], i["chunks"], i["per_chunk"]])
        kkt.close()
        bt.close()
    np.savez(os.path.join(out, f"rank{rank}.npz"), blocks=np.array(mine), **saved)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", list(CASES))
def test_two_ranks_solve_a_panel(tmp_path, case):
    world = 2
    port = 29500 + (os.getpid() % 2000) + 11 + list(CASES).index(case)
    mp.start_processes(_worker, args=(world, port, str(tmp_path), case), nprocs=world, join=True, start_method="spawn")
    ref = u.arrowhead_reference(case)
    s = ref.sys
    g = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(world)]
    assert sorted(int(b) for r in range(world) for b in g[r]["blocks"]) == list(range(s.N))
    largest = {}
    for mode in ("default", "deterministic"):
        for r in range(world):
            assert [tuple(t) for t in g[r][f"{mode}_leaf_inertia"]] == [ref.leaf_inertia[b] for b in g[r]["blocks"]]
            assert tuple(g[r][f"{mode}_root_inertia"]) == ref.root_inertia == (s.n0, s.S - s.n0, 0)
        for rep in ("first", "repeated") if mode == "deterministic" else ("first",):
            XL = np.empty((NRHS, s.N, s.n_leaf))
            for r in range(world):
                assert list(g[r][f"{mode}_{rep}_info"]) == [1, 1, NRHS]
                XL[:, g[r]["blocks"], :] = g[r][f"{mode}_{rep}_xl"].reshape(NRHS, len(g[r]["blocks"]), s.n_leaf)
                # the one collective of the chunk's Lsolve carries S x nrhs doubles (all eight group panels where they are gathered); the other
                # collectives of the call are single numbers and the ranks' leaf lengths
                big = [int(n) for n in g[r][f"{mode}_{rep}_calls"] if n > world]
                assert big == [(8 if mode == "deterministic" else 1) * s.S * NRHS], (mode, rep, r, big)
            X0 = g[0][f"{mode}_{rep}_x0"]
            assert np.array_equal(X0, g[1][f"{mode}_{rep}_x0"]), (mode, rep)
            XL = XL.reshape(NRHS, -1)
            ratios = smc.ratios(ref, X0, XL)
            print(f"solve-multi-two-rank case={case} mode={mode} {rep} " + " ".join(f"{name}={v.max():.4g}@{int(v.argmax())}" for name, v in ratios.items()))
            for name, v in ratios.items():
                largest[name] = max(largest.get(name, 0.0), float(v.max()))
            for j in range(smc.N_BASES - 1, NRHS, smc.N_BASES):
                assert not X0[j].any() and not XL[j].any(), j
            ok = smc.accepts(ref, X0, XL, M)
            assert ok.all(), (mode, rep, list(np.nonzero(~ok)[0]), {name: v[~ok] for name, v in ratios.items()})
        for r in range(world):
            if mode == "deterministic":
                assert np.array_equal(g[r]["deterministic_first_x0"], g[r]["deterministic_repeated_x0"])
                assert np.array_equal(g[r]["deterministic_first_xl"], g[r]["deterministic_repeated_xl"])
    print(f"\nsolve-multi-group group=two_rank/{case} " + " ".join(f"{name}={v:.4g}" for name, v in largest.items()) + f" M={M}")
