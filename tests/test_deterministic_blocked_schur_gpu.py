"""Deterministic mode on the blocked-solve Schur path (Schur mode 2, the reference's SC_COMPUTE_BLOCKWISE): every chunk of border columns
is solved by the atomics-free sweeps (one interleaved panel, or column by column) and k_border_tmult_chunk_det writes Br^T X group by group
into the group buffers with plain stores; the buffers are added into SC in the fixed tree of k_reduce_groups after the last chunk.  Asserted
here: bit-identical SC, x0, x_leaf and inertia over runs, handles and rank counts; the
same system as the default mode-2 path and deterministic mode 1; the options file's SC_COMPUTE_BLOCKWISE; and the IPM harness with
PIPS_IPM_SCHUR_MODE=2."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pips_ipmpp_amd as pa
from pips_ipmpp_amd import options
from tests.test_deterministic_gpu import _problem as _det_problem
from tests.util import Problem, hip_lower_as_rowmajor

pytestmark = pytest.mark.gpu


def _edge_problem():
    """Chunk edges: the non-empty border columns number 32 k + r with 0 < r < 8, at least one border column is empty in every block, and one
    block has no border rows at all."""
    prob = Problem(11, 8, 300, 150, 20, 50, 0.02)
    S = prob.S
    Bts = [prob.blocks[b]["Bt"].to_scipy().tolil() for b in range(prob.N)]
    Bts[5] = Bts[5] * 0.0                      # block 5: no border rows
    used = sorted(set(np.nonzero(sum(abs(B).tocsr() for B in Bts).sum(axis=1).A1)[0].tolist()))
    drop = [used[0]]                            # one border column empty in every block ...
    while (len(used) - len(drop)) % 32 not in (3,):   # ... and enough more that 32 k + 3 remain
        drop.append(used[len(drop)])
    for b in range(prob.N):
        B = Bts[b]
        for c in drop:
            B[c, :] = 0.0
        B = B.tocsr()
        B.eliminate_zeros()
        B.sort_indices()
        prob.blocks[b]["Bt"] = pa.Csr(S, prob.n_leaf, B.indptr, B.indices, B.data)
    return prob


def _problem(kind):
    return _edge_problem() if kind == "edge" else _det_problem(kind)


def _nonempty_cols(prob, blocks=None):
    used = set()
    for b in (range(prob.N) if blocks is None else blocks):
        used |= set(np.nonzero(np.diff(prob.blocks[b]["Bt"].rowptr) > 0)[0].tolist())
    return sorted(used)


def _batch(prob, mine, deterministic, mode, opts=None):
    bt = pa.LeafBatch(len(mine), prob.S)
    bt.set_deterministic(deterministic)
    if opts is not None:
        options.apply_options(opts, batch=bt)
    elif mode is not None:
        bt.set_schur_mode(mode)
    for i, b in enumerate(mine):
        bt.set_block(i, prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"])
    bt.analyze(4)
    for i, b in enumerate(mine):
        bt.set_values(i, prob.blocks[b]["K"].val)
    return bt


def _run(prob, mine, deterministic, mode=2, comm=None, rank=0, world=1, reps=3, opts=None):
    S = prob.S
    bt = _batch(prob, mine, deterministic, mode, opts)
    kkt = pa.KktSystem(bt, prob.n0, 0, prob.myl, 0, F0=prob.F0, comm=comm, rank=rank, n_ranks=world)
    diag = torch.tensor(np.concatenate([prob.blocks[b]["diag"] for b in mine]), device="cuda")
    xd0 = torch.tensor(prob.x_diag0, device="cuda")
    rng = np.random.default_rng(0)
    b0_full = rng.standard_normal(S)
    bs_full = [rng.standard_normal(prob.n_leaf) for _ in range(prob.N)]
    out = []
    for _ in range(reps):
        kkt.factorize(diag, xd0)
        SC = kkt.schur_to_host().copy()
        b0 = torch.tensor(b0_full, device="cuda")
        bl = torch.tensor(np.concatenate([bs_full[b] for b in mine]), device="cuda")
        kkt.solve_compressed(b0, bl)
        bt.sync()
        out.append(dict(SC=SC, x0=b0.cpu().numpy(), xl=bl.cpu().numpy().reshape(len(mine), -1), mode=bt.schur_mode(),
                        inertia=[bt.inertia(i) for i in range(len(mine))] + [kkt.root_inertia()]))
    kkt.close()
    bt.close()
    return out


def _assert_bit_identical(runs):
    for r in runs[1:]:
        assert np.array_equal(r["SC"], runs[0]["SC"]) and np.array_equal(r["x0"], runs[0]["x0"]) and np.array_equal(r["xl"], runs[0]["xl"])
        assert r["inertia"] == runs[0]["inertia"]


def _leaf_schur(prob, deterministic, mode=2):
    """The leaves' Schur contribution alone (pips_hip_batch_factor), row-major lower triangle."""
    S = prob.S
    bt = _batch(prob, list(range(prob.N)), deterministic, mode)
    SC = torch.zeros(S * S, dtype=torch.float64, device="cuda")
    bt.factor(SC, S)
    bt.sync()
    got = hip_lower_as_rowmajor(SC.cpu().numpy(), S)
    bt.close()
    return got


@pytest.mark.parametrize("kind", ["random", "banded", "edge"])
def test_bit_identical_over_runs_and_handles(kind):
    prob = _problem(kind)
    if kind == "edge":
        cols = _nonempty_cols(prob)
        assert 0 < len(cols) % 32 < 8 and len(cols) > 32 and len(cols) < prob.S
        assert prob.blocks[5]["Bt"].rowptr[-1] == 0
        assert all(len(_nonempty_cols(prob, [b])) < prob.S for b in range(prob.N))
    mine = list(range(prob.N))
    runs = _run(prob, mine, True) + _run(prob, mine, True)
    assert all(r["mode"] == 2 for r in runs)
    _assert_bit_identical(runs)
    # the same system as the default mode-2 path and as deterministic mode 1
    for ref in (_run(prob, mine, False, mode=2, reps=1)[0], _run(prob, mine, True, mode=1, reps=1)[0]):
        assert np.abs(ref["SC"] - runs[0]["SC"]).max() <= 1e-9 * np.abs(ref["SC"]).max()
        assert np.linalg.norm(ref["xl"] - runs[0]["xl"]) <= 1e-8 * np.linalg.norm(ref["xl"])
        assert ref["inertia"] == runs[0]["inertia"]
    # the leaves' contribution against the reference's blocked loop (addTermToSchurComplBlocked)
    got = _leaf_schur(prob, True)
    assert np.array_equal(got, _leaf_schur(prob, True))
    want = np.tril(prob.oracle_schur())
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def _worker(rank, world, port, out, kind):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    prob = _problem(kind)
    mine = [int(b) for b in np.nonzero(pa.map_children_to_ranks(prob.N, world) == rank)[0]]

    def allreduce(ptr, n):
        t = torch.as_tensor(pa.capi._DeviceDoubles(ptr, n), device="cuda")
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)
        torch.cuda.synchronize()

    calls = []

    def all_gather(ptr, chunk):     # in place: rank r's part at r * chunk
        t = torch.as_tensor(pa.capi._DeviceDoubles(ptr, chunk * world), device="cuda")
        h = t.cpu()
        parts = [torch.empty(chunk, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(parts, h[rank * chunk:(rank + 1) * chunk].clone())
        t.copy_(torch.cat(parts))
        torch.cuda.synchronize()
        calls.append(chunk)

    def reduce_scatter(ptr, chunk):
        allreduce(ptr, chunk * world)

    comm = pa.ExternalComm(allreduce, reduce_scatter, all_gather, n_ranks=world, rank=rank) if world == 4 else pa.ExternalComm(allreduce)
    r = _run(prob, mine, True, comm=comm, rank=rank, world=world, reps=2)
    assert r[0]["mode"] == 2
    assert world != 4 or len(calls) >= 4        # two factorisations + two solveCompressed went through the all-gather
    _assert_bit_identical(r)
    np.savez(os.path.join(out, f"det{rank}.npz"), SC=r[0]["SC"], x0=r[0]["x0"], xl=r[0]["xl"], mine=np.array(mine), inertia=np.array(r[0]["inertia"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kind,world", [("random", 2), ("banded", 2), ("random", 4), ("edge", 4), ("banded", 8)])
def test_bit_identical_between_one_and_several_ranks(tmp_path, kind, world):
    """Every rank solves only its own non-empty border columns, so a column lands in another lane / chunk than on one rank, and the panel
    slicing would follow the rank's tile-row tasks: the column's bits must not move (pinned slicing, one column per lane)."""
    port = 31500 + (os.getpid() % 2000) + {"random": 41, "banded": 43}.get(kind, 47) + 3 * world
    mp.start_processes(_worker, args=(world, port, str(tmp_path), kind), nprocs=world, join=True, start_method="spawn")
    prob = _problem(kind)
    one = _run(prob, list(range(prob.N)), True, reps=1)[0]
    for r in range(world):
        g = np.load(os.path.join(str(tmp_path), f"det{r}.npz"))
        assert np.array_equal(g["SC"], one["SC"])
        assert np.array_equal(g["x0"], one["x0"])
        for i, b in enumerate(g["mine"]):
            assert np.array_equal(g["xl"][i], one["xl"][b])
            assert tuple(g["inertia"][i]) == one["inertia"][b]
        assert tuple(g["inertia"][-1]) == one["inertia"][-1]


def test_options_file_blockwise_on_a_deterministic_batch():
    prob = _problem("random")
    mine = list(range(prob.N))
    runs = _run(prob, mine, True, opts={"SC_COMPUTE_BLOCKWISE": True}, reps=2)
    assert runs[0]["mode"] == 2
    _assert_bit_identical(runs)
    ref = _run(prob, mine, False, mode=2, reps=1)[0]
    assert np.all(np.isfinite(runs[0]["xl"])) and np.all(np.isfinite(runs[0]["x0"]))
    assert np.linalg.norm(ref["xl"] - runs[0]["xl"]) <= 1e-8 * np.linalg.norm(ref["xl"])
    assert np.linalg.norm(ref["x0"] - runs[0]["x0"]) <= 1e-8 * np.linalg.norm(ref["x0"])


def test_ipm_blocked_schur_is_bit_reproducible(monkeypatch):
    """PIPS_HIP_DETERMINISTIC=1 + PIPS_IPM_SCHUR_MODE=2 on a GAMSsmall instance with linking rows: the whole run repeats to the bit and
    reaches the objective of deterministic mode 1."""
    monkeypatch.setenv("PIPS_HIP_DETERMINISTIC", "1")
    data = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gamssmall.json")))["instances"]
    inst = [d for d in data if d["name"] == "singletonInequalityColumn_B0Bl0"][0]
    assert any(b["mBL"] + b["mDL"] > 0 for b in inst["blocks"][1:])

    def solve(mode):
        monkeypatch.setenv("PIPS_IPM_SCHUR_MODE", str(mode))
        ipm = pa.GeneralIpmSolver(inst["blocks"], dual_reg=1e-9)
        got_mode = ipm.schur_mode()
        res = ipm.solve(max_iter=200, mutol=1e-8, artol=1e-8)
        out = (got_mode, res, ipm.trace().tobytes(), ipm.iterate()["x"].tobytes(), ipm.iterate()["z"].tobytes())
        ipm.close()
        return out

    runs = [solve(2) for _ in range(3)]
    for mode, res, *_ in runs:
        assert mode == 2
        assert res["status"] == 0 and abs(res["objective"] - inst["expected_objective"]) < 1e-4
    key = [(r[1]["iterations"],) + tuple(r[2:]) for r in runs]
    assert all(k == key[0] for k in key)
    mode1, res1, *_ = solve(1)
    assert mode1 == 1
    assert abs(res1["objective"] - runs[0][1]["objective"]) <= 1e-8 * max(1.0, abs(res1["objective"]))
