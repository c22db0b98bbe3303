"""Schur mode 2 (blocked solves) with the sparse root: the border columns packed block by block.  Right-hand side q of a chunk carries, in every
block, that block's q-th non-empty border column, so one interleaved sweep solves a different Schur column in every block and the products go to
the root's CSR value array through the block's position table (k_border_rows_to_dense_packed, k_border_tmult_chunk_packed and, without FP64
atomics, k_border_tmult_chunk_packed_det).  Every case asserts schur_mode() == 2 and info()["packed_schur_rhs"] == max_b nb_b, the latter from
the Bt row pointers.

  1. the finalised value array judged against the long-double reference of tests/test_schur_judged_gpu.py (its predicate, its margin for mode 2:
     the solves and the row dot products are those of the dense mode-2 path, only the target address differs) at S = 32, 33 (the chunk boundary of
     the local column index: nb = S), 129 (five chunks) and the heterogeneous borders (blocks with fewer columns than a chunk has slots);
     lower triangular, nothing outside the pattern touched.
  2. 2-link chains against the dense oracle at the bounds of test_sparse_root_matches_dense_oracle: value array, root inertia, solveCompressed
     (path 0), and the mode-1 sparse-root handle on the same problem.  The second shape packs 585 Schur columns into at most 45.
  3. auto mode (0) with the sparse root no longer raises, whichever mode the cost model took.
  4. a second factorize with the same diagonals: judged against SC*, not 2 SC*.
  5. the reduction with a global pattern and a communicator: one reduction of nnz doubles.
  6. deterministic mode: bit-identical over three factorisations, two handles, the three root orders, and between one rank and two.
  7. the IPM harness with PIPS_IPM_SPARSE_ROOT=1 and PIPS_IPM_SCHUR_MODE=2 (and 1) on four random LPs against HiGHS.
"""
import os

import numpy as np
import pytest

import pips_ipmpp_amd as pa
from oracle import oracle as orc
from tests import util as u
from tests.test_schur_judged_gpu import M
from tests.test_sparse_root_gpu import TwoLinkProblem

pytestmark = pytest.mark.gpu


def _nb_max(prob, blocks=None):
    """max_b nb_b from the Bt row pointers"""
    blocks = range(prob.N) if blocks is None else blocks
    return max(int((np.diff(np.asarray(prob.blocks[b]["Bt"].rowptr)) > 0).sum()) for b in blocks)


def _build(prob, mode, sparse_root=True, deterministic=None, **kw):
    bt = pa.LeafBatch(prob.N, prob.S)
    bt.set_schur_mode(mode)
    if deterministic is not None:
        bt.set_deterministic(deterministic)
    for b in range(prob.N):
        bt.set_block(b, prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"])
    bt.analyze(2)
    for b in range(prob.N):
        bt.set_values(b, prob.blocks[b]["K"].val)
    kkt = pa.KktSystem(bt, prob.n0, 0, prob.myl, 0, F0=prob.F0, sparse_root=sparse_root, **kw)
    return bt, kkt


def _assert_packed(bt, prob):
    assert bt.schur_mode() == 2
    assert bt.info()["packed_schur_rhs"] == _nb_max(prob)


def _diags(prob):
    import torch
    return torch.tensor(np.concatenate([b["diag"] for b in prob.blocks]), device="cuda"), torch.tensor(prob.x_diag0, device="cuda")


def _pattern(SCs, S):
    pat = np.zeros((S, S), bool)
    rp, ci = SCs.indptr, SCs.indices
    for r in range(S):
        pat[r, ci[rp[r]:rp[r + 1]]] = True
    return pat


def _judge(ref, got, path):
    r = ref.ratio(got)
    print(f"schur-ratio path={path} ratio={r:.4g}")
    assert M[2] <= u.UNREFINED_M_CAP
    assert ref.accepts(got, M[2]), (path, r, ref.err_ref0, ref.scale)


# ---- 1. the value array judged -------------------------------------------------------------------------------------------------------------------
_JUDGED = [k for k in u.SCHUR_PROBLEMS if k[2] == 3 and (k[3] == "hetero" or k[1] in (32, 33, 129))]


def _key_id(key):
    return f"{key[0]}-S{key[1]}" + ("-hetero" if key[3] == "hetero" else "")


@pytest.mark.parametrize("key", _JUDGED, ids=[_key_id(k) for k in _JUDGED])
def test_value_array_judged(key):
    ref = u.schur_reference(key, finalized=True)
    prob = ref.prob
    bt, kkt = _build(prob, 2)
    _assert_packed(bt, prob)
    assert bt.info()["packed_schur_rhs"] == key[1]          # (block 0 holds every column, in the heterogeneous case too)
    kkt.factorize(*_diags(prob))
    SCs = kkt.schur_sparse_to_host()
    bt.sync()
    assert [bt.inertia(i) for i in range(prob.N)] == [(prob.n_i, prob.my_i, 0)] * prob.N
    kkt.close()
    bt.close()
    got = SCs.toarray()
    assert not np.triu(got, 1).any()                        # a lower-triangular value array
    assert not ref.SC_star[~_pattern(SCs, prob.S)].any()    # nothing of the true matrix falls outside the pattern (and nothing else is stored)
    _judge(ref, got, f"packed/{_key_id(key)}")


# ---- 2. chains against the dense oracle ----------------------------------------------------------------------------------------------------------
_chain_cache = {}


def _chain(shape):
    """the problem and what the oracle says about it, computed once per shape"""
    if shape not in _chain_cache:
        N, n_i, my_i, n0, L = shape
        prob = TwoLinkProblem(77, N, n_i, my_i, n0, L, 5.0 / n_i)
        want = np.tril(prob.oracle_finalize(prob.oracle_schur()))
        want.setflags(write=False)
        _chain_cache[shape] = (prob, want)
    return _chain_cache[shape]


@pytest.mark.parametrize("shape", [(6, 120, 60, 4, 3), (30, 60, 30, 5, 20)])
def test_chain_matches_dense_oracle(shape):
    import torch
    N, n_i, my_i, n0, L = shape
    prob, want = _chain(shape)
    S = prob.S
    bt, kkt = _build(prob, 2)
    _assert_packed(bt, prob)
    assert bt.info()["packed_schur_rhs"] <= n0 + 2 * L
    diag, xd0 = _diags(prob)
    kkt.factorize(diag, xd0)
    SCs = kkt.schur_sparse_to_host()
    pat = _pattern(SCs, S)
    assert np.abs(want[~pat]).max() == 0.0
    got = SCs.toarray()
    assert not np.triu(got, 1).any()
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-9
    assert kkt.root_inertia() == (prob.n0, prob.myl, 0)
    rng = np.random.default_rng(3)
    b0, bl = rng.standard_normal(S), rng.standard_normal(N * prob.n_leaf)
    b0_d, bl_d = torch.tensor(b0, device="cuda"), torch.tensor(bl, device="cuda")
    kkt.solve_compressed(b0_d, bl_d)
    bt.sync()
    assert kkt.last_solve_path() == 0
    root = orc.DenseRootSolver(S)
    root.matrixChanged(np.array(want))
    b0_o, bs_o = b0.copy(), [bl.reshape(N, -1)[b].copy() for b in range(N)]
    orc.solve_compressed(b0_o, bs_o, [prob.oracle_leaf(b) for b in range(N)], [prob.Bt_scipy(b) for b in range(N)], root, prob.n0, 0, 0, prob.myl, 0)
    assert np.linalg.norm(b0_d.cpu().numpy() - b0_o) / np.linalg.norm(b0_o) < 1e-8
    xl = bl_d.cpu().numpy().reshape(N, -1)
    for b in range(N):
        assert np.linalg.norm(xl[b] - bs_o[b]) / np.linalg.norm(bs_o[b]) < 1e-8
    # the mode-1 sparse-root handle on the same problem: the same pattern, value array and answer
    bt1, kkt1 = _build(prob, 1)
    assert bt1.schur_mode() == 1 and bt1.info()["packed_schur_rhs"] == 0
    kkt1.factorize(diag, xd0)
    SC1 = kkt1.schur_sparse_to_host()
    assert np.array_equal(SC1.indptr, SCs.indptr) and np.array_equal(SC1.indices, SCs.indices)
    assert np.abs(SC1.data - SCs.data).max() / np.abs(SC1.data).max() < 1e-8
    c0_d, cl_d = torch.tensor(b0, device="cuda"), torch.tensor(bl, device="cuda")
    kkt1.solve_compressed(c0_d, cl_d)
    bt1.sync()
    assert np.linalg.norm((c0_d - b0_d).cpu().numpy()) / np.linalg.norm(b0_o) < 1e-8
    assert np.linalg.norm((cl_d - bl_d).cpu().numpy()) / np.linalg.norm(np.concatenate(bs_o)) < 1e-8
    for h in (kkt, bt, kkt1, bt1):
        h.close()


# ---- 3. auto mode --------------------------------------------------------------------------------------------------------------------------------
def test_auto_mode_with_the_sparse_root():
    prob, want = _chain((9, 300, 150, 6, 8))
    bt, kkt = _build(prob, 0)                                # (raised "a sparse Schur complement needs Schur mode 1" where the model took 2)
    mode = bt.schur_mode()
    assert mode in (1, 2) and bt.info()["packed_schur_rhs"] == (_nb_max(prob) if mode == 2 else 0)
    kkt.factorize(*_diags(prob))
    got = kkt.schur_sparse_to_host().toarray()
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-9
    kkt.close()
    bt.close()


# ---- 4. second factorisation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
def test_second_factorisation(deterministic):
    key = (170, 129, 3, "hetero")
    ref = u.schur_reference(key, finalized=True)
    prob = ref.prob
    bt, kkt = _build(prob, 2, deterministic=deterministic)
    _assert_packed(bt, prob)
    diag, xd0 = _diags(prob)
    for n in ("first", "second", "third"):                  # judged against SC* every time, never against a multiple of it
        kkt.factorize(diag, xd0)
        got = kkt.schur_sparse_to_host().toarray()
        _judge(ref, got, f"packed_refactor/{'det' if deterministic else 'atomic'}/{n}")
    kkt.close()
    bt.close()


# ---- 5. global pattern with a communicator -------------------------------------------------------------------------------------------------------
def test_reduction_with_global_pattern(monkeypatch):
    monkeypatch.setenv("PIPS_HIP_FORCE_REDUCE", "1")
    prob = TwoLinkProblem(78, 5, 150, 75, 4, 4, 5.0 / 150)
    seen = []

    def allreduce(ptr, n):
        seen.append(n)

    comm = pa.ExternalComm(allreduce)
    cols = [np.nonzero(np.diff(prob.blocks[b]["Bt"].rowptr) > 0)[0] for b in range(prob.N)]
    bt, kkt = _build(prob, 2, comm=comm, rank=0, n_ranks=1, all_block_cols=cols)
    _assert_packed(bt, prob)
    kkt.factorize(*_diags(prob))
    SCs = kkt.schur_sparse_to_host()
    want = np.tril(prob.oracle_finalize(prob.oracle_schur()))
    assert seen == [SCs.nnz]
    assert np.abs(SCs.toarray() - want).max() / np.abs(want).max() < 1e-9
    kkt.close()
    bt.close()
    comm.close()


# ---- 6. deterministic mode -----------------------------------------------------------------------------------------------------------------------
_ROOT_ORDER = {"band": "1", "amd": "0", "dissected": "2"}


def _det_problem():
    return TwoLinkProblem(94, 8, 600, 300, 5, 16, 5.0 / 600)


def _run(prob, mine, deterministic, comm=None, rank=0, world=1, reps=3):
    import torch
    S = prob.S
    bt = pa.LeafBatch(len(mine), S)
    bt.set_schur_mode(2)
    bt.set_deterministic(deterministic)
    for i, b in enumerate(mine):
        bt.set_block(i, prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"])
    bt.analyze(4)
    for i, b in enumerate(mine):
        bt.set_values(i, prob.blocks[b]["K"].val)
    cols = [np.nonzero(np.diff(prob.blocks[b]["Bt"].rowptr) > 0)[0] for b in range(prob.N)]
    kkt = pa.KktSystem(bt, prob.n0, 0, prob.myl, 0, F0=prob.F0, comm=comm, rank=rank, n_ranks=world, sparse_root=True, all_block_cols=cols)
    assert bt.schur_mode() == 2 and bt.info()["packed_schur_rhs"] == _nb_max(prob, mine)
    diag = torch.tensor(np.concatenate([prob.blocks[b]["diag"] for b in mine]), device="cuda")
    xd0 = torch.tensor(prob.x_diag0, device="cuda")
    rng = np.random.default_rng(0)
    b0_full = rng.standard_normal(S)
    bs_full = [rng.standard_normal(prob.n_leaf) for _ in range(prob.N)]
    out = []
    for _ in range(reps):
        kkt.factorize(diag, xd0)
        SC = kkt.schur_sparse_to_host().data.copy()
        b0 = torch.tensor(b0_full, device="cuda")
        bl = torch.tensor(np.concatenate([bs_full[b] for b in mine]), device="cuda")
        kkt.solve_compressed(b0, bl)
        bt.sync()
        assert kkt.last_solve_path() == 0
        out.append(dict(SC=SC, x0=b0.cpu().numpy(), xl=bl.cpu().numpy().reshape(len(mine), -1),
                        inertia=[bt.inertia(i) for i in range(len(mine))] + [kkt.root_inertia()]))
    kkt.close()
    bt.close()
    return out


@pytest.mark.parametrize("order", list(_ROOT_ORDER))
def test_deterministic_bit_identical_over_runs_and_handles(order, monkeypatch):
    monkeypatch.setenv("PIPS_HIP_SPARSE_ROOT_BAND", _ROOT_ORDER[order])
    prob = _det_problem()
    mine = list(range(prob.N))
    runs = _run(prob, mine, True) + _run(prob, mine, True)
    for r in runs[1:]:
        assert np.array_equal(r["SC"], runs[0]["SC"]) and np.array_equal(r["x0"], runs[0]["x0"]) and np.array_equal(r["xl"], runs[0]["xl"])
        assert r["inertia"] == runs[0]["inertia"]
    ref = _run(prob, mine, False, reps=1)[0]                # the same system the atomic path solves
    assert np.abs(ref["SC"] - runs[0]["SC"]).max() <= 1e-9 * np.abs(ref["SC"]).max()
    assert np.linalg.norm(ref["x0"] - runs[0]["x0"]) <= 1e-8 * np.linalg.norm(ref["x0"])
    assert np.linalg.norm(ref["xl"] - runs[0]["xl"]) <= 1e-8 * np.linalg.norm(ref["xl"])
    assert ref["inertia"] == runs[0]["inertia"]


def _worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    prob = _det_problem()
    mine = [int(b) for b in np.nonzero(pa.map_children_to_ranks(prob.N, world) == rank)[0]]

    def allreduce(ptr, n):
        t = torch.as_tensor(pa.capi._DeviceDoubles(ptr, n), device="cuda")
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)
        torch.cuda.synchronize()

    r = _run(prob, mine, True, comm=pa.ExternalComm(allreduce), rank=rank, world=world, reps=2)
    assert np.array_equal(r[0]["SC"], r[1]["SC"]) and np.array_equal(r[0]["xl"], r[1]["xl"])
    np.savez(os.path.join(out, f"det{rank}.npz"), SC=r[0]["SC"], x0=r[0]["x0"], xl=r[0]["xl"], mine=np.array(mine), inertia=np.array(r[0]["inertia"]))
    dist.barrier()
    dist.destroy_process_group()


def test_deterministic_bit_identical_between_one_and_two_ranks(tmp_path, monkeypatch):
    import torch.multiprocessing as mp
    monkeypatch.setenv("PIPS_HIP_SPARSE_ROOT_BAND", _ROOT_ORDER["dissected"])   # (inherited by the spawned ranks)
    world = 2
    port = 29500 + (os.getpid() % 2000) + 53 + 3 * world
    mp.start_processes(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    prob = _det_problem()
    one = _run(prob, list(range(prob.N)), True, reps=1)[0]
    for r in range(world):
        g = np.load(os.path.join(str(tmp_path), f"det{r}.npz"))
        assert np.array_equal(g["SC"], one["SC"])
        assert np.array_equal(g["x0"], one["x0"])
        for i, b in enumerate(g["mine"]):
            assert np.array_equal(g["xl"][i], one["xl"][b])
            assert tuple(g["inertia"][i]) == one["inertia"][b]
        assert tuple(g["inertia"][-1]) == one["inertia"][-1]


# ---- 7. the harness ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 1])
@pytest.mark.parametrize("seed", range(4))
def test_harness_sparse_root(seed, mode, monkeypatch):
    """PIPS_IPM_SPARSE_ROOT=1 with PIPS_IPM_SCHUR_MODE set is honoured: status 0 and the optimum of HiGHS, seeds 0 .. 3 in both modes."""
    from oracle import ipm_oracle as io
    from tests.test_native_general_gpu import _highs, _random_lp
    monkeypatch.setenv("PIPS_IPM_SPARSE_ROOT", "1")
    monkeypatch.setenv("PIPS_IPM_SCHUR_MODE", str(mode))
    blocks = _random_lp(seed, 0.0)
    ref = _highs(io.assemble(blocks))
    assert ref.status == 0
    ipm = pa.GeneralIpmSolver(blocks)
    assert ipm.schur_mode() == mode
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    ipm.close()
    assert res["status"] == 0, res
    assert abs(res["objective"] - ref.fun) < 1e-6 * max(1.0, abs(ref.fun)), (res, ref.fun)
