"""Nothing leaks, as a number: every device and pinned host allocation of the library is made by the owner types of csrc/devmem.h,
which count what is live (pips_hip_device_allocs_live / _bytes_live).  Every kind of handle goes through its public life; after one
warm-up cycle (the per-device Schur scratch, workspaces and the like are allocated on first use and meant to stay) both counters must
come back to exactly the same values after every further cycle."""
import numpy as np
import pytest
import torch

import pips_ipmpp_amd as pa
from tests.util import Problem
from tests.test_kkt_gpu import build_system
from tests.test_native_general_gpu import _random_lp
from tests.test_sparse_root_gpu import TwoLinkProblem, _build as build_sparse_root_system

pytestmark = pytest.mark.gpu


def _live():
    return pa.device_allocs_live(), pa.device_bytes_live()


def _batch(prob, prob2, deterministic):
    """analyse, factor, solve; analyse again with blocks of another size, factor, destroy"""
    S = prob.S
    bt = pa.LeafBatch(prob.N, S)
    if deterministic:
        bt.set_deterministic(True)
    SC = torch.zeros(S * S, dtype=torch.float64, device="cuda")
    for p in (prob, prob2):
        for b in range(p.N):
            bt.set_block(b, p.blocks[b]["K"], p.n_i, p.blocks[b]["Bt"])
        bt.analyze(2)
        for b in range(p.N):
            bt.set_values(b, p.blocks[b]["K"].val)
        SC.zero_()
        bt.factor(SC, S)
        bt.factor(SC, S)   # (a second one: buffers made by the first factorisation are kept, not made again)
        x = torch.ones(p.N * p.n_leaf, dtype=torch.float64, device="cuda")
        bt.solve(x)
        bt.sync()
        assert bool(torch.isfinite(x).all())
    bt.close()


def _kkt(prob, sparse_root):
    bt, kkt = build_sparse_root_system(prob, True) if sparse_root else build_system(prob)
    diag = torch.tensor(np.concatenate([b["diag"] for b in prob.blocks]), device="cuda")
    xd0 = torch.tensor(prob.x_diag0, device="cuda")
    for _ in range(2):
        kkt.factorize(diag, xd0)
        b0 = torch.ones(prob.S, dtype=torch.float64, device="cuda")
        bl = torch.ones(prob.N * prob.n_leaf, dtype=torch.float64, device="cuda")
        kkt.solve_compressed(b0, bl)
        bt.sync()
        assert bool(torch.isfinite(b0).all()) and bool(torch.isfinite(bl).all())
    assert kkt.root_inertia() == (prob.n0, prob.myl, 0)
    kkt.close()
    bt.close()


def _dense_ldl(pivoting):
    n, n_primal = 200, 120
    rng = np.random.default_rng(3)
    m = n - n_primal
    H = rng.standard_normal((n_primal, n_primal))
    A = rng.standard_normal((m, n_primal))
    M = np.block([[H @ H.T + n_primal * np.eye(n_primal), A.T], [A, -1e-3 * np.eye(m)]])
    h = pa.HipDenseLdlSolver(n, n_primal)
    if pivoting:
        h.set_pivoting(1)
    h.matrixChanged(np.tril(M))
    rhs = rng.standard_normal(n)
    x = rhs.copy()
    h.solve(x)
    assert np.linalg.norm(M @ x - rhs) / np.linalg.norm(rhs) < 1e-9
    assert h.get_inertia() == (n_primal, m, 0)
    h.close()


def _leaf_handles(prob):
    """single handles with their Schur term; the host-pointer solves with 16, then 48 right-hand sides (the multi-RHS buffers grow)"""
    S = prob.S
    for b in range(prob.N):
        blk = prob.blocks[b]
        s = pa.HipLdlSolver(blk["K"], n_primal=prob.n_i)
        s.set_border(blk["Bt"])
        s.matrixChanged_with_schur_term(np.zeros((S, S)))
        for nrhs in (16, 48):
            X = np.ones((nrhs, prob.n_leaf)) * np.arange(1, nrhs + 1)[:, None]
            s.solve(X)
            assert np.isfinite(X).all()
        cs = np.zeros(prob.n_leaf, np.int32)
        cs[:20] = 1
        Xs = np.zeros((12, prob.n_leaf))
        Xs[:, :20] = 1.0
        s.solve_sparse(Xs, cs)
        assert np.isfinite(Xs).all()
        s.close()


def _handle_group(prob):
    """the handles of a rank as one batch; one of them goes away before its siblings"""
    solvers = []
    for b in range(prob.N):
        s = pa.HipLdlSolver(prob.blocks[b]["K"], n_primal=prob.n_i)
        s.set_border(prob.blocks[b]["Bt"])
        solvers.append(s)
    pa.HipLdlSolver.factor_schur_batch(solvers, np.zeros((prob.S, prob.S)))
    solvers[1].close()
    x = np.ones(prob.n_leaf)
    solvers[0].solve(x)   # (through the batch's factors)
    assert np.isfinite(x).all()
    for s in solvers:
        s.close()


def _general_ipm():
    ipm = pa.GeneralIpmSolver(_random_lp(3, 0.0), dual_reg=1e-9, scaler="geometric_equilibrium")
    assert ipm.scaling()["applied"] in (0, 1)
    ipm.solve(max_iter=5)
    ipm.close()


def _cycle():
    prob = Problem(1, 2, 400, 200, 24, 16, 0.02)
    prob2 = Problem(2, 2, 300, 150, 24, 16, 0.02)   # same Schur dimension, other blocks
    _batch(prob, prob2, deterministic=False)
    _batch(prob, prob2, deterministic=True)
    _kkt(Problem(77, 3, 200, 100, 24, 16, 0.04), sparse_root=False)
    _kkt(TwoLinkProblem(77, 6, 120, 60, 4, 3, 5.0 / 120), sparse_root=True)
    _dense_ldl(pivoting=False)
    _dense_ldl(pivoting=True)
    _leaf_handles(prob)
    _handle_group(Problem(11, 3, 500, 250, 24, 16, 0.02))
    _general_ipm()
    torch.cuda.synchronize()


def _assert_cycles_come_back():
    _cycle()   # warm-up: what is allocated on first use and meant to stay
    want = _live()
    print("live after the warm-up cycle (allocations, bytes):", want)
    for k in range(3):
        _cycle()
        got = _live()
        print(f"live after cycle {k + 1}:", got)
        assert got == want, (k, got, want)


def test_every_owner_gives_back_what_it_took():
    _assert_cycles_come_back()


def test_front_clock_buffer_goes_with_its_analysis(monkeypatch):
    """PIPS_HIP_MF_CLOCKS (read at every factorisation): the phase stamps of the fronts are analysis state like any other buffer"""
    monkeypatch.setenv("PIPS_HIP_MF_CLOCKS", "1")
    _assert_cycles_come_back()


def test_analyze_that_fails_part_way_leaves_nothing_behind():
    """A block whose pattern lacks a diagonal entry is refused in the middle of analyze(), by the host layout pass: after the previous
    analysis was released and before the first buffer of the new one exists.  Once the handle is destroyed the counters are where they were."""
    prob = Problem(1, 2, 400, 200, 24, 16, 0.02)
    _batch(prob, prob, deterministic=False)   # (warm-up)
    want = _live()
    K = prob.blocks[1]["K"]
    rp, ci = np.asarray(K.rowptr), np.asarray(K.colidx)
    row = prob.n_i // 2
    keep = np.ones(len(ci), bool)
    keep[rp[row] + np.nonzero(ci[rp[row]:rp[row + 1]] == row)[0]] = False
    assert keep.sum() == len(ci) - 1
    rp2 = rp.copy()
    rp2[row + 1:] -= 1
    bad = pa.Csr(K.nrows, K.ncols, rp2, ci[keep], np.asarray(K.val)[keep])
    bt = pa.LeafBatch(prob.N, prob.S)
    for b in range(prob.N):
        bt.set_block(b, prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"])
    bt.analyze(2)
    assert _live() != want
    bt.set_block(1, bad, prob.n_i, prob.blocks[1]["Bt"])
    with pytest.raises(pa.PipsHipError, match="no explicit diagonal entry"):
        bt.analyze(2)
    bt.close()
    assert _live() == want
