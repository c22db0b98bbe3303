"""The paths of the per-leaf handle layer (csrc/ldlhandle.hip.h) that the other files leave out: host-pointer solves whose right-hand sides are
all or nearly all zero (nothing solved; one column moved to the front), the row pack of solve_sparse below an eighth of the rows, a bound
handle's own solves with padded rows, and the dense single-handle Schur entry adding into a prefilled matrix through the device's shared
scratch array.  Each against the same handle's plain call (1e-12 max|want|) or the oracle (1e-9 relative), the tolerances of
test_plugin_batch_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import pips_ipmpp_amd as pa
from oracle import oracle as orc
from tests.util import Problem

pytestmark = pytest.mark.gpu

PAD, PAD_VALUE = 7, 7.5


@functools.lru_cache(maxsize=None)
def _two():
    return Problem(11, 2, 700, 350, 30, 20, 0.01)


@functools.lru_cache(maxsize=None)
def _three():
    return Problem(11, 3, 500, 250, 24, 16, 0.02)


@functools.lru_cache(maxsize=None)
def _terms():
    """per leaf of _two(): its non-empty border columns and the lower triangle of -Br^T K^-1 Br by the oracle (read-only)"""
    prob = _two()
    out = []
    for b in range(prob.N):
        Bt = prob.Bt_scipy(b)
        cols = np.nonzero(np.diff(Bt.indptr) > 0)[0]
        term = np.tril(orc.add_term_to_schur_compl_blocked(np.zeros((prob.S, prob.S)), prob.oracle_leaf(b), Bt))
        cols.setflags(write=False)
        term.setflags(write=False)
        out.append((cols, term))
    return out


def _factored_alone(prob, b=0):
    s = pa.HipLdlSolver(prob.blocks[b]["K"], n_primal=prob.n_i)
    s.matrixChanged()
    return s


def _padded(rows, n):
    """rows right-hand sides of length n, ld = n + PAD apart, zero but for the padding"""
    buf = np.full((rows, n + PAD), PAD_VALUE)
    buf[:, :n] = 0.0
    return buf


def _padding_intact(buf, n):
    return np.all(buf[:, n:] == PAD_VALUE)


def test_host_solve_with_zero_right_hand_sides():
    prob = _two()
    n = prob.n_leaf
    s = _factored_alone(prob)
    # no right-hand side at all
    none = _padded(1, n)
    s.solve(none[:0])
    assert not none[:, :n].any() and _padding_intact(none, n)
    # five, all zero: nothing is solved, nothing comes back
    X = _padded(5, n)
    s.solve(X)
    assert np.all(X[:, :n] == 0.0) and _padding_intact(X, n)
    # only row 3: the one column moves to the front of the staging buffer and comes back to its row
    rhs = np.random.default_rng(1).standard_normal(n)
    want = rhs.copy()
    s.solve(want)
    X[3, :n] = rhs
    s.solve(X)
    assert np.abs(X[3, :n] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.all(X[[0, 1, 2, 4], :n] == 0.0) and _padding_intact(X, n)
    s.close()


def test_solve_sparse_packs_the_marked_rows():
    prob = _two()
    n = prob.n_leaf
    s = _factored_alone(prob)
    cs = np.zeros(n, np.int32)
    cs[::16] = 1
    marked = np.nonzero(cs)[0]
    assert 8 * len(marked) < n                                   # below an eighth: the rows are packed on the host
    rhs = np.zeros(n)
    rhs[marked] = np.random.default_rng(2).standard_normal(len(marked))
    want = rhs.copy()
    s.solve(want)
    X = _padded(5, n)
    X[2, :n] = rhs
    s.solve_sparse(X, cs)
    assert np.abs(X[2, :n] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.all(X[[0, 1, 3, 4], :n] == 0.0) and _padding_intact(X, n)
    Z = _padded(5, n)
    s.solve_sparse(Z, cs)
    assert np.all(Z[:, :n] == 0.0) and _padding_intact(Z, n)
    s.close()


def test_bound_handle_solves_padded_rows_through_the_batch():
    prob = _three()
    n = prob.n_leaf
    solvers = []
    for b in range(prob.N):
        s = pa.HipLdlSolver(prob.blocks[b]["K"], n_primal=prob.n_i)
        s.set_border(prob.blocks[b]["Bt"])
        solvers.append(s)
    pa.HipLdlSolver.factor_schur_batch(solvers, np.zeros((prob.S, prob.S)))
    rhs = np.random.default_rng(3).standard_normal((3, n))
    want = rhs.copy()
    prob.oracle_leaf(1).solve(want)
    X = _padded(3, n)
    X[:, :n] = rhs
    solvers[1].solve(X)
    for r in range(3):
        assert np.linalg.norm(X[r, :n] - want[r]) / np.linalg.norm(want[r]) < 1e-9
    assert _padding_intact(X, n)
    Y = _padded(2, n)
    Y[:, :n] = rhs[:2]
    Yd = torch.tensor(Y, device="cuda")
    solvers[1].solve_dev(Yd, nrhs=2, ld=n + PAD)
    torch.cuda.synchronize()
    Y = Yd.cpu().numpy()
    for r in range(2):
        assert np.linalg.norm(Y[r, :n] - want[r]) / np.linalg.norm(want[r]) < 1e-9
    assert _padding_intact(Y, n)
    for s in solvers:
        s.close()


def test_dense_single_entry_adds_and_leaves_the_scratch_clean():
    """Two handles with common border columns take turns on the device's S x S scratch array: what one leaves there would show in the other's
    term."""
    prob = _two()
    S = prob.S
    terms = _terms()
    assert len(np.intersect1d(terms[0][0], terms[1][0])) > 0
    solvers = []
    for b in range(2):
        s = pa.HipLdlSolver(prob.blocks[b]["K"], n_primal=prob.n_i)
        s.set_border(prob.blocks[b]["Bt"])
        solvers.append(s)
    rng = np.random.default_rng(4)
    upper = np.triu(np.full((S, S), -123.25), 1)
    for b in (0, 1, 0):
        prefill = np.tril(rng.standard_normal((S, S))) + upper
        got = prefill.copy()
        solvers[b].matrixChanged_with_schur_term(got)
        want = terms[b][1]
        assert np.abs(np.tril(got) - np.tril(prefill) - want).max() / np.abs(want).max() < 1e-9
        assert np.array_equal(np.triu(got, 1), upper)
    for s in solvers:
        s.close()
