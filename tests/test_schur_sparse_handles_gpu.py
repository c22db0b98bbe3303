"""The leaf handles' Schur term added to a SPARSE Schur complement (INTEGRATION.md levels 1.5 / 1.5b for hosts with hasSparseKkt):
pips_hip_ldl_factor_schur_sparse and pips_hip_ldl_factor_schur_sparse_batch, the branch sparse_res = true of the reference's
addBiTLeftKiBiRightToResBlockedParallelSolvers.  The caller's matrix is one triangle in CSR; the device holds only the T positions the
leaves' cliques touch (csrc/schurtarget.cpp; the tables are checked without a device in tests/test_schur_target_cpu.py).

Shapes - the smallest that reach each kernel:
  random        Problem(11, 4, 700, 350, 30, 20, 0.01): dense tails, several tile columns, the tile kernels' table writes
  time_coupled  TimeCoupledProblem(5, 3, 900, 450, 10, 8, 6): multifrontal head, k_border_schur_add
  wide          a random problem with more than 128 non-empty border columns in every block: two border tile rows
Every block loses some border columns of its own (and one column is empty in all of them), so the cliques differ, share the rest, and
the pattern - their union plus extra entries - holds positions outside every clique.

  1. values: sc.data prefilled with random numbers; want = prefill + the oracle's addTermToSchurComplBlocked over the leaves read at the
     pattern's positions; max |got - want| / max |term| < 1e-9 (the bound tests/test_plugin_batch_gpu.py holds the dense entries to,
     against the same oracle); positions outside every clique keep their bits; inertia and one solve per leaf as in that file.  Single
     leaf and batch x both triangles x both Schur modes (PIPS_HIP_SCHUR_MODE; info()["schur_mode"] says which one ran).
  2. a second call with other diagonals reuses the binding and adds once more; a second array with the equal pattern works.
  3. no S^2: the Schur column ids spread by 997 (S' = 49 850, the same cliques): the live device bytes grow by less than 8 S'^2 / 100.
  4. deterministic mode: two fresh sets of handles agree to the bit, and 1. holds.
  5. errors: a missing clique entry (sc.data untouched), dense after sparse and the reverse, another pattern later.
  6. after create ... sparse calls ... close the live allocations and bytes are back where they were.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import pips_ipmpp_amd as pa
from oracle import oracle as orc
from tests.util import Problem, TimeCoupledProblem

pytestmark = pytest.mark.gpu

SPREAD = 997
_cache = {}


def _thin_borders(prob, mod):
    """block b loses the border columns s >= 4 with s % mod == b % mod, every block column 7"""
    for b, blk in enumerate(prob.blocks):
        Bt = blk["Bt"]
        rp = np.asarray(Bt.rowptr)
        keep_row = np.array([not (s == 7 or (s >= 4 and s % mod == b % mod)) for s in range(prob.S)])
        cnt = np.where(keep_row, np.diff(rp), 0)
        keep = np.repeat(keep_row, np.diff(rp))
        blk["Bt"] = pa.Csr(prob.S, Bt.ncols, np.concatenate([[0], np.cumsum(cnt)]), np.asarray(Bt.colidx)[keep], np.asarray(Bt.val)[keep])


def _make(shape):
    if shape == "random":
        prob = Problem(11, 4, 700, 350, 30, 20, 0.01)
    elif shape == "time_coupled":
        prob = TimeCoupledProblem(5, 3, 900, 450, 10, 8, 6)
    else:
        prob = Problem(13, 2, 500, 250, 110, 50, 0.02)
    _thin_borders(prob, 9)
    return prob


def _case(shape):
    """the problem, both value sets, and what the oracle says about each: the term (lower triangle, S x S) and one solve per leaf - computed once"""
    if shape not in _cache:
        prob = _make(shape)
        rng = np.random.default_rng(0)
        rhs = [rng.standard_normal(prob.n_leaf) for _ in range(prob.N)]
        vals, terms, sols = [], [], []
        for f in (1.0, 1.5):
            for blk in prob.blocks:
                blk["K"].val[blk["dpos"]] = blk["diag"] * f
            vals.append([blk["K"].val.copy() for blk in prob.blocks])
            term = np.zeros((prob.S, prob.S))
            xs = []
            for b in range(prob.N):
                leaf = prob.oracle_leaf(b)
                term = orc.add_term_to_schur_compl_blocked(term, leaf, prob.Bt_scipy(b))
                x = rhs[b].copy()
                leaf.solve(x)
                xs.append(x)
            term = np.tril(term)
            term.setflags(write=False)
            terms.append(term)
            sols.append(xs)
        cols = [np.nonzero(np.diff(np.asarray(blk["Bt"].rowptr)) > 0)[0] for blk in prob.blocks]
        _cache[shape] = dict(prob=prob, vals=vals, terms=terms, rhs=rhs, sols=sols, cols=cols)
    c = _cache[shape]
    for b, blk in enumerate(c["prob"].blocks):
        blk["K"].val[:] = c["vals"][0][b]
    return c


def _set_values(c, k):
    for b, blk in enumerate(c["prob"].blocks):
        blk["K"].val[:] = c["vals"][k][b]


def _tri(R, C, Sg, lower):
    lo, hi = np.maximum(R, C), np.minimum(R, C)
    m = sp.coo_matrix((np.ones(len(R)), (lo, hi) if lower else (hi, lo)), shape=(Sg, Sg)).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return m


def _pattern(cols, Sg, lower, seed=3, n_extra=200):
    """(sc, in_clique): one triangle of the union of the cliques on cols (global ids) plus extra entries, prefilled with random numbers"""
    rng = np.random.default_rng(seed)
    R = np.concatenate([np.repeat(bm, len(bm)) for bm in cols])
    C = np.concatenate([np.tile(bm, len(bm)) for bm in cols])
    cl = _tri(R, C, Sg, lower)
    sc = _tri(np.concatenate([R, rng.integers(0, Sg, n_extra)]), np.concatenate([C, rng.integers(0, Sg, n_extra)]), Sg, lower)
    sc.data = rng.standard_normal(sc.nnz)
    code = lambda m: np.repeat(np.arange(Sg, dtype=np.int64), np.diff(m.indptr)) * Sg + m.indices
    in_clique = np.isin(code(sc), code(cl))
    assert 0 < in_clique.sum() < sc.nnz
    return sc, in_clique


def _term_at(sc, term, ids):
    """the compact term (lower triangle, ids[k] = global id of compact column k) read at the stored positions of sc"""
    Sg = sc.shape[0]
    inv = -np.ones(Sg, np.int64)
    inv[ids] = np.arange(len(ids))
    i, j = inv[np.repeat(np.arange(Sg), np.diff(sc.indptr))], inv[sc.indices]
    ok = (i >= 0) & (j >= 0)
    return np.where(ok, term[np.maximum(i, j) * ok, np.minimum(i, j) * ok], 0.0)


def _solvers(prob, borders=None, deterministic=False):
    out = []
    for b in range(prob.N):
        s = pa.HipLdlSolver(prob.blocks[b]["K"], n_primal=prob.n_i)
        s.set_border(prob.blocks[b]["Bt"] if borders is None else borders[b])
        if deterministic:
            s.set_deterministic()
        out.append(s)
    return out


def _call(entry, solvers, sc, lower):
    if entry == "batch":
        pa.HipLdlSolver.factor_schur_sparse_batch(solvers, sc, lower=lower)
    else:
        for s in solvers:
            s.factor_schur_sparse(sc, lower=lower)


def _judge(tag, got, want, term_vals, in_clique, prefill):
    err = np.abs(got - want).max() / np.abs(term_vals).max()
    print(f"schur-sparse {tag}: max|got - want| / max|term| = {err:.3g}")
    assert err < 1e-9
    assert np.array_equal(got[~in_clique], prefill[~in_clique])            # bit for bit
    assert np.abs(got - prefill)[in_clique].max() > 1e-3 * np.abs(term_vals).max()


def _check_factors(c, k, entry, solvers, tol=1e-9):
    prob = c["prob"]
    want_inertia = [(prob.n_i, prob.my_i, 0)] * prob.N
    if entry == "batch":
        assert pa.HipLdlSolver.inertia_batch(solvers) == want_inertia
        assert solvers[1].get_inertia() == want_inertia[1]               # a bound handle answers through the batch
        sol = [r.copy() for r in c["rhs"]]
        pa.HipLdlSolver.solve_batch(solvers, sol)
    else:
        assert [s.get_inertia() for s in solvers] == want_inertia
        sol = [solvers[b].solve(c["rhs"][b].copy()) for b in range(prob.N)]
    for b in range(prob.N):
        assert np.linalg.norm(sol[b] - c["sols"][k][b]) / np.linalg.norm(c["sols"][k][b]) < tol


def _force_mode(monkeypatch, mode):
    monkeypatch.setenv("PIPS_HIP_SCHUR_MODE", str(mode))
    monkeypatch.delenv("PIPS_HIP_DETERMINISTIC", raising=False)


def _close(solvers):
    for s in solvers:
        s.close()


# ---- 1. values -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2], ids=["mode1", "mode2"])
@pytest.mark.parametrize("lower", [False, True], ids=["upper", "lower"])
@pytest.mark.parametrize("entry", ["single", "batch"])
@pytest.mark.parametrize("shape", ["random", "time_coupled", "wide"])
def test_values(shape, entry, lower, mode, monkeypatch):
    _force_mode(monkeypatch, mode)
    c = _case(shape)
    prob = c["prob"]
    if shape == "wide":
        assert min(len(bm) for bm in c["cols"]) > 128
    sc, in_clique = _pattern(c["cols"], prob.S, lower)
    prefill = sc.data.copy()
    term_vals = _term_at(sc, c["terms"][0], np.arange(prob.S))
    solvers = _solvers(prob)
    _call(entry, solvers, sc, lower)
    info = solvers[0].info()
    assert info["schur_mode"] == mode
    # T doubles on the device: the distinct clique positions of the engine's blocks
    assert info["sparse_schur_len"] == (in_clique.sum() if entry == "batch" else len(c["cols"][0]) * (len(c["cols"][0]) + 1) // 2)
    _judge(f"{shape}/{entry}/{'lower' if lower else 'upper'}/mode{mode}", sc.data, prefill + term_vals, term_vals, in_clique, prefill)
    _check_factors(c, 0, entry, solvers)
    _close(solvers)


# ---- 2. the binding is reused --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["single", "batch"])
def test_second_call_adds_once_more_and_a_second_array_works(entry, monkeypatch):
    _force_mode(monkeypatch, 1)
    c = _case("random")
    prob = c["prob"]
    sc, in_clique = _pattern(c["cols"], prob.S, False)
    prefill = sc.data.copy()
    t0, t1 = (_term_at(sc, c["terms"][k], np.arange(prob.S)) for k in (0, 1))
    assert np.abs(t1 - t0).max() > 1e-6 * np.abs(t0).max()
    solvers = _solvers(prob)
    _call(entry, solvers, sc, False)
    _set_values(c, 1)
    _call(entry, solvers, sc, False)                                      # other diagonals: the term changes and is added to what is there
    _judge(f"second/{entry}", sc.data, prefill + t0 + t1, t0 + t1, in_clique, prefill)
    _check_factors(c, 1, entry, solvers)
    live = (pa.device_allocs_live(), pa.device_bytes_live())
    sc2 = sp.csr_matrix((np.zeros(sc.nnz), sc.indices.copy(), sc.indptr.copy()), shape=sc.shape)   # another array, the equal pattern
    _call(entry, solvers, sc2, False)
    _judge(f"second-array/{entry}", sc2.data, t1, t1, in_clique, np.zeros(sc.nnz))
    assert (pa.device_allocs_live(), pa.device_bytes_live()) == live      # nothing was bound or allocated again
    _set_values(c, 0)
    _close(solvers)


# ---- 3. no S^2 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["single", "batch"])
def test_device_memory_does_not_grow_with_S_squared(entry, monkeypatch):
    _force_mode(monkeypatch, 1)
    c = _case("random")
    prob = c["prob"]
    Sg = prob.S * SPREAD
    assert Sg == 49850
    ids = np.arange(prob.S) * SPREAD
    borders = []
    for blk in prob.blocks:
        Bt = blk["Bt"]
        rp = np.zeros(Sg + 1, np.int64)
        rp[ids + 1] = np.diff(np.asarray(Bt.rowptr))
        borders.append(pa.Csr(Sg, Bt.ncols, np.cumsum(rp), Bt.colidx, Bt.val))
    sc, in_clique = _pattern([ids[bm] for bm in c["cols"]], Sg, False, n_extra=5000)
    prefill = sc.data.copy()
    term_vals = _term_at(sc, c["terms"][0], ids)                          # the dense oracle ran at the compact S
    before = pa.device_bytes_live()
    solvers = _solvers(prob, borders)
    _call(entry, solvers, sc, False)
    grown = pa.device_bytes_live() - before
    print(f"schur-sparse no-S^2/{entry}: live device bytes grew by {grown} (8 S'^2 = {8 * Sg * Sg})")
    assert grown < 8 * Sg * Sg / 100
    _judge(f"spread/{entry}", sc.data, prefill + term_vals, term_vals, in_clique, prefill)
    _check_factors(c, 0, entry, solvers)
    _close(solvers)


# ---- 4. deterministic mode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2], ids=["mode1", "mode2"])
@pytest.mark.parametrize("entry", ["single", "batch"])
@pytest.mark.parametrize("shape", ["random", "time_coupled"])
def test_deterministic_mode_repeats_to_the_bit(shape, entry, mode, monkeypatch):
    _force_mode(monkeypatch, mode)
    c = _case(shape)
    prob = c["prob"]
    runs = []
    for k in range(2):
        sc, in_clique = _pattern(c["cols"], prob.S, bool(mode == 2))
        prefill = sc.data.copy()
        if k == 1 and entry == "batch":                                   # the second set takes the mode from the environment
            monkeypatch.setenv("PIPS_HIP_DETERMINISTIC", "1")
        solvers = _solvers(prob, deterministic=not (k == 1 and entry == "batch"))
        _call(entry, solvers, sc, bool(mode == 2))
        assert solvers[0].info()["schur_mode"] == mode
        runs.append(sc.data.copy())
        if k == 0:
            term_vals = _term_at(sc, c["terms"][0], np.arange(prob.S))
            _judge(f"det/{shape}/{entry}/mode{mode}", sc.data, prefill + term_vals, term_vals, in_clique, prefill)
            _check_factors(c, 0, entry, solvers)
        _close(solvers)
    assert np.array_equal(runs[0], runs[1])


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------------------------
def _without_entry(sc, r, col):
    k = sc.indptr[r] + int(np.nonzero(sc.indices[sc.indptr[r]:sc.indptr[r + 1]] == col)[0][0])
    rp = sc.indptr.copy()
    rp[r + 1:] -= 1
    return sp.csr_matrix((np.delete(sc.data, k), np.delete(sc.indices, k), rp), shape=sc.shape)


@pytest.mark.parametrize("entry", ["single", "batch"])
def test_errors(entry, monkeypatch):
    _force_mode(monkeypatch, 1)
    c = _case("random")
    prob = c["prob"]
    sc, _ = _pattern(c["cols"], prob.S, False)
    bm = c["cols"][0]
    r, col = int(bm[2]), int(bm[5])
    # the pattern lacks a clique entry: refused before anything is written
    bad = _without_entry(sc, r, col)
    keep = bad.data.copy()
    solvers = _solvers(prob)
    with pytest.raises(pa.PipsHipError, match=rf"code 2\).*\({r}, {col}\)"):
        _call(entry, solvers, bad, False)
    assert np.array_equal(bad.data, keep)
    # ... and the handles are still free to take the whole pattern
    _call(entry, solvers, sc, False)
    # dense after sparse: one kind per handle
    dense = np.zeros((prob.S, prob.S))
    with pytest.raises(pa.PipsHipError, match=r"code 2\).*one kind per handle"):
        if entry == "batch":
            pa.HipLdlSolver.factor_schur_batch(solvers, dense)
        else:
            solvers[0].matrixChanged_with_schur_term(dense)
    assert not dense.any()
    # another pattern on a later call (an entry more in a consulted row; another triangle)
    more = sc.tolil()
    free = [k for k in range(int(bm[0]), prob.S) if sc[int(bm[0]), k] == 0 and k not in bm]
    more[int(bm[0]), free[0]] = 1.0
    more = sp.csr_matrix(more)
    more.sort_indices()
    assert more.nnz == sc.nnz + 1
    keep = more.data.copy()
    with pytest.raises(pa.PipsHipError, match=r"code 1\).*another pattern"):
        _call(entry, solvers, more, False)
    assert np.array_equal(more.data, keep)
    low = sp.csr_matrix(sc.T)
    low.sort_indices()
    with pytest.raises(pa.PipsHipError, match=r"code 1\).*another pattern"):
        _call(entry, solvers, low, True)
    # a wrong S
    big = sp.csr_matrix((sc.data, sc.indices, np.concatenate([sc.indptr, [sc.nnz]])), shape=(prob.S + 1, prob.S + 1))
    with pytest.raises(pa.PipsHipError, match=r"code 1\)"):
        _call(entry, solvers, big, False)
    _close(solvers)
    # sparse after dense
    solvers = _solvers(prob)
    if entry == "batch":
        pa.HipLdlSolver.factor_schur_batch(solvers, dense)
    else:
        solvers[0].matrixChanged_with_schur_term(dense)
    keep = sc.data.copy()
    with pytest.raises(pa.PipsHipError, match=r"code 2\).*one kind per handle"):
        _call(entry, solvers[:1] if entry == "single" else solvers, sc, False)
    assert np.array_equal(sc.data, keep)
    _close(solvers)


def test_leaf_without_border_columns_adds_nothing_and_null_array_factorises_only(monkeypatch):
    _force_mode(monkeypatch, 1)
    c = _case("random")
    prob = c["prob"]
    sc, _ = _pattern(c["cols"], prob.S, False)
    keep = sc.data.copy()
    Bt = prob.blocks[0]["Bt"]
    empty = pa.Csr(prob.S, Bt.ncols, np.zeros(prob.S + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    s = pa.HipLdlSolver(prob.blocks[0]["K"], n_primal=prob.n_i)
    s.set_border(empty)
    s.factor_schur_sparse(sc)
    assert np.array_equal(sc.data, keep) and s.info()["sparse_schur_len"] == 0
    x = s.solve(c["rhs"][0].copy())
    assert np.linalg.norm(x - c["sols"][0][0]) / np.linalg.norm(x) < 1e-9
    s.close()
    solvers = _solvers(prob)
    pa.HipLdlSolver.factor_schur_sparse_batch(solvers, None)
    _check_factors(c, 0, "batch", solvers)
    _close(solvers)


# ---- 6. nothing stays behind ---------------------------------------------------------------------------------------------------------------------
def test_live_allocations_come_back(monkeypatch):
    monkeypatch.delenv("PIPS_HIP_DETERMINISTIC", raising=False)
    c = _case("random")
    prob = c["prob"]

    def cycle():
        for mode, det in ((1, False), (2, False), (1, True)):
            monkeypatch.setenv("PIPS_HIP_SCHUR_MODE", str(mode))
            for entry in ("single", "batch"):
                sc, _ = _pattern(c["cols"], prob.S, False)
                solvers = _solvers(prob, deterministic=det)
                _call(entry, solvers, sc, False)
                _call(entry, solvers, sc, False)
                solvers[prob.N - 1].close()                               # one goes before its siblings
                x = solvers[0].solve(np.ones(prob.n_leaf))
                assert np.isfinite(x).all()
                _close(solvers)

    cycle()   # warm-up: what is allocated on first use and meant to stay
    want = (pa.device_allocs_live(), pa.device_bytes_live())
    cycle()
    assert (pa.device_allocs_live(), pa.device_bytes_live()) == want
