"""Convex QPs with a block-diagonal Hessian on the device harness (pips_ipm_create_qp): the Hessian product, long rows of Q, the solve
against the numpy restatement of tests/qp_ref.py and the optimality conditions of the original problem, the LP path untouched,
deterministic mode, the sparse root, the operator of the outer solve, argument checks, and the root entry of the KKT layer alone."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests.general_lp_gen import random_block_lp
from tests.qp_ref import block_hessians, kkt_check_qp, long_row_case, lower_dict, solve_qp

pytestmark = pytest.mark.gpu


def _random_lp(seed, free_fraction):   # the family of tests/test_native_general_gpu.py
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(2, 5))
    return random_block_lp(100 + seed, nb, int(rng.integers(4, 9)), int(rng.integers(8, 20)), int(rng.integers(2, 6)), int(rng.integers(1, 5)),
                           int(rng.integers(1, 4)), int(rng.integers(1, 4)), free_fraction=free_fraction)


@functools.lru_cache(maxsize=None)
def _case(seed, kind):
    """blocks, Hessian dicts, global Q, assembled data, the restatement's result and trace - computed once, shared, left unchanged"""
    from oracle import ipm_oracle as io
    blocks = _random_lp(seed, 0.0)
    hs, Q = block_hessians(seed, blocks, kind)
    d = io.assemble(blocks)
    trace = []
    ref = solve_qp(d, Q, max_iter=100, mutol=1e-9, artol=1e-8, trace=trace)
    return blocks, hs, Q, d, ref, trace


def _check_product(ipm, Q, seed):
    x = np.random.default_rng(seed).standard_normal(Q.shape[0])
    got, want = ipm.hessian_mult(x), Q @ x
    err = np.abs(got - want).max()
    print(f"hessian_mult: max error {err:.3e}, bar {1e-13 * np.abs(want).max():.3e}")
    assert err <= 1e-13 * np.abs(want).max()


def _check_solve(ipm, d, Q, ref, trace=None):
    """the bars the LP test holds against HiGHS and the oracle, against the restatement"""
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    f = ref["objective"]
    print(f"status {res['status']}, iterations {res['iterations']} (restatement {ref['iterations']}), objective {res['objective']!r} "
          f"(restatement {f!r}), gap {abs(res['objective'] - res['dual_objective']):.3e}")
    assert ref["status"] == 0
    assert res["status"] == 0, res
    assert abs(res["objective"] - f) < 1e-6 * max(1.0, abs(f)), (res, f)
    assert abs(res["objective"] - res["dual_objective"]) < 1e-5 * max(1.0, abs(f))
    kkt_check_qp(d, Q, ipm.iterate(), 1e-5)
    T = ipm.trace()
    assert abs(res["iterations"] - ref["iterations"]) <= 1
    assert np.array_equal(T[:, 5], T[:, 6])   # one step length
    if trace is not None:
        assert abs(len(T) - len(trace)) <= 1
        early = min(len(T), len(trace)) - 4
        for k in range(max(early, 1)):
            want = np.array(trace[k][1:8] if len(trace[k]) == 8 else list(trace[k][1:5]) + [0, 0, 0])
            scale = np.maximum(np.abs(want), [1e-12, 1e-9 * ref["dnorm"], 1.0, 1.0, 1e-3, 1e-3, 1e-3])
            assert (np.abs(T[k] - want) / scale).max() < 1e-4, (k, T[k], want)
    return res


@pytest.mark.parametrize("seed", range(4))
def test_hessian_product_against_scipy(seed):
    import pips_ipmpp_amd as pa
    blocks = random_block_lp(300 + seed, 4, 7, 30, 9, 5, 3, 2)
    hs, Q = block_hessians(seed, blocks, "pd")
    ipm = pa.GeneralIpmSolver(blocks, hessians=hs)
    _check_product(ipm, Q, seed)
    ipm.close()
    lp = pa.GeneralIpmSolver(blocks)
    assert np.array_equal(lp.hessian_mult(np.ones(Q.shape[0])), np.zeros(Q.shape[0]))
    lp.close()


def test_long_rows_of_a_dense_root_hessian():
    """n0 = 520: every row of Q0 in full storage is longer than the harness' long-row threshold (512), so the product runs through the
    pair of long-row kernels, and the root table holds off-diagonal entries; the leaves carry diagonal Hessians."""
    import pips_ipmpp_amd as pa
    from oracle import ipm_oracle as io
    blocks, hs, Q = long_row_case()
    assert np.diff(Q.indptr)[:520].min() == 520
    ipm = pa.GeneralIpmSolver(blocks, hessians=hs)
    _check_product(ipm, Q, 0)
    d = io.assemble(blocks)
    trace = []
    ref = solve_qp(d, Q, max_iter=100, mutol=1e-9, artol=1e-8, trace=trace)
    _check_solve(ipm, d, Q, ref, trace)
    ipm.close()


@pytest.mark.parametrize("kind", ["pd", "psd"])
@pytest.mark.parametrize("seed", range(8))
def test_qp_against_the_restatement_and_the_optimality_conditions(seed, kind):
    import pips_ipmpp_amd as pa
    blocks, hs, Q, d, ref, trace = _case(seed, kind)
    ipm = pa.GeneralIpmSolver(blocks, hessians=hs)
    _check_solve(ipm, d, Q, ref, trace)
    ipm.close()


def _run(pa, blocks, **kw):
    ipm = pa.GeneralIpmSolver(blocks, **kw)
    res = ipm.solve(max_iter=100, mutol=1e-9, artol=1e-8)
    out = (res, ipm.trace(), ipm.iterate())
    ipm.close()
    return out


def test_lp_path_untouched(monkeypatch):
    import pips_ipmpp_amd as pa
    monkeypatch.setenv("PIPS_HIP_DETERMINISTIC", "1")
    blocks = _random_lp(0, 0.0)
    r0, t0, i0 = _run(pa, blocks)
    r1, t1, i1 = _run(pa, blocks, hessians=[None] * len(blocks))
    assert r0["status"] == 0
    assert all(np.array_equal(r0[k], r1[k]) for k in r0), (r0, r1)
    assert np.array_equal(t0, t1)
    assert all(np.array_equal(i0[k], i1[k]) for k in i0)
    # stored zeros: a QP handle (one step length) on the same problem
    zeros = []
    for k, b in enumerate(blocks):
        n = int(b["n0"] if k == 0 else b["ni"])
        zeros.append(dict(rows=n, cols=n, rowptr=list(range(n + 1)), colidx=list(range(n)), val=[0.0] * n))
    rz, tz, _ = _run(pa, blocks, hessians=zeros)
    assert rz["status"] == 0, rz
    assert abs(rz["objective"] - r0["objective"]) <= 1e-8 * max(1.0, abs(r0["objective"]))
    assert np.array_equal(tz[:, 5], tz[:, 6])


def test_deterministic_qp_repeats_to_the_bit(monkeypatch):
    import pips_ipmpp_amd as pa
    monkeypatch.setenv("PIPS_HIP_DETERMINISTIC", "1")
    blocks, hs, Q, d, ref, trace = _case(1, "pd")
    ra, ta, ia = _run(pa, blocks, hessians=hs)
    rb, tb, ib = _run(pa, blocks, hessians=hs)
    assert ra["status"] == 0
    assert np.array_equal(ta, tb)
    assert all(np.array_equal(ia[k], ib[k]) for k in ia)


@pytest.mark.parametrize("seed", range(4))
def test_qp_with_the_sparse_root(seed, monkeypatch):
    """the root inequality rows are kept as rows of the root system there, so the path differs: no trace comparison"""
    import pips_ipmpp_amd as pa
    monkeypatch.setenv("PIPS_IPM_SPARSE_ROOT", "1")
    blocks, hs, Q, d, ref, trace = _case(seed, "pd")
    ipm = pa.GeneralIpmSolver(blocks, hessians=hs)
    _check_solve(ipm, d, Q, ref)
    ipm.close()


def test_outer_solve_runs_on_the_operator_with_q():
    import pips_ipmpp_amd as pa
    from oracle import ipm_oracle as io
    blocks = random_block_lp(77, 4, 6, 24, 8, 4, 3, 2, free_fraction=0.0)
    hs, Q = block_hessians(77, blocks, "pd")
    d = io.assemble(blocks)
    ipm = pa.GeneralIpmSolver(blocks, dual_reg=3e-2, hessians=hs)
    ipm.set_option("REGULARIZATION", 0)
    rng = np.random.default_rng(5)
    ncp = 2 * ipm.nzr + 2 * ipm.nx
    G, L = 10 ** rng.uniform(-1, 1, ncp), 10 ** rng.uniform(-1, 1, ncp)
    rhs = rng.standard_normal(ipm.nx + ipm.ny + ipm.nzr)
    sol, info = ipm.outer_solve(G, L, rhs, tol=1e-10)
    mz, nx, my = ipm.nzr, ipm.nx, ipm.ny
    M = np.concatenate([d["iclow"], d["icupp"], d["ixlow"], d["ixupp"]])
    ratio = np.where(M != 0, L / np.where(M != 0, G, 1.0), 0.0)
    dd = ratio[2 * mz:2 * mz + nx] + ratio[2 * mz + nx:]
    om = ratio[:mz] + ratio[mz:2 * mz]
    nom = np.where(om != 0, -1.0 / np.where(om != 0, om, 1.0), 0.0)
    J = sp.vstack([d["A"], d["C"]], format="csr")
    K = sp.bmat([[sp.diags(dd) + Q, J.T], [J, sp.diags(np.concatenate([np.zeros(my), nom]))]], format="csr")
    err = np.linalg.norm(K @ sol - rhs)
    print(f"outer solve: {info}, ||K sol - rhs|| = {err:.3e}, bar {1e-9 * np.linalg.norm(rhs):.3e}")
    assert io.BICG_STATUS[info["status"]] == "converged", info
    assert err <= 1e-9 * np.linalg.norm(rhs)
    ipm.close()


def test_bad_hessians_are_refused():
    import pips_ipmpp_amd as pa
    blocks = _random_lp(0, 0.0)
    n0 = int(blocks[0]["n0"])

    def with_root(h):
        return [h] + [None] * (len(blocks) - 1)

    eye = lower_dict(sp.identity(n0, format="csr"))
    upper = dict(rows=n0, cols=n0, rowptr=[0, 2] + list(range(3, n0 + 2)), colidx=[0, 1] + list(range(1, n0)), val=[1.0] * (n0 + 1))
    wrong_dim = lower_dict(sp.identity(n0 + 1, format="csr"))
    negative = dict(eye, val=[1.0] * (n0 - 1) + [-1.0])
    out_of_range = dict(eye, colidx=[-1] + list(range(1, n0)))
    for bad, message in ((upper, "above the diagonal"), (wrong_dim, "variables"), (negative, "negative diagonal"), (out_of_range, "outside")):
        with pytest.raises(pa.capi.PipsHipError, match=message):
            pa.GeneralIpmSolver(blocks, hessians=with_root(bad))
    pa.GeneralIpmSolver(blocks, hessians=with_root(eye)).close()


@pytest.mark.parametrize("sparse_root", [False, True], ids=["dense_root", "sparse_root"])
def test_root_hessian_entry_of_the_kkt_layer(sparse_root):
    """pips_hip_kkt_set_root_hessian alone: the Schur complement differs from the run without it by exactly Q0 on the x0 block
    (bar: the rounding of one addition per entry with margin)."""
    import torch
    import pips_ipmpp_amd as pa
    from tests.util import Problem, hip_lower_as_rowmajor
    prob = Problem(77, 3, 200, 100, 24, 16, 0.04)
    S, n0 = prob.S, prob.n0
    bt = pa.LeafBatch(prob.N, S)
    if sparse_root:
        bt.set_schur_mode(1)
    for b in range(prob.N):
        bt.set_block(b, prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"])
    bt.analyze(2)
    for b in range(prob.N):
        bt.set_values(b, prob.blocks[b]["K"].val)
    kkt = pa.KktSystem(bt, n0, 0, prob.myl, 0, F0=prob.F0, sparse_root=sparse_root)
    diag = torch.tensor(np.concatenate([b["diag"] for b in prob.blocks]), device="cuda")
    xd0 = torch.tensor(prob.x_diag0, device="cuda")

    def schur():
        kkt.factorize(diag, xd0)
        return kkt.schur_sparse_to_host().toarray() if sparse_root else hip_lower_as_rowmajor(kkt.schur_to_host(), S)

    base = schur()
    rng = np.random.default_rng(11)
    R = rng.standard_normal((n0, n0))
    Q0 = np.tril(R @ R.T)
    L = sp.csr_matrix(Q0)
    L.sort_indices()
    kkt.set_root_hessian(pa.Csr(n0, n0, L.indptr, L.indices, L.data))
    want = base.copy()
    want[:n0, :n0] += Q0
    got = schur()
    err = np.abs(got - want).max()
    print(f"max |SC - (SC0 + Q0)| = {err:.3e}, bar {1e-12 * np.abs(want).max():.3e}")
    assert err <= 1e-12 * np.abs(want).max()
    assert np.abs(got - base).max() >= 0.5 * np.abs(Q0).max()   # and it is really there
    # every entry given twice with half its value: added up on the host, the same matrix
    rp2 = 2 * L.indptr
    ci2 = np.concatenate([np.tile(L.indices[L.indptr[r]:L.indptr[r + 1]], 2) for r in range(n0)])
    v2 = np.concatenate([np.tile(0.5 * L.data[L.indptr[r]:L.indptr[r + 1]], 2) for r in range(n0)])
    kkt.set_root_hessian(pa.Csr(n0, n0, rp2, ci2, v2))
    assert np.abs(schur() - want).max() <= 1e-12 * np.abs(want).max()
    kkt.set_root_hessian(None)
    assert np.abs(schur() - base).max() <= 1e-12 * np.abs(base).max()
    with pytest.raises(pa.capi.PipsHipError):
        kkt.set_root_hessian(pa.Csr(n0, n0, [0, 1] + [1] * (n0 - 1), [1], [1.0]))   # above the diagonal
