"""The host layout pass of an IPM handle's creation (csrc/ipmlayout.cpp) on the CPU: pips_ipm_layout_probe runs the functions
pips_ipm_create_qp / _general_scaled run before they touch the device.  Expected values: oracle.ipm_oracle.assemble for J and the
flat vectors, numpy for the masks, weights, maps and the flat Hessian, pa.kkt_leaf_assemble / pa.border_assemble for the leaf
systems.  Everything compared is a copy, a maximum of absolute values, a sum of 0/1 weights or a single IEEE product: np.array_equal."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import pips_ipmpp_amd as pa
from oracle.ipm_oracle import assemble
from tests.general_lp_gen import random_block_lp
from tests.qp_ref import block_hessians

LONG = 512   # CSR_LONG_ROW
VEC_X, VEC_Y, VEC_Z = ("c", "xlow", "xupp", "ixlow", "ixupp"), ("b",), ("clow", "cupp", "iclow", "icupp")


def dims_of(b, k):
    return int(b["n0"] if k == 0 else b["ni"]), int(b["mA"]), int(b["mC"])


def mat(d, rows, cols):
    if d is None:
        return sp.csr_matrix((rows, cols))
    m = sp.csr_matrix((np.asarray(d["val"], float), np.asarray(d["colidx"], int), np.asarray(d["rowptr"], int)), shape=(rows, cols))
    m.sort_indices()
    return m


def csr(m):
    m = sp.csr_matrix(m)
    m.sort_indices()
    return pa.Csr(m.shape[0], m.shape[1], m.indptr, m.indices, m.data)


def varied(seed, nb=4, n0=3, ni=6, mA=2, mC=2, mBL=2, mDL=2):
    """A random block LP whose leaves reach the arms: leaf 1 without equality rows, leaf 2 without inequality rows and without
    coupling to x0, leaf 3 (where there is one) without linking rows."""
    blocks = random_block_lp(seed, nb, n0, ni, mA, mC, mBL, mDL)
    b = blocks[1]
    b.update(mA=0, A=None, B=None, b=np.zeros(0))
    b = blocks[2]
    b.update(mC=0, C=None, D=None, A=None, **{f: np.zeros(0) for f in VEC_Z})
    if nb > 3:
        blocks[3].update(BL=None, DL=None)
    return blocks


def expect(blocks, hessians=None, rank=0, eliminate=True):
    root, N = blocks[0], len(blocks) - 1
    n0, my0, mz0 = dims_of(root, 0)
    myl, mzl = int(root["mBL"]), int(root["mDL"])
    sz = np.array([dims_of(b, k) for k, b in enumerate(blocks)][1:]).reshape(N, 3)
    e = dict(N=N, n0=n0, my0=my0, mz0=mz0, myl=myl, mzl=mzl, ry=my0 + myl, rzr=mz0 + mzl)
    e["xoff"] = np.concatenate([[0], n0 + np.concatenate([[0], np.cumsum(sz[:, 0])])]).astype(np.int32)
    e["yoff"] = np.concatenate([[0], e["ry"] + np.concatenate([[0], np.cumsum(sz[:, 1])])]).astype(np.int32)
    e["zoff"] = np.concatenate([[0], e["rzr"] + np.concatenate([[0], np.cumsum(sz[:, 2])])]).astype(np.int32)
    e["koff"] = np.concatenate([[0, 0], np.cumsum(sz.sum(axis=1))]).astype(np.int64)
    nx, my, mz = int(e["xoff"][-1]), int(e["yoff"][-1]), int(e["zoff"][-1])
    ncp = 2 * mz + 2 * nx
    e.update(nx=nx, my=my, mz=mz, ncp=ncp, nxyz=nx + my + mz, NP=nx + mz + ncp, ND=my + mz + ncp, nleaf=int(e["koff"][-1]))
    e_mz0, e_mzl = (mz0, mzl) if eliminate else (0, mz0 + mzl)
    S = n0 + my0 + myl + e_mzl
    e.update(e_mz0=e_mz0, e_mzl=e_mzl, S=S, has_q=int(hessians is not None and any(h is not None for h in hessians)))
    # J: the root's matrices on rank 0 only
    d = assemble(blocks)
    local = blocks if rank == 0 else [dict(root, A=None, BL=None, C=None, DL=None)] + list(blocks[1:])
    dl = assemble(local)
    J = sp.vstack([dl["A"], dl["C"]], format="csr")
    J.sort_indices()
    Jt = sp.csr_matrix(J.T)
    Jt.sort_indices()
    e.update(J_rp=J.indptr, J_ci=J.indices, J_v=J.data, Jt_rp=Jt.indptr, Jt_ci=Jt.indices, Jt_v=Jt.data)
    e["J_long"] = np.nonzero(np.diff(J.indptr) > LONG)[0]
    e["Jt_long"] = np.nonzero(np.diff(Jt.indptr) > LONG)[0]
    # flat vectors and masks
    M = np.concatenate([d["iclow"], d["icupp"], d["ixlow"], d["ixupp"]])
    Bd = np.concatenate([d["clow"], d["cupp"], d["xlow"], d["xupp"]]) * M
    e.update(c=d["c"], b=d["b"], M=M, Bd=Bd)
    # weights: replicated entries count on rank 0
    w = 1.0 if rank == 0 else 0.0
    wz, wx = np.ones(mz), np.ones(nx)
    wz[:mz0 + mzl] = w
    wx[:n0] = w
    wy = np.ones(my)
    wy[:my0 + myl] = w
    e["wG"] = np.concatenate([wz, wz, wx, wx])
    e["wGs"] = np.concatenate([wz, -wz, wx, -wx])
    e["wXYZ"] = np.concatenate([wx, wy, wz])
    e["pairs"] = float(np.sum(e["wG"] * M))
    # maps
    pack = list(range(n0)) + [nx + k for k in range(my0)] + [nx + my + k for k in range(e_mz0)] + [nx + my0 + k for k in range(myl)] + \
        [nx + my + e_mz0 + k for k in range(e_mzl)]
    code = []
    for i in range(1, N + 1):
        xs, ys, zs = (range(int(e[o][i]), int(e[o][i + 1])) for o in ("xoff", "yoff", "zoff"))
        pack += list(xs) + [nx + k for k in ys] + [nx + my + k for k in zs]
        code += list(xs) + [-1] * len(ys) + [-2 - k for k in zs]
    e.update(pack=np.array(pack, np.int64), code=np.array(code, np.int64))
    # Hessians: lower triangles, sorted, duplicates added up
    lows = []
    for k, b in enumerate(blocks):
        h = hessians[k] if hessians is not None else None
        lows.append(None if h is None else mat(h, dims_of(b, k)[0], dims_of(b, k)[0]))   # scipy adds duplicates up in storage order
    for m in lows:
        if m is not None:
            m.sum_duplicates()
    e["hq_have"] = np.array([m is not None for m in lows], np.int32)
    have = [m for m in lows if m is not None]
    e["hq_rp"] = np.concatenate([m.indptr for m in have]) if have else np.zeros(0)
    e["hq_ci"] = np.concatenate([m.indices for m in have]) if have else np.zeros(0)
    e["hq_v"] = np.concatenate([m.data for m in have]) if have else np.zeros(0)
    if e["has_q"]:
        full = []
        for k, (m, b) in enumerate(zip(lows, blocks)):
            n = dims_of(b, k)[0]
            full.append(sp.csr_matrix((n, n)) if m is None else m + sp.tril(m, -1).T)
        Q = sp.block_diag(full, format="csr")
        Q.sort_indices()
        diag = np.zeros(nx)
        for k, (m, b) in enumerate(zip(lows, blocks)):
            if m is not None:
                diag[int(e["xoff"][k]) if k else 0:][:m.shape[0]] = m.diagonal()
        e.update(Q_rp=Q.indptr, Q_ci=Q.indices, Q_v=Q.data, qdiag=diag, Q_long=np.nonzero(np.diff(Q.indptr) > LONG)[0])
    else:
        e.update(Q_rp=np.zeros(0), Q_ci=np.zeros(0), Q_v=np.zeros(0), qdiag=np.zeros(0), Q_long=np.zeros(0))
    # leaf systems and borders through the library's assemble functions
    leaf = {k: [] for k in ("Krp", "Kci", "kvals", "Brd", "Bci", "Bv")}
    for i in range(1, N + 1):
        b = blocks[i]
        n, myi, mzi = dims_of(b, i)
        K, _ = pa.kkt_leaf_assemble(n, csr(mat(b["B"], myi, n)), csr(mat(b["D"], mzi, n)), None if lows[i] is None else csr(lows[i]))
        G = mat(b["DL"], mzl, n)
        if not eliminate:
            G = sp.vstack([sp.csr_matrix((mz0, n)), G], format="csr")   # root inequality rows among the linking ones: no leaf part
        Br = pa.border_assemble(n, myi, mzi, n0, my0, A=csr(mat(b["A"], myi, n0)), Cm=csr(mat(b["C"], mzi, n0)), F=csr(mat(b["BL"], myl, n)), G=csr(G))
        for key, a in zip(leaf, (K.rowptr, K.colidx, K.val, Br.rowptr, Br.colidx, Br.val)):
            leaf[key].append(a)
    e.update({k: np.concatenate(v) for k, v in leaf.items()})
    # the root's matrices; not eliminated: G0' = [C0; G0]
    roots = dict(A0=mat(root["A"], my0, n0), F0=mat(root["BL"], myl, n0), C0=mat(root["C"], mz0, n0), G0=mat(root["DL"], mzl, n0))
    given = dict(A0=root["A"], F0=root["BL"], C0=root["C"], G0=root["DL"])
    if not eliminate:
        roots["G0"] = sp.vstack([roots["C0"], roots["G0"]], format="csr")
    for k, m in roots.items():
        absent = (given[k] is None or m.shape[0] == 0) and (eliminate or k != "G0")
        e.update({k + "_rp": np.zeros(0) if absent else m.indptr, k + "_ci": np.zeros(0) if absent else m.indices,
                  k + "_v": np.zeros(0) if absent else m.data})
    # the data norm sees the root's matrices on every rank, the bounds under their indicators, and the Hessians
    parts = [d["A"].data, d["C"].data, d["c"], d["b"], Bd] + [m.data for m in have]
    e["norm"] = max([float(np.abs(p).max()) for p in parts if len(p)] + [0.0])
    return e


def check(blocks, hessians=None, rank=0, n_ranks=1, eliminate=True, got=None):
    want = expect(blocks, hessians, rank, eliminate)
    if got is None:
        got = pa.ipm_layout_probe(blocks, hessians, rank=rank, n_ranks=n_ranks, eliminate_z0=eliminate)
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert got[k].shape == v.shape and np.array_equal(got[k], v), k
        else:
            assert got[k] == v, k
    return got


@pytest.mark.parametrize("eliminate", [True, False])
@pytest.mark.parametrize("seed,nb,ni,mBL,mDL", [(1, 4, 6, 2, 2), (2, 3, 4, 0, 0), (3, 3, 8, 3, 1)])
def test_lp_layout(seed, nb, ni, mBL, mDL, eliminate):
    blocks = varied(seed, nb=nb, ni=ni, mBL=mBL, mDL=mDL)
    got = check(blocks, eliminate=eliminate)
    assert got["mz0"] > 0 and (got["e_mz0"], got["e_mzl"]) == ((got["mz0"], mDL) if eliminate else (0, got["mz0"] + mDL))


@pytest.mark.parametrize("eliminate", [True, False])
def test_two_ranks(eliminate):
    blocks = varied(4, nb=4)
    parts = [[blocks[0], blocks[1], blocks[2]], [blocks[0], blocks[3]]]
    got = [check(p, rank=r, n_ranks=2, eliminate=eliminate) for r, p in enumerate(parts)]
    g0, g1 = got
    # root rows are in J on rank 0 only; on rank 1 only the leaf's part of the linking rows remains among the replicated rows
    assert g0["J_rp"][g0["my0"]] > 0 and g1["J_rp"][g1["my0"]] == 0
    z0 = g1["my"]
    assert g1["J_rp"][z0 + g1["mz0"]] == g1["J_rp"][z0]
    # weights are 0 on the replicated parts elsewhere
    assert not g1["wXYZ"][:g1["n0"]].any() and g0["wXYZ"].all() and not g1["wG"][:g1["rzr"]].any()
    # the local norm still sees the root matrices on rank 1
    big = copy.deepcopy(parts[1])
    big[0]["A"]["val"][0] = 1e6
    assert pa.ipm_layout_probe(big, rank=1, n_ranks=2, eliminate_z0=eliminate)["norm"] == 1e6


def unsorted_with_duplicate(h):
    """the same lower triangle with every row reversed and its first entry split into two halves (their sum is exact)"""
    rp, ci, v = [0], [], []
    for r in range(h["rows"]):
        c, x = h["colidx"][h["rowptr"][r]:h["rowptr"][r + 1]][::-1], h["val"][h["rowptr"][r]:h["rowptr"][r + 1]][::-1]
        if c:
            c, x = [c[0]] + list(c), [x[0] / 2] + [x[0] / 2] + list(x[1:])
        ci += c
        v += x
        rp.append(len(ci))
    return dict(rows=h["rows"], cols=h["cols"], rowptr=rp, colidx=ci, val=v)


@pytest.mark.parametrize("which", ["all", "root", "some", "none", "unsorted"])
@pytest.mark.parametrize("eliminate", [True, False])
def test_qp_layout(which, eliminate):
    blocks = varied(5, nb=4)
    hess, _ = block_hessians(5, blocks, "pd")
    if which == "root":
        hess = [hess[0], None, None, None]
    elif which == "some":
        hess = [None, hess[1], None, hess[3]]
    elif which == "none":
        hess = [None] * 4
    elif which == "unsorted":
        hess = [unsorted_with_duplicate(h) for h in hess]
    got = check(blocks, hess, eliminate=eliminate)
    assert got["has_q"] == (which != "none")
    if which == "unsorted":
        sorted_ = pa.ipm_layout_probe(blocks, block_hessians(5, blocks, "pd")[0], eliminate_z0=eliminate)
        assert all(np.array_equal(got[k], sorted_[k]) for k in ("hq_rp", "hq_ci", "hq_v", "Q_rp", "Q_ci", "Q_v", "qdiag", "kvals"))


def test_qp_rank_without_hessian_of_its_own():
    blocks = varied(6, nb=3)
    hess, _ = block_hessians(6, blocks, "pd")
    check([blocks[0], blocks[2]], [None, None], rank=1, n_ranks=2)
    check([blocks[0], blocks[2]], [hess[0], hess[2]], rank=1, n_ranks=2)


def blank(k, nb, n0, n, mA, mC, mBL, mDL):
    """a block without matrices: zero cost, x >= 0, rows 0 <= . (inequalities) and = 0"""
    z = np.zeros
    return dict(numBlocks=nb, blockID=k, n0=n0, ni=n, mA=mA, mC=mC, mBL=mBL, mDL=mDL, c=z(n), xlow=z(n), xupp=z(n), ixlow=np.ones(n), ixupp=z(n),
                b=z(mA), clow=z(mC), cupp=z(mC), iclow=np.ones(mC), icupp=z(mC), bL=z(mBL), dlow=z(mDL), dupp=z(mDL), idlow=np.ones(mDL), idupp=z(mDL),
                A=None, B=None, C=None, D=None, BL=None, DL=None)


def dense_dict(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return dict(rows=M.shape[0], cols=M.shape[1], rowptr=M.indptr.tolist(), colidx=M.indices.tolist(), val=M.data.tolist())


def test_long_rows():
    """one row of J, of J^T and of Q past CSR_LONG_ROW in an otherwise tiny problem"""
    n_long = LONG + 8
    rng = np.random.default_rng(7)
    blocks = [blank(0, 3, 3, 3, 1, 0, 0, 0), blank(1, 3, 3, n_long, 1, 0, 0, 0), blank(2, 3, 3, 4, 1, n_long, 0, 0)]
    blocks[0]["A"] = dense_dict(np.array([[1.0, 2.0, 0.0]]))
    blocks[1]["B"] = dense_dict(rng.integers(1, 5, size=(1, n_long)).astype(float))                    # a long row of J
    blocks[2]["B"] = dense_dict(np.array([[1.0, 0.0, 3.0, 0.0]]))
    D = np.zeros((n_long, 4))
    D[:, 1] = rng.integers(1, 5, size=n_long)
    blocks[2]["D"] = dense_dict(D)                                                                       # a long column of J
    Q1 = np.eye(n_long)
    Q1[-1, :] = rng.integers(1, 4, size=n_long)                                                          # a long row of Q
    hess = [None, dense_dict(np.tril(Q1)), None]
    got = check(blocks, hess)
    assert got["J_long"].tolist() == [1] and got["Jt_long"].tolist() == [3 + n_long + 1] and got["Q_long"].tolist() == [3 + n_long - 1]


@pytest.mark.parametrize("eliminate", [True, False])
def test_scaled_layout(eliminate):
    blocks = varied(8, nb=4)
    w = expect(blocks)
    rng = np.random.default_rng(8)
    col, row = rng.uniform(0.25, 4.0, w["nx"]), rng.uniform(0.25, 4.0, w["my"] + w["mz"])
    re, ri = row[:w["my"]], row[w["my"]:]
    scaled = copy.deepcopy(blocks)

    def smat(d, rf, c0):   # (a col_j) row_i, in that order
        if d is not None and d["rows"] > 0:
            rows = np.repeat(np.arange(d["rows"]), np.diff(d["rowptr"]))
            d["val"] = ((np.asarray(d["val"], float) * col[c0 + np.asarray(d["colidx"], int)]) * rf[rows]).tolist()

    for k, b in enumerate(scaled):
        n, myi, mzi = dims_of(b, k)
        x0, y0, z0 = (0, 0, 0) if k == 0 else (int(w["xoff"][k]), int(w["yoff"][k]), int(w["zoff"][k]))
        smat(b["A"], re[y0:], 0); smat(b["C"], ri[z0:], 0); smat(b["B"], re[y0:], x0); smat(b["D"], ri[z0:], x0)
        smat(b["BL"], re[w["my0"]:], x0); smat(b["DL"], ri[w["mz0"]:], x0)
        cs = col[x0:x0 + n]
        b.update(c=b["c"] * cs, xlow=b["xlow"] / cs, xupp=b["xupp"] / cs, b=b["b"] * re[y0:y0 + myi], clow=b["clow"] * ri[z0:z0 + mzi],
                 cupp=b["cupp"] * ri[z0:z0 + mzi])
    for b in scaled:
        b.update(bL=blocks[0]["bL"] * re[w["my0"]:w["ry"]], dlow=blocks[0]["dlow"] * ri[w["mz0"]:w["rzr"]], dupp=blocks[0]["dupp"] * ri[w["mz0"]:w["rzr"]])
    got = pa.ipm_layout_probe(blocks, eliminate_z0=eliminate, col=col, row=row)
    check(scaled, eliminate=eliminate, got=got)
    assert not np.array_equal(got["J_v"], w["J_v"])


def fails(match, blocks, hessians=None):
    with pytest.raises(pa.capi.PipsHipError, match=match) as ei:
        pa.ipm_layout_probe(blocks, hessians)
    assert "(code 1)" in str(ei.value)   # PIPS_ERR_ARG


def test_input_errors():
    good = varied(9, nb=3)
    b = copy.deepcopy(good)
    b[2]["mC"] = -1
    fails("pips_ipm_create_general: negative block dimension", b)
    b = copy.deepcopy(good)
    b[1]["ixupp"] = np.asarray(b[1]["ixupp"], float)
    b[1]["ixupp"][0] = 0.5
    fails("pips_ipm_create_general: bound indicators must be 0 or 1", b)
    b = copy.deepcopy(good)
    b[2]["B"] = None
    fails("pips_ipm_create_general: block 2 has equality rows but no B matrix", b)
    b = copy.deepcopy(good)
    b[1]["c"] = np.zeros(0)
    fails("pips_ipm_create_general: block 1 lacks c / bounds", b)
    b = copy.deepcopy(good)
    b[0]["xupp"] = np.zeros(0)
    fails("pips_ipm_create_general: block 0 lacks c / bounds", b)
    fails("pips_ipm_layout_probe: bad arguments", good[:1])


def test_hessian_errors():
    blocks = varied(10, nb=3)
    n = blocks[1]["ni"]
    eye = dense_dict(np.eye(n))

    def at1(h):
        return [None, h, None]

    fails(rf"pips_ipm_create_qp: Q\[1\] is {n + 1} x {n + 1} but block 1 has {n} variables", blocks, at1(dense_dict(np.eye(n + 1))))
    fails(r"pips_ipm_create_qp: Q\[1\] lacks colidx / val", blocks, at1(dict(eye, colidx=[], val=[])))
    fails(rf"pips_ipm_create_qp: Q\[1\] row 2 has column index {n} outside \[0, {n}\)", blocks,
          at1(dict(eye, colidx=[0, 1, n] + list(range(3, n)))))
    fails(r"pips_ipm_create_qp: Q\[1\] has entry \(0, 1\) above the diagonal - lower-triangular storage expected", blocks,
          at1(dict(eye, colidx=[1] + list(range(1, n)))))
    neg = np.eye(n)
    neg[1, 1] = -2.0
    fails(r"pips_ipm_create_qp: Q\[1\] has the negative diagonal entry -2 in row 1 - not positive semidefinite", blocks, at1(dense_dict(neg)))
