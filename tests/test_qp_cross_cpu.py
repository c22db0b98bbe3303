"""The host layout pass with cross Hessians R_i between x0 and the blocks (pips_ipm_layout_probe_cross), without a device: every
leaf's border carries R_i under the x0 Schur rows, the flat Hessian is the global arrow matrix and exactly symmetric, its long-row
list, the data norm, the layout scaled with given factors, rank 1 of 2, the refusals of pips_ipm_create_qp_cross, and the probe
without R against pips_ipm_layout_probe.  Everything R does not touch is held against the expectations of
tests/test_ipm_layout_cpu.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import pips_ipmpp_amd as pa
from tests import qp_cross_ref as qc
from tests import qp_scaling_ref as qs
from tests import scaling_ref as sr
from tests.test_ipm_layout_cpu import csr, dims_of, expect, mat

def expect_cross(blocks, hs, rs, rank=0, eliminate=True):
    """the expectations of the layout without R, with what R changes replaced"""
    e = expect(blocks, hs, rank, eliminate)
    root, N = blocks[0], len(blocks) - 1
    n0, my0, mz0 = dims_of(root, 0)
    myl, mzl = int(root["mBL"]), int(root["mDL"])
    e["has_q"] = 1
    # borders: R_i first, through the library's own assemble function
    leaf = {k: [] for k in ("Brd", "Bci", "Bv")}
    for i in range(1, N + 1):
        b = blocks[i]
        n, myi, mzi = dims_of(b, i)
        G = mat(b["DL"], mzl, n)
        if not eliminate:
            G = sp.vstack([sp.csr_matrix((mz0, n)), G], format="csr")
        Br = pa.border_assemble(n, myi, mzi, n0, my0, R=None if rs[i] is None else csr(mat(rs[i], n, n0)), A=csr(mat(b["A"], myi, n0)),
                                Cm=csr(mat(b["C"], mzi, n0)), F=csr(mat(b["BL"], myl, n)), G=csr(G))
        for key, a in zip(leaf, (Br.rowptr, Br.colidx, Br.val)):
            leaf[key].append(a)
    e.update({k: np.concatenate(v) for k, v in leaf.items()})
    # the flat Hessian: the global matrix; on a rank != 0 without the Q0 block, whose diagonal qdiag keeps
    Q = qc.global_hessian(hs, rs, blocks)
    qdiag = Q.diagonal()
    if rank != 0:
        Q = sp.lil_matrix(Q)
        Q[:n0, :n0] = 0
        Q = sp.csr_matrix(Q)
        Q.eliminate_zeros()
        Q.sort_indices()
    e.update(Q_rp=Q.indptr, Q_ci=Q.indices, Q_v=Q.data, qdiag=qdiag, Q_long=np.nonzero(np.diff(Q.indptr) > qc.LONG)[0])
    e["norm"] = max([e["norm"]] + [float(np.abs(r["val"]).max()) for r in rs if r is not None])
    return e


def check(blocks, hs, rs, rank=0, n_ranks=1, eliminate=True, got=None):
    want = expect_cross(blocks, hs, rs, rank, eliminate)
    if got is None:
        got = pa.ipm_layout_probe(blocks, hs, rank=rank, n_ranks=n_ranks, eliminate_z0=eliminate, cross_hessians=rs)
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert got[k].shape == v.shape and np.array_equal(got[k], v), k
        else:
            assert got[k] == v, k
    return got


def check_cross_parts(blocks, rs, got, Q):
    """what the issue names, read directly off the arrays"""
    n0, S, N = got["n0"], got["S"], got["N"]
    # every leaf's border has R_i's entries under the x0 Schur rows: row c of the border, restricted to the leaf's x rows, is column c of R_i
    pos = 0
    for i in range(1, N + 1):
        n = dims_of(blocks[i], i)[0]
        rd = got["Brd"][(i - 1) * (S + 1):i * (S + 1)]
        B = sp.csr_matrix((got["Bv"][pos:pos + rd[-1]], got["Bci"][pos:pos + rd[-1]], rd), shape=(S, int(got["koff"][i + 1] - got["koff"][i])))
        pos += rd[-1]
        want = mat(rs[i], n, n0) if rs[i] is not None else sp.csr_matrix((n, n0))
        assert (B[:n0, :n] != sp.csr_matrix(want.T)).nnz == 0, i
    F = sp.csr_matrix((got["Q_v"], got["Q_ci"], got["Q_rp"]), shape=(got["nx"], got["nx"]))
    assert (F != Q).nnz == 0 and (F != F.T).nnz == 0   # equal to the global matrix, exactly symmetric
    assert np.array_equal(got["Q_long"], np.nonzero(np.diff(Q.indptr) > qc.LONG)[0])


@pytest.mark.parametrize("eliminate", [True, False])
@pytest.mark.parametrize("kind", qc.KINDS)
def test_random_case(kind, eliminate):
    c = qc.case(3 if kind == "pd" else 4, kind)
    got = check(c["blocks"], c["hs"], c["rs"], eliminate=eliminate)
    check_cross_parts(c["blocks"], c["rs"], got, c["Q"])
    assert len(got["Q_long"]) == 0 and got["norm"] >= max(np.abs(r["val"]).max() for r in c["rs"] if r is not None)


def test_long_x0_rows():
    blocks, hs, rs, Q = qc.long_row_case()
    got = check(blocks, hs, rs)
    check_cross_parts(blocks, rs, got, Q)
    assert np.array_equal(got["Q_long"], np.arange(4))   # the x0 rows, 541 entries each
    # the data norm takes max |R|
    big = [None] + [dict(r) for r in rs[1:]]
    big[2]["val"] = list(big[2]["val"])
    big[2]["val"][7] = -1e7
    assert pa.ipm_layout_probe(blocks, hs, cross_hessians=big)["norm"] == 1e7


def test_rank_one_of_two():
    """its own blocks' R only; the flat copy leaves the Q0 block out (rank 0 contributes Q0 x0 to the summed x0 rows), qdiag keeps it"""
    c = qc.case(0, "pd")
    b1, h1, r1, mine = qc.split(c["blocks"], c["hs"], c["rs"], 1)
    assert len(mine) >= 1 and all(r is not None for r in r1[1:])
    got = check(b1, h1, r1, rank=1, n_ranks=2)
    n0 = got["n0"]
    F = sp.csr_matrix((got["Q_v"], got["Q_ci"], got["Q_rp"]), shape=(got["nx"], got["nx"]))
    assert F[:n0, :n0].nnz == 0 and F[:n0, n0:].nnz == qc.cross_entries(r1) and (F != F.T).nnz == 0
    assert np.array_equal(got["qdiag"][:n0], qc.global_hessian(h1, r1, b1).diagonal()[:n0]) and got["qdiag"][:n0].min() > 0
    # the scaled layout of that rank with given factors
    cs, rq, rn = sr.random_factors(b1, 78, 2.0)
    sb, sh, sx = sr.transform_blocks(b1, cs, rq, rn), qs.scale_hessians(h1, b1, cs), qc.scale_cross(r1, b1, cs)
    check(sb, sh, sx, rank=1, n_ranks=2,
          got=pa.ipm_layout_probe(b1, h1, rank=1, n_ranks=2, col=cs, row=np.concatenate([rq, rn]), cross_hessians=r1))
    # rank 0 keeps Q0; a rank != 0 without a cross Hessian of its own keeps it too (the harness takes it out once the ranks have agreed)
    b0, h0, r0, _ = qc.split(c["blocks"], c["hs"], c["rs"], 0)
    g0 = check(b0, h0, r0, rank=0, n_ranks=2)
    assert sp.csr_matrix((g0["Q_v"], g0["Q_ci"], g0["Q_rp"]), shape=(g0["nx"], g0["nx"]))[:n0, :n0].nnz > 0
    none = pa.ipm_layout_probe(b1, h1, rank=1, n_ranks=2, cross_hessians=[None] * len(b1))
    assert sp.csr_matrix((none["Q_v"], none["Q_ci"], none["Q_rp"]), shape=(none["nx"], none["nx"]))[:n0, :n0].nnz > 0


@pytest.mark.parametrize("which", ["pd", "psd", "long"])
def test_scaled_layout_with_given_factors(which):
    """R'_i(r, c) = (v col[xoff_i + r]) col[c]: the probe with factors equals the probe of the data scaled beforehand"""
    if which == "long":
        blocks, hs, rs, _ = qc.long_row_case()
    else:
        c = qc.case(3 if which == "pd" else 4, which)
        blocks, hs, rs = c["blocks"], c["hs"], c["rs"]
    cs, rq, rn = sr.random_factors(blocks, 77, 2.0)
    sb, sh, sx = sr.transform_blocks(blocks, cs, rq, rn), qs.scale_hessians(hs, blocks, cs), qc.scale_cross(rs, blocks, cs)
    got = pa.ipm_layout_probe(blocks, hs, col=cs, row=np.concatenate([rq, rn]), cross_hessians=rs)
    want = pa.ipm_layout_probe(sb, sh, cross_hessians=sx)
    for k in ("Q_rp", "Q_ci", "Q_v", "qdiag", "Q_long", "Brd", "Bci", "Bv", "Krp", "Kci", "kvals"):
        assert np.array_equal(got[k], want[k]), k
    assert got["norm"] == want["norm"]
    check(sb, sh, sx, got=got)
    F = sp.csr_matrix((got["Q_v"], got["Q_ci"], got["Q_rp"]), shape=(got["nx"], got["nx"]))
    assert (F != F.T).nnz == 0
    # and the order of the two multiplications matters on these factors: the other order gives other bits somewhere
    X = qc.cross_matrix(rs, blocks).tocoo()
    assert np.any((X.data * cs[X.row]) * cs[X.col] != (X.data * cs[X.col]) * cs[X.row])


def test_unsorted_rows_and_duplicates_are_added_up():
    c = qc.case(3, "pd")
    blocks, hs, rs = c["blocks"], c["hs"], c["rs"]
    messy = list(rs)
    r = rs[1]
    rp, ci, v = np.asarray(r["rowptr"]), np.asarray(r["colidx"]), np.asarray(r["val"])
    ci2 = np.concatenate([np.tile(ci[rp[k]:rp[k + 1]][::-1], 2) for k in range(r["rows"])])
    v2 = np.concatenate([np.tile(0.5 * v[rp[k]:rp[k + 1]][::-1], 2) for k in range(r["rows"])])
    messy[1] = dict(rows=r["rows"], cols=r["cols"], rowptr=(2 * rp).tolist(), colidx=ci2.tolist(), val=v2.tolist())
    a, b = pa.ipm_layout_probe(blocks, hs, cross_hessians=messy), pa.ipm_layout_probe(blocks, hs, cross_hessians=rs)
    for k in b:
        assert np.array_equal(a[k], b[k]), k


def test_probe_without_r_equals_the_old_probe():
    for blocks, hs in ((qc.case(3, "pd")["blocks"], qc.case(3, "pd")["hs"]), (qc.case(4, "psd")["blocks"], None)):
        n = qc.sizes(blocks)
        empty = [None] + [dict(rows=m, cols=n[0], rowptr=[0] * (m + 1), colidx=[], val=[]) for m in n[1:]]
        old = pa.ipm_layout_probe(blocks, hs)
        for rs in ([None] * len(blocks), empty):
            new = pa.ipm_layout_probe(blocks, hs, cross_hessians=rs)
            assert set(new) == set(old)
            for k in old:
                assert np.array_equal(new[k], old[k]), k
    # the C entry with R == NULL
    import ctypes as C
    capi = pa.capi
    blocks, hs = qc.case(3, "pd")["blocks"], qc.case(3, "pd")["hs"]
    keep, cb, cq, tail = capi._ipm_input(blocks, hs)
    dims, scal, sizes = (C.c_longlong * len(capi.IPM_LAYOUT_DIMS))(), (C.c_double * 2)(), (C.c_longlong * len(capi.IPM_LAYOUT_ARRAYS))()
    capi._check(capi.lib.pips_ipm_layout_probe_cross(C.c_int(len(blocks)), cb, cq, None, *tail, C.c_int(0), C.c_int(1), C.c_int(1), None, None, dims,
                                                     scal, sizes, None), "pips_ipm_layout_probe_cross")
    old = pa.ipm_layout_probe(blocks, hs)
    assert [int(s) for s in sizes] == [len(old[k]) for k, _ in capi.IPM_LAYOUT_ARRAYS]
    assert [int(d) for d in dims] == [old[k] for k in capi.IPM_LAYOUT_DIMS] and scal[1] == old["norm"]


def _refusals(blocks):
    n = qc.sizes(blocks)
    good = qc.general_dict(sp.random(n[1], n[0], density=0.5, random_state=np.random.RandomState(1), format="csr"))
    rest = [None] * (len(blocks) - 2)
    yield [None, dict(good, rows=n[1] + 1, rowptr=good["rowptr"] + [good["rowptr"][-1]])] + rest, "variables"       # wrong row count
    yield [None, dict(good, cols=n[0] + 1)] + rest, "variables"                                                       # wrong column count
    yield [None, dict(good, colidx=[n[0]] + good["colidx"][1:])] + rest, "outside"                                    # column index out of range
    yield [None, dict(good, colidx=[-1] + good["colidx"][1:])] + rest, "outside"
    yield [qc.general_dict(sp.identity(n[0], format="csr")), good] + rest, r"R\[0\] is present"                        # R[0] present
    yield [dict(rows=n[0], cols=n[0], rowptr=[0] * (n[0] + 1), colidx=[], val=[]), good] + rest, r"R\[0\] is present"  # even without an entry


def test_refusals_of_the_layout_pass():
    blocks = qc.case(3, "pd")["blocks"]
    for rs, message in _refusals(blocks):
        with pytest.raises(pa.capi.PipsHipError, match=message):
            pa.ipm_layout_probe(blocks, None, cross_hessians=rs)


def test_refusals_of_the_creation_entry():
    """pips_ipm_create_qp_cross checks its arguments before it touches a device, with and without a scaler"""
    blocks, hs = qc.case(3, "pd")["blocks"], qc.case(3, "pd")["hs"]
    for scaler in (None, "ruiz"):
        for rs, message in _refusals(blocks):
            with pytest.raises(pa.capi.PipsHipError, match=message):
                pa.GeneralIpmSolver(blocks, hessians=hs, cross_hessians=rs, scaler=scaler)
    with pytest.raises(pa.capi.PipsHipError, match="entries for"):
        pa.GeneralIpmSolver(blocks, cross_hessians=[None])
    with pytest.raises(pa.capi.PipsHipError, match="not supported"):
        pa.GeneralIpmSolver(blocks, cross_hessians=[None] * len(blocks), scaler="curtis_reid")


def test_a_cross_hessian_without_x0_is_refused():
    """n0 == 0: nothing to couple with.  The root block of a case emptied of its variables, R_1 with a stored entry."""
    blocks = [dict(b) for b in qc.case(3, "pd")["blocks"]]
    n = qc.sizes(blocks)
    root = blocks[0]
    root.update(n0=0, A=None, C=None, BL=None, DL=None, **{f: np.zeros(0) for f in ("c", "xlow", "xupp", "ixlow", "ixupp")})
    for b in blocks[1:]:
        b.update(A=None, C=None)
    bad = [None, dict(rows=n[1], cols=0, rowptr=[0, 1] + [1] * (n[1] - 1), colidx=[0], val=[1.0])] + [None] * (len(blocks) - 2)
    with pytest.raises(pa.capi.PipsHipError, match="n0 == 0"):
        pa.ipm_layout_probe(blocks, None, cross_hessians=bad)
    with pytest.raises(pa.capi.PipsHipError, match="n0 == 0"):
        pa.GeneralIpmSolver(blocks, cross_hessians=bad)
    ok = [None, dict(rows=n[1], cols=0, rowptr=[0] * (n[1] + 1), colidx=[], val=[])] + [None] * (len(blocks) - 2)
    assert pa.ipm_layout_probe(blocks, None, cross_hessians=ok)["has_q"] == 0


def test_the_restatement_completes_on_the_fixed_draws():
    """the precondition of the device tests, on the restatement alone (qc.case asserts status 0)"""
    for kind in qc.KINDS:
        for seed in range(8):
            c = qc.case(seed, kind)
            assert 8 <= c["ref"]["iterations"] <= 17 and np.linalg.eigvalsh(c["Q"].toarray()).min() >= -1e-14
    assert qc.long_case()["ref"]["iterations"] == 15
    for seed, kind in qc.TWINS:   # and on the Ruiz-scaled twins the device solves
        o = qc.scaled_twin_ref(seed, kind)
        assert abs(o["objective"] - qc.case(seed, kind)["ref"]["objective"]) < 1e-6 * max(1.0, abs(o["objective"]))
