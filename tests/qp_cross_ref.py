"""Helpers of the cross-Hessian tests (no test in here): arrow-shaped Hessians
        [ Q0   R_1^T ... R_N^T ]
   Q =  [ R_1  Q_1             ]      R_i : n_i x n0
        [ R_N              Q_N ]
for the random block problems of tests/general_lp_gen.py, the long-row case whose x0 rows pass the harness' long-row threshold, the
global matrix as the harness' flat copy holds it, the scaled cross Hessians as make_scaled forms them, the badly scaled twins, and
the cases shared by the tests with the result of the numpy restatement (tests/qp_ref.solve_qp), computed once."""
import functools

import numpy as np
import scipy.sparse as sp

from tests import qp_scaling_ref as qs
from tests import scaling_ref as sr
from tests.general_lp_gen import random_block_lp
from tests.qp_ref import lower_dict, solve_qp

KINDS = ["pd", "psd"]
LONG = 512   # CSR_LONG_ROW


def general_dict(R):
    """scipy matrix -> general CSR dict in the layout of the block dicts' matrices (sorted rows, no stored zeros)"""
    R = sp.csr_matrix(R)
    R.eliminate_zeros()
    R.sort_indices()
    return dict(rows=R.shape[0], cols=R.shape[1], rowptr=R.indptr.tolist(), colidx=R.indices.tolist(), val=R.data.tolist())


def random_lp(seed, free_fraction=0.0):   # the family of tests/test_qp_gpu.py (_random_lp), number for number
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(2, 5))
    return random_block_lp(100 + seed, nb, int(rng.integers(4, 9)), int(rng.integers(8, 20)), int(rng.integers(2, 6)), int(rng.integers(1, 5)),
                           int(rng.integers(1, 4)), int(rng.integers(1, 4)), free_fraction=free_fraction)


def sizes(blocks):
    return [int(b["n0"] if k == 0 else b["ni"]) for k, b in enumerate(blocks)]


def arrow_hessians(seed, blocks, kind):
    """(lower dicts [Q0, Q_1, ...] or None, general dicts [None, R_1, ...] or None, global scipy matrix).  Every leaf block i with a
    Hessian adds [V0; Vi][V0; Vi]^T on (x0, x_i): Q0 += V0 V0^T, Q_i = Vi Vi^T, R_i = Vi V0^T, with V0 (n0 x k), Vi (n_i x k),
    k = max(1, n_i // 3), density 0.4 - positive semidefinite by construction.
    "pd": every leaf block has one, and diag(U(0.1, 2)) is added over all x;
    "psd": odd-numbered blocks get no Q_i and no R_i and nothing is added to the diagonal (singular)."""
    if kind not in KINDS:
        raise ValueError(kind)
    rng = np.random.default_rng(2000 + seed)
    n = sizes(blocks)
    Q0 = sp.csr_matrix((n[0], n[0]))
    Qi, Ri = [None] * len(blocks), [None] * len(blocks)
    for i in range(1, len(blocks)):
        if kind == "psd" and i % 2 == 1:
            continue
        k = max(1, n[i] // 3)
        V0 = sp.random(n[0], k, density=0.4, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
        Vi = sp.random(n[i], k, density=0.4, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
        Q0 = Q0 + V0 @ V0.T
        Qi[i], Ri[i] = sp.csr_matrix(Vi @ Vi.T), sp.csr_matrix(Vi @ V0.T)
    Qi[0] = sp.csr_matrix(Q0)
    if kind == "pd":
        for i in range(len(blocks)):
            Qi[i] = sp.csr_matrix(Qi[i] + sp.diags(rng.uniform(0.1, 2.0, n[i])))
    hs = [None if m is None else lower_dict(sp.csr_matrix((m + m.T) * 0.5)) for m in Qi]
    rs = [None if m is None or sp.csr_matrix(m).count_nonzero() == 0 else general_dict(m) for m in Ri]
    return hs, rs, global_hessian(hs, rs, blocks)


def cross_matrix(rs, blocks):
    """the strictly block-lower part [0; R_1; ...; R_N] over x, n x n"""
    n = sizes(blocks)
    off = np.concatenate([[0], np.cumsum(n)])
    rows, cols, vals = [], [], []
    for i, r in enumerate(rs or []):
        if r is None:
            continue
        assert i > 0
        rp, ci, v = np.asarray(r["rowptr"], dtype=np.int64), np.asarray(r["colidx"], dtype=np.int64), np.asarray(r["val"], dtype=np.float64)
        rows.append(off[i] + np.repeat(np.arange(int(r["rows"])), np.diff(rp)))
        cols.append(ci)
        vals.append(v)
    if not rows:
        return sp.csr_matrix((off[-1], off[-1]))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(off[-1], off[-1]))


def global_hessian(hs, rs, blocks):
    """the symmetric matrix over x = [x0 | blocks]: the block diagonal of the lower dicts (tests/qp_scaling_ref.global_hessian) plus
    the cross part and its mirror, both from the one stored value, as the harness' flat copy"""
    D = qs.global_hessian(hs if hs is not None else [None] * len(blocks), blocks)
    X = cross_matrix(rs, blocks)
    Q = sp.csr_matrix(D + X + X.T)
    Q.sort_indices()
    return Q


def cross_entries(rs):
    return sum(len(r["val"]) for r in rs if r is not None)


def long_row_case():
    """n0 = 4 and three leaf blocks of 180 variables; Q = diag(U(1, 2) on x0, U(0.1, 2) on the blocks), R_i dense 180 x 4 with entries
    U(-1e-3, 1e-3): diagonally dominant, hence positive definite.  Every x0 row of the flat copy has 1 + 3 * 180 = 541 entries, more
    than the long-row threshold of 512; block rows have 5."""
    blocks = random_block_lp(600, 4, 4, 180, 3, 2, 2, 2, free_fraction=0.0)
    rng = np.random.default_rng(2600)
    n = sizes(blocks)
    hs = [lower_dict(sp.diags(rng.uniform(1.0, 2.0, n[0])).tocsr())] + [lower_dict(sp.diags(rng.uniform(0.1, 2.0, m)).tocsr()) for m in n[1:]]
    rs = [None] + [general_dict(rng.uniform(-1e-3, 1e-3, (m, n[0]))) for m in n[1:]]
    Q = global_hessian(hs, rs, blocks)
    assert np.diff(Q.indptr)[:n[0]].min() == 541 > LONG and np.diff(Q.indptr)[n[0]:].max() == 5
    return blocks, hs, rs, Q


def scale_cross(rs, blocks, col):
    """the general dicts with the stored entry (r, c) of block i -> (v col[xoff_i + r]) col[c], in that order (make_scaled)"""
    if rs is None:
        return None
    off = np.concatenate([[0], np.cumsum(sizes(blocks))])
    out = []
    for i, h in enumerate(rs):
        if h is None:
            out.append(None)
            continue
        rp, ci, v = np.asarray(h["rowptr"], dtype=np.int64), np.asarray(h["colidx"], dtype=np.int64), np.asarray(h["val"], dtype=np.float64)
        r = np.repeat(np.arange(int(h["rows"])), np.diff(rp))
        out.append(dict(rows=h["rows"], cols=h["cols"], rowptr=rp.tolist(), colidx=ci.tolist(), val=((v * col[off[i] + r]) * col[ci]).tolist()))
    return out


def twin(blocks, hs, rs, seed, decades=4.0):
    """tests/qp_scaling_ref.twin with the cross Hessians following: R' = Cs_i R Cs_0.  Returns (blocks', hs', rs', (cs, rq, rn))."""
    tb, th, fac = qs.twin(blocks, hs, seed, decades)
    return tb, th, scale_cross(rs, blocks, fac[0]), fac


@functools.lru_cache(maxsize=None)
def case(seed, kind):
    """A random case with the restatement's result and trace - computed once, shared, left unchanged.  The restatement must complete
    on the draws fixed here: a condition on the inputs, not on the device."""
    from oracle import ipm_oracle as io
    blocks = random_lp(seed)
    hs, rs, Q = arrow_hessians(seed, blocks, kind)
    assert cross_entries(rs) > 0
    d = io.assemble(blocks)
    trace = []
    ref = solve_qp(d, Q, max_iter=100, mutol=1e-9, artol=1e-8, trace=trace)
    assert ref["status"] == 0, (seed, kind, ref["status"])
    return dict(blocks=blocks, hs=hs, rs=rs, Q=Q, d=d, ref=ref, trace=trace)


@functools.lru_cache(maxsize=None)
def long_case():
    from oracle import ipm_oracle as io
    blocks, hs, rs, Q = long_row_case()
    d = io.assemble(blocks)
    trace = []
    ref = solve_qp(d, Q, max_iter=100, mutol=1e-9, artol=1e-8, trace=trace)
    assert ref["status"] == 0, ref["status"]
    return dict(blocks=blocks, hs=hs, rs=rs, Q=Q, d=d, ref=ref, trace=trace)


@functools.lru_cache(maxsize=None)
def twin_case(seed, kind):
    """a random case's badly scaled twin with its J, my and global Hessian"""
    c = case(seed, kind)
    tb, th, tr, fac = twin(c["blocks"], c["hs"], c["rs"], seed)
    J, my, _ = qs.J_of(tb)
    return dict(tb=tb, th=th, tr=tr, fac=fac, J=J, my=my, Qt=global_hessian(th, tr, tb))


# The twins the device solve is held against.  As for the block-diagonal family (tests/qp_scaling_ref.TWIN_SEED), the restatement - plain
# sparse LU, no refinement, no regularisation - does not complete on every Ruiz-scaled twin: of the 16 (seeds 0-7, both kinds) it ends
# with status 0 on 15 and stalls on `pd` 0 (status 4 after 31 iterations, objective off by 2.7e-5).  The four are taken from the 15: two
# per kind, among them the one with the most cross entries (`pd` 4) and one with three leaf blocks of which one carries R (`psd` 7).
# scaled_twin_ref asserts the precondition; tests/test_qp_cross_cpu.py checks it on the restatement alone.
TWINS = [(2, "pd"), (1, "psd"), (4, "pd"), (7, "psd")]


@functools.lru_cache(maxsize=None)
def scaled_twin_ref(seed, kind):
    """the restatement on the twin scaled with the restatement's Ruiz factors: must complete"""
    from oracle import ipm_oracle as io
    t = twin_case(seed, kind)
    col, re, ri, _ = qs.ruiz(t["J"], t["Qt"], my=t["my"])
    sb, sh, sx = sr.transform_blocks(t["tb"], col, re, ri), qs.scale_hessians(t["th"], t["tb"], col), scale_cross(t["tr"], t["tb"], col)
    o = solve_qp(io.assemble(sb), global_hessian(sh, sx, sb), max_iter=100, mutol=1e-9, artol=1e-8)
    assert o["status"] == 0, (seed, kind, o["status"])
    return o


def split(blocks, hs, rs, rank, world=2):
    """the arguments of rank `rank`: [root] + its own blocks (pips_map_children_to_ranks), Hessians and cross Hessians alike"""
    import pips_ipmpp_amd as pa
    mine = np.nonzero(pa.map_children_to_ranks(len(blocks) - 1, world) == rank)[0]
    pick = lambda a: [a[0]] + [a[1 + k] for k in mine]   # noqa: E731
    return pick(blocks), pick(hs), pick(rs), mine
