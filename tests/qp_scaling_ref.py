"""Helpers of the QP scaling tests (no test in here): the numpy restatement of the Ruiz scaler the device harness runs
(PIPS_SCALER_RUIZ), the scaled lower-triangular Hessians Q' = Cs Q Cs as make_scaled forms them, and the
badly scaled twins of the QP family.

Ruiz equilibration of K = [Q J^T; J 0] by D = diag(col, row): `passes` simultaneous passes of d <- d / sqrt(max |row of D K D|), every
pass from the factors at its start.  The products are formed as the device forms them - |a_ij col_j| first, the row's own positive
factor afterwards (exact: rounding is monotone) - and the maxima come from scaling_ref._minmax, so the factors agree bit for bit."""
import numpy as np
import scipy.sparse as sp

from tests import scaling_ref as sr

RUIZ = 5          # PIPS_SCALER_RUIZ
RUIZ_PASSES = 10  # OSQP's default


def ruiz(J, Q=None, passes=RUIZ_PASSES, my=None):
    """J: (my + mz) x nx, rows [equality | inequality]; Q: the symmetric nx x nx Hessian (both triangles) or None.
    Returns (col, row_eq, row_ineq, info8) like scaling_ref.scale; my = None puts every row into row_eq."""
    J = sp.csr_matrix(J)
    Jt = sp.csr_matrix(J.T)
    Qm = sp.csr_matrix(Q) if Q is not None else None
    nr, nx = J.shape
    my = nr if my is None else my
    col, row = np.ones(nx), np.ones(nr)
    info = np.zeros(8)
    info[1], info[2] = sr._ratio(*sr._minmax(J, None)), sr._ratio(*sr._minmax(Jt, None))
    for _ in range(passes):
        mr = sr._minmax(J, col)[1]
        mc = sr._minmax(Jt, row)[1]
        mq = sr._minmax(Qm, col)[1] if Qm is not None else np.zeros(nx)
        rmax = mr * row
        cmax = np.maximum(mc, mq) * col
        row = np.where(rmax > 0.0, row / np.sqrt(np.where(rmax > 0.0, rmax, 1.0)), row)
        col = np.where(cmax > 0.0, col / np.sqrt(np.where(cmax > 0.0, cmax, 1.0)), col)
    S = sr.scaled_matrix(J, col, row)
    info[3], info[4] = sr._ratio(*sr._minmax(S, None)), sr._ratio(*sr._minmax(sp.csr_matrix(S.T), None))
    info[0], info[5], info[6], info[7] = 1.0, passes, 0.0, 2.0   # applied; passes; no geometric stage; the read before and the read after
    return col, row[:my], row[my:], info


def _offsets(blocks):
    off = [0, int(blocks[0]["n0"])]
    for b in blocks[1:]:
        off.append(off[-1] + int(b["ni"]))
    return off


def scale_hessians(hessians, blocks, col):
    """the lower-triangular dicts with the stored entry (r, c) of block i -> (q col[xi + r]) col[xi + c], in that order"""
    if hessians is None:
        return None
    off = _offsets(blocks)
    out = []
    for k, h in enumerate(hessians):
        if h is None:
            out.append(None)
            continue
        rp, ci, v = np.asarray(h["rowptr"], dtype=np.int64), np.asarray(h["colidx"], dtype=np.int64), np.asarray(h["val"], dtype=np.float64)
        r = np.repeat(np.arange(int(h["rows"])), np.diff(rp))
        cf = col[off[k]:off[k + 1]]
        out.append(dict(rows=h["rows"], cols=h["cols"], rowptr=rp.tolist(), colidx=ci.tolist(), val=((v * cf[r]) * cf[ci]).tolist()))
    return out


def global_hessian(hessians, blocks):
    """the symmetric matrix over x = [x0 | blocks] of the lower dicts: both triangles carry the stored value, as the harness' flat copy"""
    off = _offsets(blocks)
    mats = []
    for k, h in enumerate(hessians):
        n = off[k + 1] - off[k]
        if h is None:
            mats.append(sp.csr_matrix((n, n)))
            continue
        L = sp.csr_matrix((np.asarray(h["val"], dtype=np.float64), np.asarray(h["colidx"], dtype=np.int32), np.asarray(h["rowptr"], dtype=np.int32)),
                          shape=(n, n))
        mats.append(sp.csr_matrix(L + sp.tril(L, -1).T))
    return sp.block_diag(mats, format="csr")


# Seed offset of the twins' random factors.  The tests that compare the device with tests/qp_ref.solve_qp need twins on which that
# restatement - plain sparse LU, no refinement, no regularisation - completes after Ruiz scaling.  It does not on every draw: of the
# offsets 0..63 tried with seeds 0-7 and both Hessian kinds, nine left all 16 Ruiz-scaled twins at status 0; on the others one to five
# of the 16 stall near mu ~ 2e-9 with collapsing step lengths and end with status 4 or at the iteration limit (offset 9000, the LP
# tests': `pd` 0 and `pd` 5).  37 is the one of the nine whose iteration counts stay closest to the unscaled originals' (all within two).
# tests/test_qp_scaling_cpu.py checks this precondition on the restatement alone.
TWIN_SEED = 37


def twin(blocks, hessians, seed, decades=4.0):
    """The badly scaled twin: rows and variables multiplied by 10^U(-decades, decades), J -> R J Cs, Q -> Cs Q Cs, the vectors follow.
    Returns (blocks', hessians', (cs, rq, rn)); x = cs x', y = rq y', z = rn z' map its iterate back."""
    cs, rq, rn = sr.random_factors(blocks, TWIN_SEED + seed, decades)
    return sr.transform_blocks(blocks, cs, rq, rn), scale_hessians(hessians, blocks, cs), (cs, rq, rn)


def J_of(blocks):
    """(J = [A; C] in the harness' row order, my, the assembled data)"""
    from oracle import ipm_oracle as io
    d = io.assemble(blocks)
    return sp.csr_matrix(sp.vstack([d["A"], d["C"]])), d["A"].shape[0], d


def kkt_abs(J, Q, col, row):
    """|D K D| of K = [Q J^T; J 0], D = diag(col, row)"""
    S = abs(sr.scaled_matrix(J, col, row))
    nx = J.shape[1]
    Qs = abs(sp.diags(col) @ sp.csr_matrix(Q) @ sp.diags(col)) if Q is not None else sp.csr_matrix((nx, nx))
    return sp.bmat([[Qs, S.T], [S, None]], format="csr")
