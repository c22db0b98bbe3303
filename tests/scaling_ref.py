"""numpy restatement of the reference's problem scalers, written independently of the device code:
   Scaler.cpp            maxRowRatio :187-243, maxColRatio :245-275, invertAndRound :138-142 (safe_invert(1.0), no rounding:
                         PreprocessFactory::make_scaler passes bitshifting = false), applyScaling :152-184, setScalingVecsToOne
   EquilibriumScaler.C   scale :38-92
   GeometricMeanScaler.C scale :70-190 (minImpr 0.85, goodEnough 500, maxIters 10), applyGeoMean, postEquiScale :212-255
   SparseStorage.C       getRowMinVec / getRowMaxVec :1703-1773 (min over |a s| > pips_eps starting at DBL_MAX, max from 0)
   DenseVector.cpp       safe_invert :618-625, divideSome
with_sides is false (Scaler.hpp:35), so the direction with the smaller ratio goes first.  The matrix is J = [A; C] in the device
harness' row order; the row factors of J are [row_eq | row_ineq]."""
import numpy as np
import scipy.sparse as sp

EPS = 1e-13                       # pips_eps (pipsdef.h:34)
NO_ENTRY = np.finfo(np.float64).max
NONE, EQUILIBRIUM, GEOMETRIC, GEOMETRIC_EQUILIBRIUM, CURTIS_REID = 0, 1, 2, 3, 4


def _minmax(M, s):
    """per row of the CSR M: (min of |a_ij s_j| over the entries above pips_eps, max of all |a_ij s_j|)"""
    M = sp.csr_matrix(M)
    vals = np.abs(M.data * s[M.indices]) if s is not None else np.abs(M.data)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    mn, mx = np.full(M.shape[0], NO_ENTRY), np.zeros(M.shape[0])
    np.maximum.at(mx, rows, vals)
    big = vals > EPS
    np.minimum.at(mn, rows[big], vals[big])
    return mn, mx


def _ratio(mn, mx):
    """divideSome(min, min) and the maximum entry (0 for no rows)"""
    r = np.where(mn != 0.0, mx / np.where(mn != 0.0, mn, 1.0), mx)
    return float(r.max()) if r.size else 0.0


def _inv(g):
    """safe_invert(1.0)"""
    return np.where(g != 0.0, 1.0 / np.where(g != 0.0, g, 1.0), 1.0)


def scale(J, my, kind):
    """J: (my + mz) x nx, rows [equality | inequality].  Returns (col, row_eq, row_ineq, info8) with info8 as pips_ipm_get_scaling:
    applied, row / column ratio before, after, geometric passes, geometric stage kept, host reads (one per sweep pair)."""
    J = sp.csr_matrix(J)
    Jt = sp.csr_matrix(J.T)
    nr, nx = J.shape
    col, row = np.ones(nx), np.ones(nr)
    reads = 0

    def rows(c):                       # getRowMinMaxVec over A and C with the column factors
        return _minmax(J, c)

    def cols(r):                       # getColMinMaxVec over A and C with the row factors
        return _minmax(Jt, r)

    def post_equi(col, row):
        mn, mx = rows(col)
        rr = _ratio(mn, mx)
        cmn, cmx = cols(row)
        cr = _ratio(cmn, cmx)
        if cr < rr:                    # columns first
            col = _inv(cmx)
            row = _inv(rows(col)[1])
        else:
            row = _inv(mx)
            col = _inv(cols(row)[1])
        return col, row, rr, cr

    info = np.zeros(8)
    passes, kept, applied = 0, False, False
    if kind == EQUILIBRIUM:
        col, row, rr, cr = post_equi(col, row)
        reads += 1
        info[1], info[2] = rr, cr
        applied = True
    elif kind in (GEOMETRIC, GEOMETRIC_EQUILIBRIUM):
        rowratio, colratio = _ratio(*rows(None)), _ratio(*cols(None))
        reads += 1
        info[1], info[2] = rowratio, colratio
        colfirst = colratio < rowratio
        p0start, p1start = (colratio, rowratio) if colfirst else (rowratio, colratio)
        geoscale = p1start > 500.0
        if geoscale:
            p0prev, p1prev = p0start, p1start
            p0 = p1 = 0.0
            for i in range(10):
                if colfirst:
                    mn, mx = cols(row)
                    p0 = _ratio(mn, mx)
                    col = _inv(np.sqrt(mx * mn))
                    mn, mx = rows(col)
                    p1 = _ratio(mn, mx)
                    row = _inv(np.sqrt(mx * mn))
                else:
                    mn, mx = rows(col)
                    p0 = _ratio(mn, mx)
                    row = _inv(np.sqrt(mx * mn))
                    mn, mx = cols(row)
                    p1 = _ratio(mn, mx)
                    col = _inv(np.sqrt(mx * mn))
                reads += 1
                passes = i + 1
                if p0 > 0.85 * p0prev and p1 > 0.85 * p1prev:
                    break
                p0prev, p1prev = p0, p1
            geoscale = p0 <= 0.85 * p0start or p1 <= 0.85 * p1start
        kept = geoscale
        if geoscale or kind == GEOMETRIC_EQUILIBRIUM:
            if kind == GEOMETRIC_EQUILIBRIUM:
                if not geoscale:
                    col, row = np.ones(nx), np.ones(nr)
                col, row, _, _ = post_equi(col, row)
                reads += 1
            applied = True
    elif kind != NONE:
        raise ValueError(f"scaler {kind} not restated")
    info[3], info[4] = info[1], info[2]
    if not applied:
        col, row = np.ones(nx), np.ones(nr)
    else:
        S = scaled_matrix(J, col, row)
        info[3], info[4] = _ratio(*_minmax(S, None)), _ratio(*_minmax(sp.csr_matrix(S.T), None))
        reads += 1
    info[0], info[5], info[6] = float(applied), passes, float(kept)
    info[7] = reads if kind != NONE else 0
    return col, row[:my], row[my:], info


def scaled_matrix(J, col, row):
    """R J Cs entry by entry as applyScaling forms it: columnScale, then rowScale"""
    J = sp.csr_matrix(J)
    rows = np.repeat(np.arange(J.shape[0]), np.diff(J.indptr))
    S = J.copy()
    S.data = (J.data * col[J.indices]) * row[rows]
    return S


def _mat(m):
    if m is None:
        return None
    if hasattr(m, "rowptr") and not isinstance(m, dict):
        m = dict(rows=m.nrows, cols=m.ncols, rowptr=m.rowptr, colidx=m.colidx, val=m.val)
    return m


def transform_blocks(blocks, col, row_eq, row_ineq):
    """The reader's block dicts with A -> R A Cs, c -> Cs c, b / clow / cupp -> R (.), xlow / xupp -> (.) / col (applyScaling);
    the factors in the harness order (x = [x0 | blocks], rows [root | linking | blocks])."""
    root = blocks[0]
    n0, my0, mz0, myl, mzl = int(root["n0"]), int(root["mA"]), int(root["mC"]), int(root["mBL"]), int(root["mDL"])
    out = []

    def mat(m, rf, cf):
        m = _mat(m)
        if m is None or int(m["rows"]) == 0:
            return m
        rp, ci, v = np.asarray(m["rowptr"], dtype=np.int64), np.asarray(m["colidx"], dtype=np.int64), np.asarray(m["val"], dtype=np.float64)
        r = np.repeat(np.arange(int(m["rows"])), np.diff(rp))
        w = v.copy()
        w[rp[0]:rp[-1]] = (v[rp[0]:rp[-1]] * cf[ci[rp[0]:rp[-1]]]) * rf[r]
        return dict(rows=m["rows"], cols=m["cols"], rowptr=list(rp), colidx=list(ci), val=list(w))

    xo, yo, zo = n0, my0 + myl, mz0 + mzl
    for k, b in enumerate(blocks):
        nb = dict(b)
        n, ma, mc = int(b["n0"] if k == 0 else b["ni"]), int(b["mA"]), int(b["mC"])
        xi, yi, zi = (0, 0, 0) if k == 0 else (xo, yo, zo)
        cx, re, ri = col[xi:xi + n], row_eq[yi:yi + ma], row_ineq[zi:zi + mc]
        nb["A"] = mat(b["A"], re, col[:n0])
        nb["C"] = mat(b["C"], ri, col[:n0])
        if k:
            nb["B"] = mat(b["B"], re, cx)
            nb["D"] = mat(b["D"], ri, cx)
        nb["BL"] = mat(b["BL"], row_eq[my0:my0 + myl], cx)
        nb["DL"] = mat(b["DL"], row_ineq[mz0:mz0 + mzl], cx)
        nb["c"] = np.asarray(b["c"], dtype=np.float64) * cx
        nb["xlow"] = np.asarray(b["xlow"], dtype=np.float64) / cx
        nb["xupp"] = np.asarray(b["xupp"], dtype=np.float64) / cx
        nb["b"] = np.asarray(b["b"], dtype=np.float64) * re
        nb["clow"] = np.asarray(b["clow"], dtype=np.float64) * ri
        nb["cupp"] = np.asarray(b["cupp"], dtype=np.float64) * ri
        if k == 0:
            nb["bL"] = np.asarray(b["bL"], dtype=np.float64) * row_eq[my0:my0 + myl]
            nb["dlow"] = np.asarray(b["dlow"], dtype=np.float64) * row_ineq[mz0:mz0 + mzl]
            nb["dupp"] = np.asarray(b["dupp"], dtype=np.float64) * row_ineq[mz0:mz0 + mzl]
        else:
            xo, yo, zo = xo + n, yo + ma, zo + mc
        out.append(nb)
    return out


def dims(blocks):
    root = blocks[0]
    nx = int(root["n0"]) + sum(int(b["ni"]) for b in blocks[1:])
    my = int(root["mA"]) + int(root["mBL"]) + sum(int(b["mA"]) for b in blocks[1:])
    mz = int(root["mC"]) + int(root["mDL"]) + sum(int(b["mC"]) for b in blocks[1:])
    return nx, my, mz


def random_factors(blocks, seed, decades=4.0):
    """10^U(-decades, decades) factors in the harness order: one per variable and row, so x0 columns and linking rows share
    one factor across all blocks"""
    nx, my, mz = dims(blocks)
    rng = np.random.default_rng(seed)
    f = lambda n: 10.0 ** rng.uniform(-decades, decades, size=n)   # noqa: E731
    return f(nx), f(my), f(mz)
