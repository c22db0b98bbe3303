"""The cases of tests/test_harness_kernels_judged_gpu.py and tests/test_harness_kernels_reference_cpu.py: the sparse products, the fused
reductions and the element-wise step kernels of csrc/harness.hip, reached beside a handle through pips_ipm_probe_spmv / _reduce / _step, with
their long-double references, the predicates that judge a result and host emulations of plausible defects.  Host-only, numpy only; the helpers
U, LD, SENTINEL, _ratio, _same_bits and Verdict are tests/vec_cases.py's.

A backend has spmv(), reduce() and step() with the argument lists of pa.capi.harness; HostBackend is FP64 numpy (optionally with one named
defect), the GPU module's backend calls the library.  judge(case, backend) runs one case and returns a Verdict; nothing is compared with a
device's output.  u = 2^-53 throughout.

Products (k_spmv<MODE, LPR>, k_spmv_long_part, k_spmv_long_finish; MATS, SP_CASES)
  A row's sum s of len products in ANY order is within (len - 1) u sum|v_p in_p| of the exact sum plus one rounding per product: len u sum|.|.
  The epilogue adds r roundings, each relative to a partial result no larger than sum|v_p in_p| + sum|epilogue terms|:
      |got - ref| <= (len + r) u (sum|v_p in_p| + sum|epilogue terms|),   r = EPI_ROUNDINGS[mode, e3 given] counted from spmv_epilogue:
      SP_QX s: 0; SP_RAC s - e: 1; SP_KX, SP_KYZ e0 e1 + s: 2 (+1 with e3); SP_RQ e0 - s - e1 + e2: 3 (+1); SP_RES_X, SP_RES_YZ e2 - (e0 e1 + s):
      3 (+1); a replicated row of a rank with lin != 0: +-s 0, e3 +- s (lin = 2) 1.  Contraction to FMA only removes roundings.
  A row without entries has s = +0.0 and, where the epilogue has no product that could contract with e3, the bits of the FP64 formula: compared
  exactly.  The long-double reference rounds its products and sums them sequentially (np.add.reduceat): its own error, at most
  len 2^-64 sum|v_p in_p| (2^-11 of the bound), is added to the bound - a row of one entry can come within that of u |v in|.
  out holds SENTINEL before the call and GUARD entries behind nrows: a row nobody writes fails its bound, a write behind nrows changes a guard.
  The operands a replicated row's formula does not use hold NaN there: a finite result has not read them.

Reductions (k_multi_reduce, k_multi_reduce_final; RED_CASES)
  sums      |got - ref| <= (d + r) u S as vec_cases.sum_bound.  sum_depth, from k_multi_reduce's order: a lane owns T = ceil(n / 65 536) entries
            (stride RED_GRID * 256); its unrolled trips add four entries as a two-level tree and that to the accumulator, one addition per trip
            (T // 4 of them, the first to 0.0 exact), then T % 4 single additions; the workgroup's LDS tree has 8 levels; k_multi_reduce_final
            gives each of its 256 lanes one partial (0.0 + p, exact) and adds them in 8 levels: d = 2 + T // 4 + T % 4 + 16.
            r = SUM_ROUNDINGS: a b: 1, a b w: 2, (a + p c)(b + q d): 5, with w: 6.  S = sum of the products of the absolute values of the parts,
            for the shifted dot sum (|a| + |p c|)(|b| + |q d|) |w|.  n = 0: the identity, exactly.
  extrema   fabs, fmax, fmin are exact and |a w|, |a / d|, -a / b round once, as numpy's FP64 does: bit for bit against the FP64 formula.

Step kernels (STEP_CASES): the reference repeats a kernel's statements in long double and carries, per entry written, the sum of the absolute
  values of the terms (mag) and the depth k of the expression (STEP_ROUNDINGS): |got - ref| <= k (u + 2^-64) mag, the second term for the
  reference's own roundings (a single rounding of the kernel comes within 2^-11 of u mag).  k = 0 (copies, sets, sign flips,
  k_masked_const, k_gather): the bits of the value.  dyz = -1 / om with om a sum of two quotients: 3 roundings in om, relative to
  S = sum|quotients|, pass through the reciprocal as 3 u S / om^2 = (3 S / |om|) u |1 / om|, plus the division and a second-order term: k =
  3 S / |om| + 2 on mag = |1 / om|.  Every output starts as SENTINEL with GUARD entries behind its length; what the kernel's statements do not
  write must keep its bits.

Defects (HostBackend(defect=...)): DEFECTS names them, KILLERS lists the cases that must reject each."""
import numpy as np

from tests.vec_cases import LD, SENTINEL, U, Verdict, _bits, _ratio, _same_bits

GUARD = 4
CSR_LONG_ROW = 512
LONG_PARTS = 32
RED_GRID = 256
RED_MAX = 12
RED_STRIDE = RED_GRID * 256
TRIP = 2048 * 256
SP_RQ, SP_RAC, SP_KX, SP_KYZ, SP_RES_X, SP_RES_YZ, SP_QX = range(7)
MODE_NAMES = ("rq", "rac", "kx", "kyz", "res_x", "res_yz", "qx")
X_MODES = (SP_RQ, SP_KX, SP_RES_X)          # the modes whose epilogue takes e3
R_DOT, R_ABSMAX, R_MIN_MASKED, R_STEPBOUND, R_DOT_SHIFTED = range(5)

SP_DEFECTS = ("later_trips_dropped", "second_row_dropped", "first_lpr_entries_only", "threshold_off_by_one", "last_long_part_dropped",
              "long_rows_past_256_unfinished", "replicated_full_epilogue", "e3_ignored", "lin2_as_lin1", "split_off_by_one", "pred_ignored")
RED_DEFECTS = ("tail_dropped", "last_partial_left_out", "mask_gt_zero", "stepbound_le_zero", "weight_ignored", "q_ignored",
               "neighbour_partials", "float32_sum")
STEP_DEFECTS = ("second_trip_dropped", "rows_beyond_min_dropped", "my_rows_dropped", "mask_ignored", "zero_lin_ignored",
                "upper_at_lower_offset", "dz_sign")
DEFECTS = SP_DEFECTS + RED_DEFECTS + STEP_DEFECTS


def egrid(n):
    return max(1, min(2048, (n + 255) // 256))


# =================================================================================================================================
# products
# =================================================================================================================================
# roundings of the epilogue on a row that is not replicated: [mode] -> (without e3, with e3)
EPI_ROUNDINGS = {SP_RQ: (3, 4), SP_RAC: (1, 1), SP_KX: (2, 3), SP_KYZ: (2, 2), SP_RES_X: (3, 4), SP_RES_YZ: (3, 3), SP_QX: (0, 0)}

_SHORT8 = (0, 1, 7, 8, 9, 17)            # 0, 1, LPR - 1, LPR, LPR + 1, 2 LPR + 1
_SHORT4 = (0, 1, 3, 4, 5, 9)
_EDGE = (511, 512, 513, 544)
# name -> nrows, ncols, (lo, hi) of the random row lengths, planted {row: length}
MATS = {}


def _mat(name, nrows, ncols, lo, hi, planted):
    assert name not in MATS and all(0 <= r < nrows for r in planted)
    MATS[name] = dict(nrows=nrows, ncols=ncols, lo=lo, hi=hi, planted=dict(planted))


def _spread(nrows, lengths, first=0):
    """plant `lengths` at rows spread over [first, nrows), the last of them at the last row"""
    k = len(lengths)
    rows = [first + (nrows - 1 - first) * j // max(k - 1, 1) for j in range(k)]
    assert len(set(rows)) == k, (nrows, k)
    return dict(zip(rows, lengths))


# eight lanes: the rows average at least six entries
_mat("l8-r1", 1, 40, 9, 9, {})
_mat("l8-r7", 7, 900, 0, 0, dict(enumerate(_SHORT8 + (513,))))                 # short rows below eight entries: one long row lifts the average
_mat("l8-r8", 8, 900, 0, 0, dict(enumerate((511, 512, 513, 544, 0, 1, 7, 8))))
_mat("l8-r9", 9, 900, 0, 0, dict(enumerate((0, 511, 512, 513, 544, 1, 9, 17, 7))))
_BIG8 = _SHORT8[:-1] + _EDGE + (8191, 17)          # the last row - at 65 rows the one second row, at 131 073 alone in its trip - is a short one
for _n in (63, 64, 65):
    _mat(f"l8-r{_n}", _n, 3000, 6, 12, _spread(_n, _BIG8))
for _n in (131071, 131072, 131073, 300001):
    _p = _spread(_n, _BIG8)
    if _n == 131073:
        _p[70001] = 262145          # parts of 8193 entries: 33 trips of 256 inside a part
    _mat(f"l8-r{_n}", _n, 50000, 6, 12, _p)
# four lanes: fewer than six on average
_mat("l4-r1", 1, 40, 3, 3, {})
_mat("l4-r3", 3, 40, 0, 0, {0: 0, 1: 1, 2: 5})
_mat("l4-r4", 4, 40, 0, 0, {0: 3, 1: 4, 2: 5, 3: 9})
_mat("l4-r5", 5, 40, 0, 0, {0: 0, 1: 3, 2: 4, 3: 5, 4: 9})
for _n in (262144, 262145, 600001):
    _mat(f"l4-r{_n}", _n, 50000, 1, 5, _spread(_n, _SHORT4[:-1] + _EDGE + (8191, 9)))
# counts of long rows (0: l4-r5): rows 3, 6, 9, .. long, the rest short; and every row long
for _k in (1, 255, 256, 257):
    _mat(f"long{_k}", 3 * _k + 2, 4000, 2, 9, {3 * j + 1: 513 + (37 * j) % 200 for j in range(_k)})
_mat("all-long", 40, 4000, 0, 0, {j: 513 + 31 * j for j in range(40)})
# epilogues: long rows inside both replicated ranges ([0, 3) and [10, 14)), short, empty and edge rows on either side
_mat("epi8", 70, 3000, 6, 12, {0: 0, 1: 513, 2: 7, 3: 0, 4: 9, 9: 1, 10: 8, 12: 544, 13: 0, 14: 17, 40: 511, 41: 512, 69: 600})
_mat("epi4", 300, 3000, 1, 5, {0: 0, 1: 3, 2: 9, 3: 0, 10: 4, 12: 0, 13: 5, 14: 1, 299: 0})

_mats = {}


class Mat:
    def __init__(self, name):
        sp = MATS[name]
        rng = np.random.default_rng([sp["nrows"], sp["ncols"], len(name), sum(map(ord, name))])
        n = self.nrows = sp["nrows"]
        self.ncols = sp["ncols"]
        lens = rng.integers(sp["lo"], sp["hi"] + 1, n)
        for r, ln in sp["planted"].items():
            lens[r] = ln
        self.lens = lens
        self.rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        nnz = self.nnz = int(self.rp[-1])
        self.ci = rng.integers(0, self.ncols, nnz, dtype=np.int32)
        self.v = rng.standard_normal(nnz)
        self.x = rng.standard_normal(self.ncols)
        self.e = [rng.standard_normal(n) for _ in range(4)]
        self.lanes = 0 if n == 0 else (4 if nnz < 6 * n else 8)
        self.long = np.flatnonzero(lens > CSR_LONG_ROW).astype(np.int32)
        self.pos = np.arange(nnz) - np.repeat(self.rp[:-1].astype(np.int64), lens)      # an entry's place in its row
        prod = self.v.astype(LD) * self.x[self.ci].astype(LD)
        self.s_ref, self.s_abs = self.rowsum(prod), self.rowsum(np.abs(prod))
        for a in (self.rp, self.ci, self.v, self.x, *self.e):
            a.flags.writeable = False

    def rowsum(self, t):
        out = np.zeros(self.nrows, dtype=t.dtype)
        ne = self.lens > 0
        if ne.any():
            out[ne] = np.add.reduceat(t, self.rp[:-1][ne])
        return out


def matrix(name):
    """the matrix `name` with its operands and long-double row sums; small ones are kept, of the large ones the last"""
    if name not in _mats:
        for k in [k for k in _mats if _mats[k].nnz > 300000]:
            del _mats[k]
        _mats[name] = Mat(name)
    return _mats[name]


class SpCase:
    group = "products"

    def __init__(self, cid, mat, mode, e3=False, lin=0, rng=(0, 0, 0), split=0, pred=-1, group="products"):
        self.id, self.mat, self.mode, self.e3, self.lin, self.rng, self.split, self.pred, self.group = cid, mat, mode, e3, lin, rng, split, pred, group


SP_CASES = {}


def _sp(cid, *a, **k):
    assert cid not in SP_CASES, cid
    SP_CASES[cid] = SpCase(cid, *a, **k)


for _name in MATS:
    if _name.startswith(("l8-", "l4-")):
        _g = "products_8_lanes" if _name.startswith("l8") else "products_4_lanes"
        _sp(f"{_name}-qx", _name, SP_QX, group=_g)
        _sp(f"{_name}-kyz", _name, SP_KYZ, group=_g)                                  # J's product inside K z
    elif not _name.startswith("epi"):
        _sp(f"{_name}-qx", _name, SP_QX, group="long_rows")
        _sp(f"{_name}-rac", _name, SP_RAC, split=MATS[_name]["nrows"] // 3, group="long_rows")      # J
        _sp(f"{_name}-rq", _name, SP_RQ, group="long_rows")                           # J^T
_sp("l4-r5-rq", "l4-r5", SP_RQ, group="long_rows")                                    # no long row at all
_sp("l8-r131073-kx-e3", "l8-r131073", SP_KX, e3=True, group="long_rows")              # the row of 262 145 under an epilogue
_RANGES = {"both": (3, 10, 14), "empty": (0, 5, 5), "tail": (0, 60, 70)}
for _m in ("epi8", "epi4"):
    for _mode in range(7):
        for _e3 in ((False, True) if _mode in X_MODES else (False,)):
            for _lin in (0, 1, 2):
                if _lin == 2 and _mode in X_MODES and not _e3:
                    continue        # a handle with a cross Hessian has a Hessian: lin = 2 comes with e3
                for _rn, _r in _RANGES.items():
                    if (_lin == 0 and _rn != "both") or (_rn == "tail" and _m == "epi4"):
                        continue
                    _sp(f"{_m}-{MODE_NAMES[_mode]}{'-e3' if _e3 else ''}-lin{_lin}-{_rn}", _m, _mode, e3=_e3, lin=_lin, rng=_r,
                        split=12 if _mode == SP_RAC else 0, group="epilogues")
    for _s in (0, 11, MATS[_m]["nrows"]):
        for _lin in (0, 1):
            _sp(f"{_m}-rac-split{_s}-lin{_lin}", _m, SP_RAC, lin=_lin, rng=_RANGES["both"], split=_s, group="epilogues")
    for _p in (0, 1):
        _sp(f"{_m}-res_x-e3-pred{_p}", _m, SP_RES_X, e3=True, pred=_p, group="epilogues")
        _sp(f"{_m}-kyz-pred{_p}", _m, SP_KYZ, pred=_p, group="epilogues")
_sp("long257-rq-pred0", "long257", SP_RQ, pred=0, group="long_rows")
_sp("long257-rq-pred1", "long257", SP_RQ, pred=1, group="long_rows")
_sp("l8-r300001-kyz-pred0", "l8-r300001", SP_KYZ, pred=0, group="products_8_lanes")
SP_IDS = sorted(SP_CASES, key=lambda c: (MATS[SP_CASES[c].mat]["nrows"] > 1000, SP_CASES[c].mat, c))      # a matrix's cases side by side


def sp_rep(case, nrows):
    r0e, r1b, r1e = case.rng
    r = np.arange(nrows)
    return (r < r0e) | ((r >= r1b) & (r < r1e)) if case.lin else np.zeros(nrows, dtype=bool)


def sp_operands(case):
    """e0..e3 as the probe takes them: SP_RAC's e0 / e1 cut at split; NaN where a replicated row's formula does not read"""
    M = matrix(case.mat)
    n, mode = M.nrows, case.mode
    e = [M.e[k].copy() for k in range(4)]
    rep = sp_rep(case, n)
    for k in range(3):
        e[k][rep] = np.nan
    if not (case.lin == 2 and mode in X_MODES):
        e[3][rep] = np.nan
    if mode == SP_RAC:
        e[0], e[1] = e[0][:case.split].copy(), e[1][case.split:].copy()
    if mode == SP_QX:
        return [None] * 4
    used = {SP_RQ: 3, SP_RAC: 2, SP_KX: 2, SP_KYZ: 2, SP_RES_X: 3, SP_RES_YZ: 3}[mode]
    return [e[k] if k < used else None for k in range(3)] + [e[3] if case.e3 else None]


def epilogue(T, mode, s, e, split, lin, rep):
    """spmv_epilogue in the type T for every row: (value, sum|terms|, roundings); e = [e0, e1, e2, e3] as the probe takes them"""
    n = s.size
    with np.errstate(all="ignore"):
        c = [None if a is None else a.astype(T) for a in e]
        if mode == SP_QX:
            return s.copy(), np.abs(s), np.zeros(n)
        e3 = c[3] if mode in X_MODES else None
        if mode == SP_RAC:
            sub = np.zeros(n, dtype=T)
            if split > 0:
                sub[:split] = c[0][:split]
            if split < n:
                sub[split:] = c[1][:n - split]
            full, mag = s - sub, np.abs(s) + np.abs(sub)
        elif mode == SP_RQ:
            full = (c[0] + e3 - s - c[1] + c[2]) if e3 is not None else (c[0] - s - c[1] + c[2])
            mag = np.abs(c[0]) + np.abs(s) + np.abs(c[1]) + np.abs(c[2]) + (np.abs(e3) if e3 is not None else 0)
        elif mode in (SP_KX, SP_KYZ):
            full = (c[0] * c[1] + e3 + s) if e3 is not None else (c[0] * c[1] + s if mode == SP_KX else s + c[0] * c[1])
            mag = np.abs(c[0] * c[1]) + np.abs(s) + (np.abs(e3) if e3 is not None else 0)
        else:
            inner = (c[0] * c[1] + e3 + s) if e3 is not None else (c[0] * c[1] + s if mode == SP_RES_X else s + c[0] * c[1])
            full = c[2] - inner
            mag = np.abs(c[2]) + np.abs(c[0] * c[1]) + np.abs(s) + (np.abs(e3) if e3 is not None else 0)
        k = np.full(n, float(EPI_ROUNDINGS[mode][e3 is not None]))
        if lin and rep.any():
            neg = mode in (SP_RQ, SP_RES_X, SP_RES_YZ)
            if lin == 2 and e3 is not None:
                lv = e3 + s if mode == SP_KX else (e3 - s if mode == SP_RQ else -(e3 + s))
                lm, lk = np.abs(e3) + np.abs(s), 1.0
            else:
                lv, lm, lk = (-s if neg else s), np.abs(s), 0.0
            full, mag, k = np.where(rep, lv, full), np.where(rep, lm, mag), np.where(rep, lk, k)
    return full, mag, k


def _sp_call(be, case, out, pred):
    M = matrix(case.mat)
    e = sp_operands(case)
    return be.spmv(case.mode, M.nrows, M.ncols, M.rp, M.ci, M.v, M.x, out, e0=e[0], e1=e[1], e2=e[2], e3=e[3], split=case.split, lin=case.lin,
                   r0e=case.rng[0], r1b=case.rng[1], r1e=case.rng[2], pred=pred)


def judge_sp(case, be):
    M = matrix(case.mat)
    n = M.nrows
    out = np.full(n + GUARD, SENTINEL)
    lanes, long_rows = _sp_call(be, case, out, case.pred)
    if lanes != M.lanes:
        return Verdict(False, case.group, np.inf, f"{lanes} lanes per row chosen, {M.lanes} expected (nnz {M.nnz}, {n} rows)")
    if not np.array_equal(np.asarray(long_rows), M.long):
        return Verdict(False, case.group, np.inf, f"long-row list {np.asarray(long_rows)[:8]}.. is not the rows longer than {CSR_LONG_ROW}")
    if not _same_bits(out[n:], np.full(GUARD, SENTINEL)):
        return Verdict(False, case.group, np.inf, f"a guard behind out changed: {out[n:]}")
    if case.pred == 0:
        ok = _same_bits(out, np.full(n + GUARD, SENTINEL))
        return Verdict(ok, case.group, 0.0 if ok else np.inf, "pred = 0: out must keep its bits")
    if case.pred == 1:
        plain = np.full(n + GUARD, SENTINEL)
        _sp_call(be, case, plain, -1)
        if not _same_bits(out, plain):
            return Verdict(False, case.group, np.inf, "pred = 1 differs from no predicate")
    e = sp_operands(case)
    rep = sp_rep(case, n)
    ref, mag, k = epilogue(LD, case.mode, M.s_ref, e, case.split, case.lin, rep)
    if not np.isfinite(out[:n]).all():
        bad = np.flatnonzero(~np.isfinite(out[:n]))
        return Verdict(False, case.group, np.inf, f"row {bad[0]}: {out[bad[0]]!r} (an operand a replicated row must not read?)")
    # mag counts |s| once: replace it by sum|v in|; the reference's own products and additions round to 2^-64 each
    bound = (M.lens + k) * LD(U) * (M.s_abs + mag - np.abs(M.s_ref)) + M.lens * LD(2.0) ** -64 * M.s_abs
    err = np.abs(out[:n].astype(LD) - ref)
    ratio = _ratio(err, bound)
    # rows without entries: the bits of the FP64 formula, unless e0 e1 + e3 could contract
    empty = (M.lens == 0) & ~((case.e3 and case.mode in (SP_KX, SP_RES_X)) & ~rep)
    if empty.any():
        f64 = epilogue(np.float64, case.mode, np.zeros(n), e, case.split, case.lin, rep)[0]
        if not _same_bits(out[:n][empty], f64[empty]):
            return Verdict(False, case.group, np.inf, f"an empty row differs from the exact epilogue: {out[:n][empty]} for {f64[empty]}")
    worst = int(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1), err))) if n else 0
    return Verdict(ratio <= 1.0, case.group, ratio, f"worst row {worst} (length {M.lens[worst] if n else 0}): |got - ref| / ((len + r) u sum|terms|)")


# =================================================================================================================================
# reductions
# =================================================================================================================================
SUM_ROUNDINGS = {"dot": 1, "dot_w": 2, "shifted": 5, "shifted_w": 6}
RED_N = (0, 1, 255, 256, 257, 65535, 65536, 65537, 262143, 262144, 262145, 600001)
# variant -> (kind, operand names by role, p, q)
RED_VARIANTS = {
    "dot": (R_DOT, dict(a="g1", b="g2"), 0.0, 0.0),
    "dot_w": (R_DOT, dict(a="g1", b="g2", w="w01"), 0.0, 0.0),
    "absmax": (R_ABSMAX, dict(a="g1"), 0.0, 0.0),
    "absmax_w": (R_ABSMAX, dict(a="g1", w="p2"), 0.0, 0.0),
    "absmax_d": (R_ABSMAX, dict(a="g1", d="p1"), 0.0, 0.0),
    "min_masked": (R_MIN_MASKED, dict(a="g3", c="mask"), 0.0, 0.0),
    "stepbound": (R_STEPBOUND, dict(a="p1", b="g2"), 0.0, 0.0),
    "shifted": (R_DOT_SHIFTED, dict(a="p1", b="p2", c="g1", d="g2"), 0.3, 0.7),
    "shifted_w": (R_DOT_SHIFTED, dict(a="p1", b="p2", c="g1", d="g2", w="w01"), 0.3, 0.7),
    "dot_onesigned": (R_DOT, dict(a="p1", b="p2"), 0.0, 0.0),                 # no cancellation: S is the sum, the bound is tight
}
_vecs = {}
_VNAMES = ("g1", "g2", "g3", "p1", "p2", "w01", "mask")


def vec(n, name):
    if (n, name) not in _vecs:
        rng = np.random.default_rng([n, 77, _VNAMES.index(name)])
        if name[0] == "g":
            v = rng.standard_normal(n)
        elif name[0] == "p":
            v = rng.random(n) + 0.05
        elif name == "w01":
            v = (rng.random(n) < 0.7).astype(np.float64)                      # the weights that count replicated entries once
        else:
            v = np.array([0.0, -0.0, 1.0, -1.0, 1e-300, 2.0])[rng.integers(0, 6, n)]
        v.flags.writeable = False
        _vecs[n, name] = v
    return _vecs[n, name]


class Term:
    def __init__(self, variant, n, patches=None):
        self.variant, self.n, self.patches = variant, n, patches or {}
        self.kind, self.roles, self.p, self.q = RED_VARIANTS[variant]

    def opds(self):
        o = {}
        for role, name in self.roles.items():
            v = vec(self.n, name)
            if role in self.patches:
                v = v.copy()
                for i, val in self.patches[role]:
                    v[i] = val
            o[role] = v
        return o

    def spec(self):
        return dict(kind=self.kind, n=self.n, p=self.p, q=self.q, **self.opds())


class RedCase:
    group = "reductions"

    def __init__(self, cid, terms, pred=-1, expect=None):
        self.id, self.terms, self.pred, self.expect = cid, terms, pred, expect


RED_CASES = {}


def _red(cid, terms, **k):
    assert cid not in RED_CASES and 1 <= len(terms) <= RED_MAX, cid
    RED_CASES[cid] = RedCase(cid, terms, **k)


for _n in RED_N:
    for _v in RED_VARIANTS:
        _red(f"{_v}-n{_n}", [Term(_v, _n)])
_NR = 600001
_MIX = ("dot", "absmax_d", "min_masked", "shifted_w", "stepbound", "dot_w", "absmax", "shifted", "absmax_w", "dot_onesigned", "dot", "min_masked")
_MIXN = (600001, 0, 257, 65537, 600001, 0, 262145, 1, 65536, 600001, 255, 0)
_red("pack12-mixed", [Term(v, n) for v, n in zip(_MIX, _MIXN)])
_red("pack12-mixed-reversed", [Term(v, n) for v, n in zip(_MIX[::-1], _MIXN[::-1])])          # the same terms at the other positions
_red("pack12-mixed-pred1", [Term(v, n) for v, n in zip(_MIX, _MIXN)], pred=1)
_red("pack12-mixed-pred0", [Term(v, n) for v, n in zip(_MIX, _MIXN)], pred=0)
_red("pack1-pred0", [Term("dot", 257)], pred=0)
for _k in (0, 5, 11):       # one term among eleven others of another length
    _red(f"pack12-dot-at{_k}", [Term("dot", 65537) if j == _k else Term("absmax", 257) for j in range(12)])
# planted extrema: first and last lane of the first workgroup, the second one, the last entry of the first sweep of the grid, the next one,
# inside the unrolled zone (second and fifth entry of a lane), the last entry (the tail loop)
PLANTED = (0, 255, 256, 65535, 65536, 3 * RED_STRIDE + 77, 5 * RED_STRIDE + 3, _NR - 1)
for _i in PLANTED:
    _red(f"planted-at{_i}", [Term("absmax", _NR, dict(a=[(_i, -60.0)])), Term("absmax_w", _NR, dict(a=[(_i, 50.0)], w=[(_i, -2.0)])),
                             Term("absmax_d", _NR, dict(a=[(_i, -3.0)], d=[(_i, 1e-3)])), Term("min_masked", _NR, dict(a=[(_i, -50.0)], c=[(_i, -1.0)])),
                             Term("stepbound", _NR, dict(a=[(_i, 1e-6)], b=[(_i, -4.0)]))], expect=(60.0, 100.0, 3000.0, -50.0, 2.5e-7))
_Q = 400000     # the runner-up
_red("min_masked-tiny-on", [Term("min_masked", _NR, dict(a=[(256, -50.0)], c=[(256, 1e-300)]))], expect=(-50.0,))
_red("min_masked-minus-one-on", [Term("min_masked", _NR, dict(a=[(_NR - 1, -50.0)], c=[(_NR - 1, -1.0)]))], expect=(-50.0,))
_red("min_masked-planted-off", [Term("min_masked", _NR, dict(a=[(256, -50.0), (_Q, -40.0)], c=[(256, -0.0), (_Q, -1.0)]))], expect=(-40.0,))
_red("min_masked-planted-off-plus-zero", [Term("min_masked", _NR, dict(a=[(65536, -50.0), (_Q, -40.0)], c=[(65536, 0.0), (_Q, 1e-300)]))], expect=(-40.0,))
_ALL = list(range(1000))
_red("min_masked-all-off", [Term("min_masked", 1000, dict(c=[(i, -0.0 if i % 2 else 0.0) for i in _ALL]))], expect=(np.inf,))
# step bounds: b in {-0.0, 0.0, positive} beside a = 0 - a 0 / 0 must not enter; b = 0.0 beside a > 0 is no bound either
_red("stepbound-zero-b", [Term("stepbound", _NR, dict(a=[(7, 0.0), (300, 0.0), (70000, 0.0), (_Q, 3.0), (9, 1e-6)],
                                                     b=[(7, -0.0), (300, 0.0), (70000, 2.0), (_Q, 0.0), (9, -4.0)]))], expect=(2.5e-7,))
_red("stepbound-no-negative-b", [Term("stepbound", 1000, dict(a=[(i, 0.0 if i % 3 == 0 else 1.0) for i in _ALL],
                                                               b=[(i, (-0.0, 0.0, 2.5)[i % 3]) for i in _ALL]))], expect=(np.inf,))
_red("stepbound-a-zero-blocks", [Term("stepbound", _NR, dict(a=[(_NR - 2, 0.0)], b=[(_NR - 2, -1.0)]))], expect=(0.0,))
# the weight and q must matter
_red("shifted-q", [Term("shifted", 65537)])
RED_IDS = sorted(RED_CASES, key=lambda c: (max(t.n for t in RED_CASES[c].terms), c))


def sum_depth(n):
    """d: the additions an entry passes through in k_multi_reduce and k_multi_reduce_final (module docstring)"""
    T = -(-n // RED_STRIDE)
    return 2 + T // 4 + T % 4 + 16


def red_terms(T, kind, p, q, o, defect=None):
    """the entries of a term in the type T, and the products of the absolute values of their parts"""
    g = lambda r: None if o.get(r) is None else o[r].astype(T)     # noqa: E731
    a, b, c, d, w = (g(r) for r in "abcdw")
    if defect == "weight_ignored":
        w = None
    with np.errstate(all="ignore"):
        if kind == R_DOT:
            v, s = a * b, np.abs(a) * np.abs(b)
            return (v * w, s * np.abs(w)) if w is not None else (v, s)
        if kind == R_ABSMAX:
            v = np.abs(a * w) if w is not None else (np.abs(a / d) if d is not None else np.abs(a))
            return v, v
        if kind == R_MIN_MASKED:
            v = np.where(o["c"] > 0.0 if defect == "mask_gt_zero" else o["c"] != 0.0, a, np.inf)
            return v, v
        if kind == R_STEPBOUND:
            neg = o["b"] <= 0.0 if defect == "stepbound_le_zero" else o["b"] < 0.0
            v = np.where(neg, -a / np.where(neg, b, 1), np.inf)
            return v, v
        p, q = T(p), T(0.0 if defect == "q_ignored" else q)
        v = (a + p * c) * (b + q * d)
        s = (np.abs(a) + np.abs(p * c)) * (np.abs(b) + np.abs(q * d))
        return (v * w, s * np.abs(w)) if w is not None else (v, s)


def red_identity(kind):
    return np.inf if kind in (R_MIN_MASKED, R_STEPBOUND) else 0.0


def _is_sum(kind):
    return kind in (R_DOT, R_DOT_SHIFTED)


def judge_red(case, be, depth=None):
    nt = len(case.terms)
    out = np.full(nt, SENTINEL)
    be.reduce([t.spec() for t in case.terms], out, pred=case.pred)
    if case.pred == 0:
        ok = _same_bits(out, np.full(nt, SENTINEL))
        return Verdict(ok, "reductions", 0.0 if ok else np.inf, "pred = 0: out must keep its bits")
    if case.pred == 1:
        plain = np.full(nt, SENTINEL)
        be.reduce([t.spec() for t in case.terms], plain, pred=-1)
        if not _same_bits(out, plain):
            return Verdict(False, "reductions", np.inf, "pred = 1 differs from no predicate")
    worst, why = 0.0, ""
    for k, t in enumerate(case.terms):
        got = out[k]
        if t.n == 0:
            if not _same_bits(got, red_identity(t.kind)):
                return Verdict(False, "reductions", np.inf, f"term {k} ({t.variant}, n = 0): {got!r} for the identity")
            continue
        if _is_sum(t.kind):
            v, s = red_terms(LD, t.kind, t.p, t.q, t.opds())
            d = sum_depth(t.n) if depth is None else depth
            r = _ratio(abs(LD(got) - v.sum()), (d + SUM_ROUNDINGS.get(t.variant, 1)) * LD(U) * s.sum()) if np.isfinite(got) else np.inf
            if r > worst:
                worst, why = r, f"term {k} ({t.variant}, n {t.n}): got {got!r}, ref {float(v.sum())!r}"
            if r > 1.0:
                return Verdict(False, "reductions", r, why)
        else:
            v = red_terms(np.float64, t.kind, t.p, t.q, t.opds())[0]
            want = np.fmax.reduce(v) if t.kind == R_ABSMAX else np.fmin.reduce(v)
            if case.expect is not None and want != case.expect[k]:
                return Verdict(False, "reductions", np.inf, f"the table plants {case.expect[k]!r} but the FP64 formula gives {want!r}")
            if not _same_bits(got, want):
                return Verdict(False, "reductions", np.inf, f"term {k} ({t.variant}, n {t.n}): got {got!r}, want {want!r}")
    return Verdict(True, "reductions", worst, why)


# =================================================================================================================================
# step kernels
# =================================================================================================================================
STEP_DIMS = ((1, 0, 0), (5, 3, 0), (3, 5, 2), (2, 1, 7), (300, 100, 200), (524289, 10, 17), (10, 524289, 17), (10, 17, 524289))
STEP_KERNELS = ("bound_residuals", "diagonals", "leaf_diag", "reg_operator", "rhs_reduce", "recover", "compl_rhs", "masked_const", "gather")
# the depth of the deepest expression a kernel writes, in roundings (module docstring; per output in step_formula)
STEP_ROUNDINGS = {"bound_residuals": 3, "diagonals": 4, "leaf_diag": 2, "reg_operator": 1, "rhs_reduce": 7, "recover": 6, "compl_rhs": 8,
                  "masked_const": 0, "gather": 0}
_MASKS = ("mixed", "alloff", "allon")
_step_data = {}


def step_data(nx, my, mz, masks):
    """every array a step kernel reads, for one size and mask pattern, generated once"""
    key = (nx, my, mz, masks)
    if key in _step_data:
        return _step_data[key]
    if nx + my + mz > 4096:
        for k in [k for k in _step_data if sum(k[:3]) > 4096]:
            del _step_data[k]
    rng = np.random.default_rng([nx, my, mz, _MASKS.index(masks)])
    ncp, nyz = 2 * mz + 2 * nx, my + mz
    pz, px = (rng.integers(0, 4, m) if masks == "mixed" else np.full(m, 0 if masks == "alloff" else 3) for m in (mz, nx))
    if masks == "mixed":      # every pair pattern at the first entries and at the last one
        pz[:4], px[:4] = np.arange(4)[:min(4, mz)], np.arange(4)[::-1][:min(4, nx)]
        pz[-1:], px[-1:] = 3, 3
    on = np.concatenate([pz & 1, pz >> 1, px & 1, px >> 1]).astype(bool)
    d = dict(on=on, M=np.where(on, 1.0, np.where(np.arange(ncp) % 2 == 1, -0.0, 0.0)))
    pos = lambda n: rng.random(n) + 0.05      # noqa: E731
    # branch kernels: behind a mask that is off, G = 0 and NaN in L, rL, rG
    d["G"], d["L"] = np.where(on, pos(ncp), 0.0), np.where(on, pos(ncp), np.nan)
    d["rG"], d["rL"] = np.where(on, rng.standard_normal(ncp), np.nan), np.where(on, rng.standard_normal(ncp), np.nan)
    # kernels that multiply by the mask: large finite values behind it
    d["Gm"], d["Lm"] = np.where(on, pos(ncp), 1e150), np.where(on, pos(ncp), 1e150)
    d["dGm"], d["dLm"] = np.where(on, rng.standard_normal(ncp), 1e150), np.where(on, rng.standard_normal(ncp), 0.0)      # mode 1: 0 + alpha M
    d["Bd"] = np.where(on, rng.standard_normal(ncp), 1e150)
    for name, n in (("x", nx), ("s", mz), ("z", mz), ("rQ", nx), ("rAC", nyz), ("rz", mz), ("rs", mz), ("sol", nx + nyz), ("ddp", nx), ("qdiag", nx)):
        d[name] = rng.standard_normal(n)
    d["dyz"] = np.concatenate([np.zeros(my), -pos(mz)])
    nleaf = 2 * (nx + nyz) + 3
    code = rng.integers(-2 - max(mz, 1) + 1, nx, nleaf) if mz > 0 else rng.integers(-1, nx, nleaf)
    code[:3] = (nx - 1, -1, -1 - mz if mz > 0 else -1)      # the last x index, an equality row, the last inequality row
    d["code"], d["nleaf"] = code.astype(np.int64), nleaf
    npack = nx + nyz + 5
    d["perm"], d["npack"] = rng.permutation(npack + 7)[:npack].astype(np.int64), npack
    d["gin"] = rng.standard_normal(npack + 7)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    _step_data[key] = d
    return d


class StepCase:
    group = "step_kernels"

    def __init__(self, cid, kernel, dims, masks="mixed", flag=0, scalars=(), variant=""):
        self.id, self.kernel, self.dims, self.masks, self.flag, self.scalars, self.variant = cid, kernel, dims, masks, flag, tuple(scalars), variant


STEP_CASES = {}
_NAN = lambda a: np.full(a.shape, np.nan)     # noqa: E731
GONDZIO = (0.0, 0.7, 0.6, 0.1, 0.4)           # alpha ap ad rmin rmax: products of the data fall below rmin, inside, above rmax and above 2 rmax


def _step(cid, *a, **k):
    assert cid not in STEP_CASES, cid
    STEP_CASES[cid] = StepCase(cid, *a, **k)


for _d in STEP_DIMS:
    _t = "x".join(map(str, _d))
    for _mk in (_MASKS if sum(_d) < 4096 else ("mixed",)):
        _s = f"{_t}-{_mk}"
        _step(f"bound_residuals-{_s}", "bound_residuals", _d, _mk)
        _step(f"diagonals-{_s}", "diagonals", _d, _mk, scalars=(1e-6,))
        for _z in (0, 1):
            _step(f"rhs_reduce-{_s}-zero_lin{_z}", "rhs_reduce", _d, _mk, flag=_z)
            _step(f"recover-{_s}-zero_lin{_z}", "recover", _d, _mk, flag=_z)
        _step(f"compl_rhs-{_s}-mode0", "compl_rhs", _d, _mk, flag=0, scalars=GONDZIO)
        _step(f"compl_rhs-{_s}-mode1", "compl_rhs", _d, _mk, flag=1, scalars=(0.37,) + GONDZIO[1:])
        _step(f"compl_rhs-{_s}-mode2", "compl_rhs", _d, _mk, flag=2, scalars=GONDZIO)
        _step(f"masked_const-{_s}-set", "masked_const", _d, _mk, flag=0, scalars=(2.5,))
        _step(f"masked_const-{_s}-add", "masked_const", _d, _mk, flag=1, scalars=(0.1,))
    _step(f"leaf_diag-{_t}", "leaf_diag", _d, scalars=(1e-8, 3e-8, 2e-8))
    _step(f"leaf_diag-{_t}-qdiag", "leaf_diag", _d, scalars=(1e-8, 3e-8, 2e-8), variant="qdiag")
    _step(f"reg_operator-{_t}", "reg_operator", _d, scalars=(1e-8, 1e-9))
    _step(f"gather-{_t}", "gather", _d, flag=0)
    _step(f"scatter-{_t}", "gather", _d, flag=1)
STEP_IDS = sorted(STEP_CASES, key=lambda c: (sum(STEP_CASES[c].dims), STEP_CASES[c].dims, c))


def step_args(case):
    """(ins, out lengths, n, idx) of a case, in the order of pips_ipm_probe_step"""
    nx, my, mz = case.dims
    d = step_data(nx, my, mz, case.masks)
    ncp, nyz, k, z = 2 * mz + 2 * nx, my + mz, case.kernel, case.flag
    lin = (lambda a: _NAN(a) if z else a)
    if k == "bound_residuals":
        return [d["x"], d["s"], d["z"], d["G"], d["Lm"], d["M"], d["Bd"]], [mz, ncp], 0, None      # rz reads L whatever the mask says
    if k == "diagonals":
        return [d["G"], d["L"], d["M"]], [nx, nx, nyz], 0, None
    if k == "leaf_diag":
        return [d["ddp"], -d["dyz"][my:], d["qdiag"] if case.variant == "qdiag" else None], [d["nleaf"]], d["nleaf"], d["code"]
    if k == "reg_operator":
        return [d["ddp"], d["dyz"]], [nx, nyz], 0, None
    if k == "rhs_reduce":
        return [lin(d["rQ"]), lin(d["rAC"]), lin(d["rz"]), lin(d["rG"]), d["rL"], d["G"], d["L"], d["M"], d["dyz"]], [nx + nyz, mz], 0, None
    if k == "recover":
        return [d["sol"], d["rs"], lin(d["rG"]), d["rL"], d["G"], d["L"], d["M"], d["dyz"]], [nx + mz + ncp, nyz + ncp], 0, None
    if k == "compl_rhs":
        return [d["Gm"], d["Lm"], d["dGm"], d["dLm"], d["M"]], [ncp], ncp, None
    if k == "masked_const":
        return [d["M"]], [ncp], ncp, None
    n = d["npack"]
    return ([d["gin"]], [n], n, d["perm"]) if z == 0 else ([d["gin"][:n]], [n + 7], n, d["perm"])


def step_outs(case):
    """the outputs before the call: SENTINEL and GUARD more entries; k_masked_const's y holds values (its add mode reads them)"""
    _, lens, _, _ = step_args(case)
    outs = [np.full(m + GUARD, SENTINEL) for m in lens]
    if case.kernel == "masked_const":
        nx, my, mz = case.dims
        outs[0][:lens[0]] = np.random.default_rng([nx, my, mz, 5]).standard_normal(lens[0])
    return outs


def step_formula(T, case, ins, outs0, n, idx, defect=None):
    """the statements of the kernel in the type T: a list of writes (output, positions, values, roundings k, sum|terms|)"""
    nx, my, mz = case.dims
    kern, flag, sc = case.kernel, case.flag, case.scalars
    c = [None if a is None else np.asarray(a).astype(T) for a in ins]
    W = []
    three = kern in ("rhs_reduce", "recover")
    nloop = {"bound_residuals": max(nx, mz), "diagonals": max(nx, mz), "reg_operator": max(nx, my + mz), "rhs_reduce": max(nx, mz, my),
             "recover": max(nx, mz, my)}.get(kern, n)
    if defect == "rows_beyond_min_dropped" and kern in ("bound_residuals", "diagonals", "rhs_reduce", "recover"):
        nloop = max(min(nx, mz), my) if three else min(nx, mz)
    if defect == "my_rows_dropped" and three:
        nloop = max(nx, mz)
    if defect == "second_trip_dropped":
        nloop = min(nloop, TRIP)
    loop = lambda m: np.arange(min(m, nloop))     # noqa: E731
    put = lambda o, pos, val, k, mag: W.append((o, np.asarray(pos), val, k, mag))     # noqa: E731
    ab = np.abs
    uz, ux = (0, 0) if defect == "upper_at_lower_offset" else (mz, nx)      # where the upper pair of an entry is read
    o = 2 * mz
    with np.errstate(all="ignore"):
        if kern == "bound_residuals":
            x, s, z, G, L, M, Bd = c
            if defect == "mask_ignored":
                M = np.ones_like(M)
            iz, ix = loop(mz), loop(nx)
            put(0, iz, z[iz] - L[iz] + L[uz + iz], 2, ab(z[iz]) + ab(L[iz]) + ab(L[uz + iz]))
            put(1, iz, (s[iz] - Bd[iz]) * M[iz] - G[iz], 3, (ab(s[iz]) + ab(Bd[iz])) * ab(M[iz]) + ab(G[iz]))
            j = uz + iz
            put(1, mz + iz, (s[iz] - Bd[j]) * M[j] + G[j], 3, (ab(s[iz]) + ab(Bd[j])) * ab(M[j]) + ab(G[j]))
            put(1, o + ix, (x[ix] - Bd[o + ix]) * M[o + ix] - G[o + ix], 3, (ab(x[ix]) + ab(Bd[o + ix])) * ab(M[o + ix]) + ab(G[o + ix]))
            j = o + ux + ix
            put(1, o + nx + ix, (x[ix] - Bd[j]) * M[j] + G[j], 3, (ab(x[ix]) + ab(Bd[j])) * ab(M[j]) + ab(G[j]))
        elif kern == "diagonals":
            G, L, M = c
            on = np.ones(M.shape, dtype=bool) if defect == "mask_ignored" else ins[2] != 0.0
            quo = lambda j: np.where(on[j], L[j] / np.where(on[j], G[j], 1), 0)     # noqa: E731
            iz, ix = loop(mz), loop(nx)
            om = quo(iz) + quo(uz + iz)
            S = ab(quo(iz)) + ab(quo(uz + iz))
            nz = om != 0
            put(2, my + iz, np.where(nz, -1 / np.where(nz, om, 1), 0), np.where(nz, 3 * S / np.where(nz, ab(om), 1) + 2, 0), np.where(nz, 1 / np.where(nz, ab(om), 1), 0))
            v = quo(o + ix) + quo(o + ux + ix)
            S = ab(quo(o + ix)) + ab(quo(o + ux + ix))
            free = ~(on[o + ix] | on[o + ux + ix])
            put(0, ix, v, 3, S)
            put(1, ix, v + np.where(free, T(sc[0]), 0), 4, S + np.where(free, ab(T(sc[0])), 0))
        elif kern == "leaf_diag":
            ddp, nom, qd = c
            p = loop(n)
            code = np.asarray(idx)[p]
            xs, eq, iq = p[code >= 0], p[code == -1], p[code <= -2]
            cx = np.asarray(idx)[xs]
            if qd is not None:
                put(0, xs, ddp[cx] + qd[cx] + T(sc[0]), 2, ab(ddp[cx]) + ab(qd[cx]) + abs(sc[0]))
            else:
                put(0, xs, ddp[cx] + T(sc[0]), 1, ab(ddp[cx]) + abs(sc[0]))
            put(0, eq, np.full(eq.size, -T(sc[1])), 0, 0)
            ci = -2 - np.asarray(idx)[iq]
            put(0, iq, nom[ci] - T(sc[2]), 1, ab(nom[ci]) + abs(sc[2]))
        elif kern == "reg_operator":
            ddp, dyz = c
            ix, iy = loop(nx), loop(my)
            iz = np.arange(my, min(my + mz, nloop))
            put(0, ix, ddp[ix] + T(sc[0]), 1, ab(ddp[ix]) + abs(sc[0]))
            put(1, iy, np.full(iy.size, -(T(sc[1]) + T(sc[0]))), 1, abs(sc[1]) + abs(sc[0]))
            put(1, iz, dyz[iz] - T(sc[0]), 1, ab(dyz[iz]) + abs(sc[0]))
        elif kern in ("rhs_reduce", "recover"):
            zl = bool(flag) and defect != "zero_lin_ignored"
            Mraw = ins[7] if kern == "rhs_reduce" else ins[6]
            on = np.ones(Mraw.shape, dtype=bool) if defect == "mask_ignored" else Mraw != 0.0
            if kern == "rhs_reduce":
                rQ, rAC, rz, rG, rL, G, L, M, dyz = c
                lin0 = (lambda a, j: np.zeros(j.size, dtype=T) if zl else a[j])

                def pairs(base, lo, up):      # r = base + ((L rG + rL) / G)[lo] + ((L rG - rL) / G)[up] where the masks are on, with its sum|terms|
                    def part(j, sign):
                        num = (np.zeros(j.size, dtype=T) if zl else L[j] * rG[j]) + sign * rL[j]
                        nm = (np.zeros(j.size, dtype=T) if zl else ab(L[j] * rG[j])) + ab(rL[j])
                        return np.where(on[j], num / G[j], 0), np.where(on[j], nm / ab(G[j]), 0)
                    (a1, m1), (a2, m2) = part(lo, 1), part(up, -1)
                    return base + a1 + a2, ab(base) + m1 + m2
                ix, iy, iz = loop(nx), loop(my), loop(mz)
                r, m = pairs(lin0(rQ, ix), o + ix, o + ux + ix)
                put(0, ix, r, 5, m)
                put(0, nx + iy, lin0(rAC, iy), 0, 0)
                r, m = pairs(lin0(rz, iz), iz, uz + iz)
                put(1, iz, r, 5, m)
                put(0, nx + my + iz, lin0(rAC, my + iz) - dyz[my + iz] * r, 7, ab(lin0(rAC, my + iz)) + ab(dyz[my + iz]) * m)
            else:
                sol, rs, rG, rL, G, L, M, dyz = c
                lin0 = (lambda j: np.zeros(j.size, dtype=T) if zl else rG[j])
                ix, iy, iz = loop(nx), loop(my), loop(mz)
                gP, gD = nx + mz, my + mz         # dG = sP + gP, dL = sD + gD

                def pair(d0, m0, lo, up):      # the four steps of one entry's pairs from the primal step d0 (dx or ds) with sum|terms| m0
                    for j, sign in ((lo, 1), (up, -1)):
                        dv = np.where(on[j], sign * (d0 - lin0(j)), 0)
                        mv = np.where(on[j], m0 + ab(lin0(j)), 0)
                        dg = np.where(on[j], (rL[j] - L[j] * dv) / G[j], 0)
                        mg = np.where(on[j], (ab(rL[j]) + ab(L[j]) * mv) / ab(G[j]), 0)
                        yield j, dv, mv, dg, mg
                dx = sol[ix]
                put(0, ix, -dx, 0, 0)
                for (j, dv, mv, dg, mg), w in zip(pair(dx, ab(dx), o + ix, o + ux + ix), (o + ix, o + nx + ix)):
                    put(0, gP + w, -dv, 1, mv)
                    put(1, gD + w, -dg, 4, mg)
                put(1, iy, sol[nx + iy], 0, 0)
                dzp = sol[nx + my + iz]
                put(1, my + iz, dzp, 0, 0)
                dz = dzp if defect == "dz_sign" else -dzp
                ds = -(dyz[my + iz] * (rs[iz] - dz))
                ms = ab(dyz[my + iz]) * (ab(rs[iz]) + ab(dz))
                put(0, nx + iz, -ds, 2, ms)
                for (j, dv, mv, dg, mg), w in zip(pair(ds, ms, iz, uz + iz), (iz, mz + iz)):
                    put(0, gP + w, -dv, 3, mv)
                    put(1, gD + w, -dg, 6, mg)
        elif kern == "compl_rhs":
            G, L, dG, dL, M = c
            if defect == "mask_ignored":
                M = np.ones_like(M)
            i = loop(n)
            alpha, ap, ad, rmin, rmax = (T(v) for v in sc)
            if flag == 0:
                put(0, i, G[i] * L[i], 1, ab(G[i] * L[i]))
            elif flag == 1:
                put(0, i, dG[i] * dL[i] + alpha * M[i], 3, ab(dG[i] * dL[i]) + ab(alpha * M[i]))
            else:
                p = (G[i] + ap * dG[i]) * (L[i] + ad * dL[i])
                mp = (ab(G[i]) + ab(ap * dG[i])) * (ab(L[i]) + ab(ad * dL[i]))
                t = np.where(p < rmin, rmin - p, np.where(p > rmax, rmax - p, 0))
                t = np.where(t < -rmax, -rmax, t)
                put(0, i, -t * M[i], 8, (mp + ab(rmin) + ab(rmax)) * ab(M[i]))
        elif kern == "masked_const":
            i = loop(n)
            on = np.ones(n, dtype=bool)[i] if defect == "mask_ignored" else (ins[0] != 0.0)[i]
            y = np.asarray(outs0[0])[i]       # one FP64 addition, the same on both sides: not repeated in T
            put(0, i, np.where(on, y + np.float64(sc[0]) if flag else np.full(i.size, sc[0]), 0.0), 0, 0)
        else:
            i = loop(n)
            src = np.asarray(idx)[i]
            if flag:
                put(0, src, c[0][i], 0, 0)
            else:
                put(0, i, c[0][src], 0, 0)
    return W


def judge_step(case, be):
    nx, my, mz = case.dims
    ins, lens, n, idx = step_args(case)
    outs0 = step_outs(case)
    outs = [a.copy() for a in outs0]
    be.step(case.kernel, nx, my, mz, ins, outs, n=n, flag=case.flag, scalars=case.scalars, idx=idx, case=case)
    W = step_formula(LD, case, ins, outs0, n, idx)
    written = [np.zeros(a.size, dtype=bool) for a in outs]
    worst, why = 0.0, ""
    for o, pos, val, k, mag in W:
        if pos.size == 0:
            continue
        assert not written[o][pos].any(), (case.id, o)
        written[o][pos] = True
        got = outs[o][pos]
        if not np.isfinite(got).all() and np.isfinite(val.astype(np.float64)).all():
            return Verdict(False, "step_kernels", np.inf, f"output {o}: a value that is not finite (an entry behind a mask or a cleared residual read?)")
        exact = np.broadcast_to(np.asarray(k) == 0, pos.shape)
        if exact.any() and not _same_bits(got[exact], val.astype(np.float64)[exact]):
            j = np.flatnonzero(exact & (_bits(got) != _bits(val.astype(np.float64))))[0]
            return Verdict(False, "step_kernels", np.inf, f"output {o} at {pos[j]}: {got[j]!r} for the exact {float(val[j])!r}")
        # k roundings of u in the kernel, and as many of 2^-64 in the long-double reference
        r = _ratio(np.abs(got.astype(LD) - val)[~exact], (np.broadcast_to(k, pos.shape) * (LD(U) + LD(2.0) ** -64) * np.broadcast_to(mag, pos.shape))[~exact])
        if r > worst:
            worst, why = r, f"output {o}"
        if r > 1.0:
            return Verdict(False, "step_kernels", r, f"output {o}: |got - ref| / (k u sum|terms|)")
    for o in range(len(outs)):
        if not _same_bits(outs[o][~written[o]], outs0[o][~written[o]]):
            j = np.flatnonzero(~written[o] & (_bits(outs[o]) != _bits(outs0[o])))[0]
            return Verdict(False, "step_kernels", np.inf, f"output {o} at {j} (length {lens[o]}): written where the kernel has no statement")
    return Verdict(True, "step_kernels", worst, why)


# =================================================================================================================================
# the FP64 host backend and its defects
# =================================================================================================================================
class HostBackend:
    """The three probe entries in FP64 numpy.  defect=None: the plain formulas.  Otherwise one of DEFECTS, emulated with the grid rules of
    csrc/harness.hip.  summation: how reduce() adds ('pairwise': numpy's sum; 'sequential': one entry after the other)."""

    def __init__(self, defect=None, summation="pairwise"):
        assert defect is None or defect in DEFECTS, defect
        self.defect, self.summation = defect, summation

    def spmv(self, mode, nrows, ncols, rp, ci, v, x, out, e0=None, e1=None, e2=None, e3=None, split=0, lin=0, r0e=0, r1b=0, r1e=0, pred=-1):
        D = self.defect
        rp = np.asarray(rp, dtype=np.int64)
        lens = np.diff(rp)
        nnz = int(rp[-1])
        lanes = 0 if nrows == 0 else (4 if nnz < 6 * nrows else 8)
        is_long = lens > CSR_LONG_ROW
        long_rows = np.flatnonzero(is_long).astype(np.int32)
        if pred == 0 and D != "pred_ignored":
            return lanes, long_rows
        if nrows == 0:
            return lanes, long_rows
        prod = np.asarray(v) * np.asarray(x)[np.asarray(ci)]
        pos = np.arange(nnz) - np.repeat(rp[:-1], lens)
        rowof = np.repeat(np.arange(nrows), lens)
        keep = np.ones(nnz, dtype=bool)
        if D == "first_lpr_entries_only":
            keep &= is_long[rowof] | (pos < lanes)
        if D == "last_long_part_dropped":
            part = -(-lens // LONG_PARTS)
            keep &= ~(is_long[rowof] & (pos >= (LONG_PARTS - 1) * part[rowof]))
        s = np.zeros(nrows)
        ne = lens > 0
        if ne.any():
            s[ne] = np.add.reduceat(np.where(keep, prod, 0.0), rp[:-1][ne])
        r = np.arange(nrows)
        rep = ((r < r0e) | ((r >= r1b) & (r < r1e))) if lin else np.zeros(nrows, dtype=bool)
        if D == "replicated_full_epilogue":
            rep = np.zeros(nrows, dtype=bool)
        if D == "e3_ignored":
            e3 = None
        if D == "lin2_as_lin1":
            lin = min(lin, 1)
        e = [e0, e1, e2, e3]
        val = epilogue(np.float64, mode, s, e, split, lin, rep)[0]
        if D == "split_off_by_one" and mode == SP_RAC and split < nrows:
            val[split] = s[split]                                  # the row at the split reads neither operand
        write = np.ones(nrows, dtype=bool)
        sh = 2 if lanes == 4 else 3
        step = (egrid((2 if lanes == 4 else 4) * nrows) * 256) >> sh
        if D == "later_trips_dropped":
            write &= is_long | (r < 2 * step)
        if D == "second_row_dropped":
            write &= is_long | (r % (2 * step) < step)
        if D == "threshold_off_by_one":
            write &= lens != CSR_LONG_ROW + 1
        if D == "long_rows_past_256_unfinished":
            write &= ~is_long | (np.cumsum(is_long) <= 256)
        out[:nrows][write] = val[write]
        return lanes, long_rows

    def reduce(self, terms, out, pred=-1):
        D = self.defect
        if pred == 0:
            return out
        res = []
        for t in terms:
            kind, n = t["kind"], t["n"]
            if n == 0:
                res.append(red_identity(kind))
                continue
            v = red_terms(np.float64, kind, t.get("p", 0.0), t.get("q", 0.0), {r: t.get(r) for r in "abcdw"}, D)[0]
            j = np.arange(n)
            if D == "tail_dropped":
                v = v[(j % RED_STRIDE) + 4 * RED_STRIDE * (j // RED_STRIDE // 4) + 3 * RED_STRIDE < n]
            if D == "last_partial_left_out":
                v = v[(j // 256) % RED_GRID != RED_GRID - 1]
            if v.size == 0:
                res.append(red_identity(kind))
            elif kind == R_ABSMAX:
                res.append(float(np.fmax.reduce(v)))
            elif not _is_sum(kind):
                res.append(float(np.fmin.reduce(v)))
            elif D == "float32_sum":
                res.append(float(np.add.reduce(v, dtype=np.float32)))
            else:
                res.append(float(np.cumsum(v)[-1] if self.summation == "sequential" else v.sum()))
        if D == "neighbour_partials":
            res = res[1:] + res[:1]
        out[:len(terms)] = res
        return out

    def step(self, kernel, nx, my, mz, ins, outs, n=0, flag=0, scalars=(), idx=None, case=None):
        outs0 = [a.copy() for a in outs]
        for o, pos, val, k, mag in step_formula(np.float64, case, ins, outs0, n, idx, self.defect):
            outs[o][pos] = val


def judge(case, be, depth=None):
    if isinstance(case, SpCase):
        return judge_sp(case, be)
    return judge_red(case, be, depth) if isinstance(case, RedCase) else judge_step(case, be)


CASES = {**SP_CASES, **RED_CASES, **STEP_CASES}
assert len(CASES) == len(SP_CASES) + len(RED_CASES) + len(STEP_CASES)

# ---- which cases reject which defect (asserted by tests/test_harness_kernels_reference_cpu.py) ----------------------------------------------
KILLERS = {
    "later_trips_dropped": ("l8-r131073-qx", "l8-r300001-kyz", "l4-r262145-qx", "l4-r600001-kyz"),
    "second_row_dropped": ("l8-r63-qx", "l8-r65-kyz", "l8-r131071-qx", "l4-r262145-kyz", "epi4-kyz-lin0-both"),
    "first_lpr_entries_only": ("l8-r9-qx", "l4-r5-kyz", "l8-r65-qx", "epi4-kyz-lin0-both"),
    "threshold_off_by_one": ("l8-r7-qx", "l8-r8-kyz", "l4-r262144-qx", "epi8-rq-lin1-both", "long1-rac"),
    "last_long_part_dropped": ("l8-r8-qx", "l8-r63-kyz", "all-long-rq", "l8-r131073-kx-e3"),
    "long_rows_past_256_unfinished": ("long257-qx", "long257-rac", "long257-rq"),
    "replicated_full_epilogue": ("epi8-rq-lin1-both", "epi4-rac-lin1-both", "epi8-kx-e3-lin2-both", "epi8-res_yz-lin2-tail", "epi4-kyz-lin1-both"),
    "e3_ignored": ("epi8-rq-e3-lin0-both", "epi4-kx-e3-lin1-both", "epi8-res_x-e3-lin2-both", "l8-r131073-kx-e3"),
    "lin2_as_lin1": ("epi8-rq-e3-lin2-both", "epi4-kx-e3-lin2-both", "epi8-res_x-e3-lin2-tail"),
    "split_off_by_one": ("epi8-rac-split11-lin0", "epi4-rac-split11-lin0", "epi8-rac-split0-lin0", "long255-rac"),
    "pred_ignored": ("epi8-kyz-pred0", "epi4-res_x-e3-pred0", "long257-rq-pred0", "l8-r300001-kyz-pred0"),
    "tail_dropped": ("dot-n1", "dot-n65537", "shifted_w-n262143", "absmax-n255", "planted-at600000", "dot_onesigned-n600001"),
    "last_partial_left_out": ("dot-n65536", "dot_onesigned-n600001", "planted-at65535", "shifted-n262145"),
    "mask_gt_zero": ("min_masked-minus-one-on", "planted-at0"),
    "stepbound_le_zero": ("stepbound-zero-b",),
    "weight_ignored": ("dot_w-n257", "shifted_w-n600001", "absmax_w-n65537", "planted-at256"),
    "q_ignored": ("shifted-q", "shifted-n1", "shifted_w-n600001"),
    "neighbour_partials": ("pack12-mixed", "pack12-mixed-reversed", "pack12-dot-at0", "pack12-dot-at5", "pack12-dot-at11"),
    "float32_sum": ("dot-n1", "dot_onesigned-n600001", "shifted-n257", "dot_w-n65536"),
    "second_trip_dropped": ("bound_residuals-524289x10x17-mixed", "diagonals-10x17x524289-mixed", "rhs_reduce-10x524289x17-mixed-zero_lin0",
                            "recover-10x524289x17-mixed-zero_lin1", "compl_rhs-524289x10x17-mixed-mode2", "masked_const-10x17x524289-mixed-set",
                            "leaf_diag-10x524289x17", "reg_operator-10x524289x17", "gather-524289x10x17", "scatter-10x17x524289"),
    "rows_beyond_min_dropped": ("bound_residuals-5x3x0-mixed", "diagonals-2x1x7-mixed", "rhs_reduce-1x0x0-mixed-zero_lin0", "recover-2x1x7-allon-zero_lin0",
                                "bound_residuals-10x17x524289-mixed"),
    "my_rows_dropped": ("rhs_reduce-3x5x2-mixed-zero_lin0", "recover-3x5x2-alloff-zero_lin1", "rhs_reduce-10x524289x17-mixed-zero_lin0",
                        "recover-10x524289x17-mixed-zero_lin0"),
    "mask_ignored": ("bound_residuals-3x5x2-mixed", "diagonals-2x1x7-alloff", "rhs_reduce-5x3x0-mixed-zero_lin0", "recover-300x100x200-mixed-zero_lin1",
                     "compl_rhs-3x5x2-mixed-mode1", "compl_rhs-3x5x2-mixed-mode2", "compl_rhs-300x100x200-alloff-mode2", "masked_const-2x1x7-mixed-set", "masked_const-5x3x0-alloff-add"),
    "zero_lin_ignored": ("rhs_reduce-1x0x0-allon-zero_lin1", "recover-3x5x2-mixed-zero_lin1", "rhs_reduce-10x17x524289-mixed-zero_lin1"),
    "upper_at_lower_offset": ("bound_residuals-2x1x7-allon", "diagonals-3x5x2-mixed", "rhs_reduce-300x100x200-mixed-zero_lin0", "recover-5x3x0-allon-zero_lin0"),
    "dz_sign": ("recover-2x1x7-mixed-zero_lin0", "recover-3x5x2-allon-zero_lin1", "recover-10x17x524289-mixed-zero_lin0"),
}
