"""The cases of tests/test_border_products_judged_gpu.py and tests/test_border_products_reference_cpu.py: the two border products of a leaf batch

    pips_hip_batch_border_tmult_dev   b0  += alpha * sum_b Br_b^T z_b     (addLniziLinkCons)
    pips_hip_batch_border_mult_dev    t_b += alpha * Br_b x0              (LniTransMult)

on every path (k_border_tmult; k_border_mult_rows; deterministic mode: k_border_rowdot / k_border_entry_products + k_gather_slots over g_btm /
g_bm), with the reference, the predicate that judges a result, a host backend and host emulations of plausible defects.  Host-only.

A batch is a list of blocks (n_b, Bt_b): Bt_b the CSR of Br_b^T (S rows over the block's n_b leaf rows) as LeafBatch.set_block takes it, or None for a
block without a border; K_b is a diagonal (the products read the border alone).  By csrc/layout.cpp (layout_border_csr) the border rows of a batch are
(blocks that have a border) x S in block order, the rows of a block with Bt = None are absent, and a row's entries address the flat leaf vector at the
block's x_off, which counts every block before it, bordered or not.

Reference.  Both products in np.longdouble from the Csr objects of the batch, the caller's initial b0 / t and alpha included: ref_i = y0_i + alpha
sum_k a_k x_k over the n_i entries (products) that flow into output entry i; T_i = |y0_i| + |alpha| sum_k |a_k| |x_k|.

Bound (u = 2^-53, gamma(k) = k u / (1 - k u)).   |got_i - ref_i| <= gamma(n_i + 3) T_i.   Derivation: every operation of the kernels is an FP64
product, sum or fused multiply-add, each with a relative error of at most u, so got_i = y0_i prod(1 + d) + alpha sum_k a_k x_k prod_k(1 + d), |d| <= u,
and by Higham's Lemma 3.1 a product of r such factors differs from 1 by at most gamma(r).  It remains to count the roundings a term passes through.
Let output i be fed by m_i non-empty border rows (row-side form: one list) of n_row entries each, sum n_row = n_i, so n_row + (m_i - 1) <= n_i.
  a product a_k x_k                     the product: 1 (none under an FMA); the additions of its row's sum, in any order or tree (lanes, shuffles,
                                        a sequential loop): at most n_row - 1, since a sum of n_row terms has n_row - 1 additions and the first
                                        addition to 0.0 is exact; alpha: 1 (alpha s of a row, or alpha x0 before the product in
                                        k_border_entry_products); the way into the output: the row's own atomic add and those of the rows that
                                        arrive later, at most m_i - or the gather's sum of the m_i slots (m_i - 1 additions) and its one addition
                                        to the target.  Together at most 1 + (n_row - 1) + 1 + m_i <= n_i + 2.
  y0_i                                  the additions to the output: at most m_i <= n_i.
So every term carries at most n_i + 2 roundings, whatever the order, with or without FMA, atomics or gather: gamma(n_i + 2) T_i.  The third unit
pays for the reference's own error (numpy's long-double sums: a few hundred roundings of 2^-64 = u / 2048 at most) and for the conversion of alpha.
The bound is derived, not measured; nothing is compared with a device's earlier output (bit-identity of repeated calls aside).

Untouched entries.  An output entry that receives no product (n_i = 0: a Schur column empty in every block, a leaf row no border entry names, every
row of a block without a border) keeps its value: NaN stays NaN, every other value compares equal.  The sign of a zero is not asserted - the gather adds
+0.0 sums, which turn a -0.0 into +0.0 - but counted and reported (Verdict.zero_signs).  In every case the initial output is Gaussian with NaN at every
second untouched entry, and the input vector holds NaN wherever no border entry reads it: a read through a wrong offset shows as NaN.

Cases (CASES; ids <batch>-<product>-<what>), the smallest shapes that reach each edge:
  row_lengths   S = 12, blocks of 531 and 40 rows: border rows of 0, 1, 15, 16, 17, 33 and 531 entries (the 16 lanes of k_border_tmult with idle
                lanes, one full pass, one entry into the second and third pass, a full row); Schur column 7 empty in every block, column 1 in one
                block only, columns 3 and 6 in both (several addends into one b0 entry).
  last_wave     border-row counts 1, 3, 4, 5, 13 (4 k + 1) on one block and 21 = 3 x 7 on three: the last wave of k_border_tmult (4 rows of 16
                lanes) holds idle rows whose lanes still take part in the shuffles.
  heterogeneous blocks [None(7), 5, None(11), 300, 64, None(6)]: a block without a border in the first position, between two with one, and last;
                Schur column 4 empty everywhere, column 2 in one block, column 0 in all three.
  leaf_rows     S = 37, blocks of 25 and 9 rows: leaf row 7 named by every Schur column (a long list of k_border_mult_rows / g_bm), leaf rows 13 .. 24
                named by none (NaN and -0.0 there in t).
  every batch above: both products x alpha in {-1, 1, 0.37, -2^-20}.
  zeros         x0 / z with exact zeros: every input that feeds one chosen output entry (its sums are exactly 0: the `s != 0` skip of
                k_border_tmult; -0.0 before the call there), and a fifth of the others.
  sequence      tmult, mult, tmult, mult on one handle with the same operands: d_bt_tmp is reused in deterministic mode.  The first and third result
                must be bit-equal in deterministic mode, the second and fourth in both modes (k_border_mult_rows sums in a fixed order).
  factor        tmult, mult, factor(), tmult, mult: the same rule across the factorisation.
  second_trip   1025 blocks x S = 1024, 4 leaf rows each, 2 - 3 border entries per block: 1 049 600 border rows, 1 024 past the one trip of
                k_border_tmult (65 536 workgroups x 16 rows) and of k_border_rowdot / k_border_entry_products (4 096 x 256 threads).  The last block
                lies wholly in the second trip; it alone holds Schur columns 511 and 1023 (the last border row) and shares column 0.  Analysed only.

Host backend and defects.  HostBackend computes the products in FP64 numpy in shuffled orders, in two forms (alpha times the sum; alpha times x
before the product), from a table it lays out as the engine does.  HostBackend(defect=...) applies one of DEFECTS; KILLERS names the cases that reject
each (asserted by the CPU module)."""
import zlib

import numpy as np

import pips_ipmpp_amd as pa

U = 2.0 ** -53
LD = np.longdouble
TRIP_ROWS = 1 << 20          # border rows per trip: 65 536 workgroups x 16 rows (k_border_tmult), 4 096 x 256 threads (rowdot, entry products)
ALPHAS = {"m1": -1.0, "p1": 1.0, "0.37": 0.37, "m2^-20": -2.0 ** -20}
DEFECTS = ("store_instead_of_add", "alpha_dropped", "alpha_twice", "lane15_dropped", "rows_truncated_at_16", "last_row_dropped", "last_wave_dropped",
           "second_trip_dropped", "xoff_borderless_not_skipped", "block0_offset_everywhere", "val_p_not_val_src", "shared_column_addend_missing",
           "row_added_twice", "colidx_row_sc_exchanged")


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * LD(U) / (1 - k * LD(U))


# ---- batches ----------------------------------------------------------------------------------------------------------------------------------
class Batch:
    """blocks: [(n_b, Csr of Br_b^T or None)]"""

    def __init__(self, name, S, blocks):
        self.name, self.S, self.blocks = name, int(S), blocks
        self.n = np.array([n for n, _ in blocks], dtype=np.int64)
        self.x_off = np.concatenate([[0], np.cumsum(self.n)])
        self.N = int(self.x_off[-1])
        self.bordered = [b for b, (_, Bt) in enumerate(blocks) if Bt is not None]
        self.rows = len(self.bordered) * self.S
        self._entries = self._structure = None

    def K(self, b):
        n = int(self.n[b])
        return pa.Csr(n, n, np.arange(n + 1), np.arange(n), 2.0 + 0.25 * (np.arange(n) % 5))

    def entries(self):
        """(block, Schur column, leaf row inside the block, value) of every border entry, in the order of the Csr objects"""
        if self._entries is None:
            blk, sc, col, val = [], [], [], []
            for b in self.bordered:
                Bt = self.blocks[b][1]
                assert Bt.nrows == self.S and Bt.ncols == self.n[b]
                sc.append(np.repeat(np.arange(self.S, dtype=np.int64), np.diff(Bt.rowptr)))
                col.append(Bt.colidx.astype(np.int64))
                val.append(Bt.val)
                blk.append(np.full(Bt.nnz, b, dtype=np.int64))
            self._entries = tuple(np.concatenate(a) for a in (blk, sc, col, val))
        return self._entries

    def structure(self, op):
        """(target, input index, value, products per output entry n_i, which inputs are read) of a product, from the Csr objects"""
        if self._structure is None:
            blk, sc, col, val = self.entries()
            leaf = self.x_off[blk] + col
            n_sc, n_leaf = np.bincount(sc, minlength=self.S), np.bincount(leaf, minlength=self.N)
            self._structure = {"tmult": (sc, leaf, val, n_sc, n_leaf > 0), "mult": (leaf, sc, val, n_leaf, n_sc > 0)}
        return self._structure[op]


def _bt(S, n, rows, seed):
    """Csr of S rows over n columns; rows: {Schur column: number of entries, or the columns themselves}"""
    rng = np.random.default_rng(seed)
    count, colidx = np.zeros(S, dtype=np.int64), []
    for s in sorted(rows):
        c = rows[s]
        c = np.sort(rng.choice(n, size=c, replace=False)) if np.isscalar(c) else np.asarray(c)
        assert 0 <= s < S and c.size > 0 and (np.diff(c) > 0).all() and 0 <= c[0] and c[-1] < n
        colidx.extend(c.tolist())
        count[s] = c.size
    rowptr = np.concatenate([[0], np.cumsum(count)])
    val = rng.standard_normal(len(colidx))
    val[val == 0] = 1.0
    return pa.Csr(S, n, rowptr, colidx, val)


def _row_lengths():
    b0 = _bt(12, 531, {1: 1, 2: 15, 3: 16, 4: 17, 5: 33, 6: 531, 8: 2, 9: 16, 10: 1, 11: 5}, 1)
    b1 = _bt(12, 40, {0: 3, 3: 16, 4: 1, 6: 40, 8: 2, 11: 4}, 2)
    return Batch("row_lengths", 12, [(531, b0), (40, b1)])


def _rows(S, nblk=1):
    """every border row holds 1 - 3 entries: the last row and the rows of the last wave are not empty"""
    return Batch(f"rows{S * nblk}", S, [(10, _bt(S, 10, {s: 1 + (s + b) % 3 for s in range(S)}, [3, S, b])) for b in range(nblk)])


_HETERO_ROWS = ({0: 2, 1: 1, 3: 5, 8: 3}, {0: 20, 1: 300, 2: 7, 5: 16, 6: 17, 7: 1, 8: 31}, {0: 1, 3: 64, 5: 2, 6: 15, 8: 9})


def _hetero(name):
    B = [_bt(9, n, r, [4, n]) for n, r in zip((5, 300, 64), _HETERO_ROWS)]
    return Batch(name, 9, [(7, None), (5, B[0]), (11, None), (300, B[1]), (64, B[2]), (6, None)])


def _leaf_rows():
    rng = np.random.default_rng(5)
    r0 = {s: np.unique(np.concatenate([[7], rng.choice(13, size=s % 3, replace=False)])) for s in range(37)}
    r1 = {s: np.array([0, 8][:1 + s % 2]) for s in range(0, 37, 5)}
    return Batch("leaf_rows", 37, [(25, _bt(37, 25, r0, 6)), (9, _bt(37, 9, r1, 7))])


def _second_trip():
    S, nblk, rng = 1024, 1025, np.random.default_rng(8)
    blocks = []
    for b in range(nblk):
        if b == nblk - 1:
            rows = {0: np.array([1]), 511: np.array([0, 3]), 1023: np.array([2])}
        else:
            cols = np.sort(rng.choice(1023, size=2 + b % 2, replace=False))
            cols = cols[(cols != 511)]
            rows = {int(s): np.array([int(rng.integers(0, 4))]) for s in cols}
            if b % 97 == 0:
                rows[0] = np.array([b % 4])
        blocks.append((4, _bt(S, 4, rows, [9, b])))
    return Batch("second_trip", S, blocks)


_BUILDERS = {"row_lengths": _row_lengths, "rows1": lambda: _rows(1), "rows3": lambda: _rows(3), "rows4": lambda: _rows(4), "rows5": lambda: _rows(5),
             "rows13": lambda: _rows(13), "rows21": lambda: _rows(7, 3), "heterogeneous": lambda: _hetero("heterogeneous"),
             "heterogeneous_factor": lambda: _hetero("heterogeneous_factor"), "leaf_rows": _leaf_rows, "second_trip": _second_trip}
_batches = {}


def batch(name):
    if name not in _batches:
        _batches[name] = _BUILDERS[name]()
    return _batches[name]


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------
class Step:
    """a call: op in (tmult, mult) with alpha; or op = factor.  zeros: exact zeros in the input vector (module docstring)"""

    def __init__(self, op, alpha=0.0, zeros=False):
        self.op, self.alpha, self.zeros = op, float(alpha), zeros


class Case:
    """same_bits: (i, j, op) - the results of steps i and j must be bit-equal on a backend that repeats `op` to the bit"""

    def __init__(self, cid, group, batch_name, steps, same_bits=()):
        self.id, self.group, self.batch_name, self.steps, self.same_bits = cid, group, batch_name, tuple(steps), tuple(same_bits)


CASES = {}


def _add(cid, group, batch_name, steps, same_bits=()):
    assert cid not in CASES, cid
    CASES[cid] = Case(cid, group, batch_name, steps, same_bits)


_GROUP = {"row_lengths": "row_lengths", "rows1": "last_wave", "rows3": "last_wave", "rows4": "last_wave", "rows5": "last_wave", "rows13": "last_wave",
          "rows21": "last_wave", "heterogeneous": "heterogeneous", "leaf_rows": "leaf_rows"}
for _b, _g in _GROUP.items():
    for _op in ("tmult", "mult"):
        for _tag, _a in ALPHAS.items():
            _add(f"{_b}-{_op}-a{_tag}", _g, _b, [Step(_op, _a)])
for _b in ("row_lengths", "rows5", "heterogeneous", "leaf_rows"):
    for _op in ("tmult", "mult"):
        _add(f"{_b}-{_op}-zeros", "zeros", _b, [Step(_op, 0.37, zeros=True)])
_SEQ = [Step("tmult", 0.37), Step("mult", -1.0), Step("tmult", 0.37), Step("mult", -1.0)]
for _b in ("row_lengths", "heterogeneous"):
    _add(f"{_b}-sequence", "sequence", _b, _SEQ, [(0, 2, "tmult"), (1, 3, "mult")])
_add("heterogeneous_factor-before-and-after", "factor", "heterogeneous_factor",
     [Step("tmult", -1.0), Step("mult", 0.37), Step("factor"), Step("tmult", -1.0), Step("mult", 0.37)], [(0, 3, "tmult"), (1, 4, "mult")])
_add("second_trip-tmult-a0.37", "second_trip", "second_trip", [Step("tmult", 0.37)])
_add("second_trip-mult-am1", "second_trip", "second_trip", [Step("mult", -1.0)])
_add("second_trip-sequence", "second_trip", "second_trip", _SEQ, [(0, 2, "tmult"), (1, 3, "mult")])

BATCH_NAMES = list(_BUILDERS)
CASE_IDS = sorted(CASES, key=lambda c: (BATCH_NAMES.index(CASES[c].batch_name), c))     # a batch's cases side by side


# ---- operands and reference ---------------------------------------------------------------------------------------------------------------------
def operands(case, k):
    """(x, y0) of step k: the input vector (z / x0) and the initial output (b0 / t).  Steps of one case with the same product share them."""
    step = case.steps[k]
    if step.op == "factor":
        return None
    bt = batch(case.batch_name)
    tgt, inp, _, n_out, read = bt.structure(step.op)
    rng = np.random.default_rng([zlib.crc32(case.id.encode()), step.op == "mult"])
    x, y0 = rng.standard_normal(read.size), rng.standard_normal(n_out.size)
    assert (x != 0).all() and (y0 != 0).all()
    if step.zeros:
        x[rng.random(x.size) < 0.2] = 0.0
        t = int(np.flatnonzero(n_out > 1)[0])         # an output entry with several addends: every input that feeds it is zero
        x[inp[tgt == t]] = 0.0
        y0[t] = -0.0
    x[~read] = np.nan
    untouched = np.flatnonzero(n_out == 0)
    y0[untouched[0::2]] = np.nan
    y0[untouched[1::4]] = -0.0
    return x, y0


def reference(case, k):
    """(ref, bound, n_i) of step k in long double from the Csr objects of the batch"""
    step = case.steps[k]
    tgt, inp, val, n_out, _ = batch(case.batch_name).structure(step.op)
    x, y0 = operands(case, k)
    a, p = LD(step.alpha), val.astype(LD) * x[inp].astype(LD)
    acc, mag = np.zeros(n_out.size, dtype=LD), np.zeros(n_out.size, dtype=LD)
    np.add.at(acc, tgt, p)
    np.add.at(mag, tgt, np.abs(p))
    with np.errstate(invalid="ignore"):
        return y0.astype(LD) + a * acc, gamma(n_out + 3) * (np.abs(y0.astype(LD)) + np.abs(a) * mag), n_out


# ---- host backend ---------------------------------------------------------------------------------------------------------------------------------
class HostBackend:
    """The two products in FP64 numpy.  form: "sum_then_alpha" (y0 + alpha s) or "alpha_then_product" (y0 + sum a (alpha x)); seed: the order in
    which the products are added (a fixed seed repeats to the bit; reshuffle=True draws a new order for every call).  defect: one of DEFECTS.
    repeats: the products a backend repeats to the bit from call to call (judge() holds it to that)."""

    def __init__(self, defect=None, form="sum_then_alpha", seed=0, reshuffle=False):
        assert defect is None or defect in DEFECTS
        self.defect, self.form, self.seed, self.reshuffle, self.calls = defect, form, seed, reshuffle, 0
        self.repeats = () if reshuffle else ("tmult", "mult")

    def _table(self, bt, op):
        """(target, input index, value) per product, laid out as layout_border_csr does: border rows = bordered blocks x S, x_off over all blocks"""
        D = self.defect
        blk, sc, col, val = bt.entries()
        nnz = val.size
        rank = np.full(len(bt.blocks), -1)
        rank[bt.bordered] = np.arange(len(bt.bordered))
        row = rank[blk] * bt.S + sc                                   # ascending: blocks in order, a block's entries row by row
        pos = np.arange(nnz) - np.searchsorted(row, row, side="left")
        has = np.array([Bt is not None for _, Bt in bt.blocks])
        xoff = bt.x_off[:-1].copy()
        if D == "xoff_borderless_not_skipped":
            xoff = np.concatenate([[0], np.cumsum(np.where(has, bt.n, 0))])[:-1]
        if D == "block0_offset_everywhere":
            xoff[:] = 0
        v, keep = val, np.ones(nnz, dtype=bool)
        if D == "colidx_row_sc_exchanged":
            sc, col = col % bt.S, sc % bt.n[blk]
        leaf = xoff[blk] + col
        if D == "lane15_dropped":
            keep = pos % 16 != 15
        if D == "rows_truncated_at_16":
            keep = pos < 16
        if D == "last_row_dropped":
            keep = row != bt.rows - 1
        if D == "last_wave_dropped":
            keep = row < bt.rows // 4 * 4
        if D == "second_trip_dropped":
            keep = row < TRIP_ROWS
        if D == "shared_column_addend_missing":
            for c in range(bt.S):
                owners = np.unique(blk[sc == c])
                if owners.size > 1:
                    keep = ~((sc == c) & (blk == owners[-1]))
                    break
        if D == "val_p_not_val_src" and op == "mult":
            order = np.argsort(leaf, kind="stable")                   # src of the row-side lists: ascending (block, Schur column) per leaf row
            v = np.empty_like(val)
            v[order] = val                                            # the entry at list position q reads val[q] in place of val[src[q]]
        idx = np.flatnonzero(keep)
        if D == "row_added_twice" and nnz:
            idx = np.concatenate([idx, np.flatnonzero(row == row[0])])
        tgt, inp = (sc, leaf) if op == "tmult" else (leaf, sc)
        return tgt[idx], inp[idx], v[idx]

    def _product(self, bt, op, alpha, x, y0):
        D = self.defect
        tgt, inp, v = self._table(bt, op)
        a = 1.0 if D == "alpha_dropped" else alpha * alpha if D == "alpha_twice" else alpha
        self.calls += 1
        perm = np.random.default_rng([self.seed, self.calls if self.reshuffle else 0]).permutation(tgt.size)
        acc = np.zeros(y0.size)
        with np.errstate(all="ignore"):
            if self.form == "sum_then_alpha":
                np.add.at(acc, tgt[perm], (v * x[inp])[perm])
                acc *= a
            else:
                np.add.at(acc, tgt[perm], (v * (a * x[inp]))[perm])
        touched = np.bincount(tgt, minlength=y0.size) > 0
        out = y0.copy()
        out[touched] = acc[touched] if D == "store_instead_of_add" else y0[touched] + acc[touched]
        return out

    def run(self, case, ops):
        """ops[k] = (x, y0) or None (factor): the results of the steps, None for factor"""
        bt = batch(case.batch_name)
        return [None if o is None else self._product(bt, s.op, s.alpha, *o) for s, o in zip(case.steps, ops)]


# ---- judging ----------------------------------------------------------------------------------------------------------------------------------------
class Verdict:
    def __init__(self, ok, group, ratio=0.0, why="", zero_signs=0):
        self.ok, self.group, self.ratio, self.why, self.zero_signs = bool(ok), group, float(ratio), why, int(zero_signs)

    def __repr__(self):
        return f"Verdict(ok={self.ok}, group={self.group}, ratio={self.ratio:.4g}, zero_signs={self.zero_signs}, {self.why})"


def _same_bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def judge_step(case, k, got):
    """(ok, error / bound, why, zeros whose sign differs from the FP64 formula's) of the result of step k"""
    _, y0 = operands(case, k)
    ref, bound, n_out = reference(case, k)
    got = np.asarray(got)
    if got.shape != y0.shape or got.dtype != np.float64:
        return False, np.inf, f"step {k}: shape {got.shape} for {y0.shape}", 0
    un = n_out == 0
    kept = (got[un] == y0[un]) | (np.isnan(got[un]) & np.isnan(y0[un]))
    if not kept.all():
        i = np.flatnonzero(un)[np.flatnonzero(~kept)[0]]
        return False, np.inf, f"step {k}: entry {i} receives no product and went from {y0[i]!r} to {got[i]!r} ({(~kept).sum()} such entries)", 0
    g = got[~un]
    if not np.isfinite(g).all():
        i = np.flatnonzero(~un)[np.flatnonzero(~np.isfinite(g))[0]]
        return False, np.inf, f"step {k}: entry {i} is {got[i]!r}", 0
    err, bd = np.abs(g.astype(LD) - ref[~un]), bound[~un]
    with np.errstate(all="ignore"):
        q = np.where(bd > 0, err / np.where(bd > 0, bd, 1), np.where(err == 0, 0.0, np.inf))
    ratio = float(q.max()) if q.size else 0.0
    why = ""
    if ratio > 1.0:
        i = np.flatnonzero(~un)[int(np.argmax(q))]
        why = f"step {k}: entry {i} (n_i = {n_out[i]}): got {got[i]!r}, ref {float(ref[i])!r}, error / bound {ratio:.4g}; {(q > 1).sum()} entries beyond the bound"
    with np.errstate(invalid="ignore"):
        plain = np.where(un, y0, ref.astype(np.float64))
    signs = int(((got == 0) & (plain == 0) & (np.signbit(got) != np.signbit(plain))).sum())
    return ratio <= 1.0, ratio, why, signs


def judge(case, be):
    """run `case` on the backend and judge every step's result; the bit-equality rules hold for the products the backend repeats to the bit"""
    ops = [operands(case, k) for k in range(len(case.steps))]
    res = be.run(case, [None if o is None else (o[0].copy(), o[1].copy()) for o in ops])
    ok, ratio, whys, signs = True, 0.0, [], 0
    for k, got in enumerate(res):
        if case.steps[k].op == "factor":
            continue
        o, r, why, z = judge_step(case, k, got)
        ok, ratio, signs = ok and o, max(ratio, r), signs + z
        if why:
            whys.append(why)
    for i, j, op in case.same_bits:
        assert case.steps[i].op == case.steps[j].op == op and case.steps[i].alpha == case.steps[j].alpha
        if op in be.repeats and not _same_bits(res[i], res[j]):
            ok = False
            whys.append(f"steps {i} and {j} ({op}) differ in {(np.asarray(res[i]).view(np.uint64) != np.asarray(res[j]).view(np.uint64)).sum()} entries")
    return Verdict(ok, case.group, ratio, "; ".join(whys), signs)


# ---- which cases reject which defect (asserted by tests/test_border_products_reference_cpu.py) ----------------------------------------------------
KILLERS = {
    "store_instead_of_add": ("row_lengths-mult-ap1", "rows1-tmult-ap1", "leaf_rows-mult-a0.37", "second_trip-mult-am1"),
    "alpha_dropped": ("row_lengths-tmult-a0.37", "heterogeneous-mult-am1", "rows5-mult-am2^-20"),
    "alpha_twice": ("row_lengths-tmult-am1", "leaf_rows-mult-a0.37", "rows13-tmult-am2^-20"),
    "lane15_dropped": ("row_lengths-tmult-ap1", "row_lengths-tmult-zeros", "heterogeneous-tmult-a0.37"),
    "rows_truncated_at_16": ("row_lengths-tmult-ap1", "heterogeneous-tmult-am1"),
    "last_row_dropped": ("rows1-tmult-ap1", "rows5-tmult-a0.37", "row_lengths-tmult-am1", "heterogeneous-mult-ap1", "second_trip-tmult-a0.37"),
    "last_wave_dropped": ("rows1-tmult-ap1", "rows3-tmult-ap1", "rows5-tmult-am1", "rows13-tmult-a0.37", "rows21-tmult-ap1", "heterogeneous-tmult-ap1"),
    "second_trip_dropped": ("second_trip-tmult-a0.37", "second_trip-mult-am1", "second_trip-sequence"),
    "xoff_borderless_not_skipped": ("heterogeneous-tmult-ap1", "heterogeneous-mult-ap1", "heterogeneous_factor-before-and-after"),
    "block0_offset_everywhere": ("row_lengths-tmult-ap1", "rows21-mult-ap1", "heterogeneous-tmult-a0.37"),
    "val_p_not_val_src": ("row_lengths-mult-ap1", "heterogeneous-mult-a0.37", "leaf_rows-mult-am1", "second_trip-mult-am1"),
    "shared_column_addend_missing": ("row_lengths-tmult-ap1", "heterogeneous-tmult-am1", "rows21-tmult-ap1", "second_trip-tmult-a0.37"),
    "row_added_twice": ("rows1-tmult-ap1", "row_lengths-mult-ap1", "second_trip-sequence"),
    "colidx_row_sc_exchanged": ("rows4-tmult-ap1", "leaf_rows-mult-ap1", "heterogeneous-tmult-ap1"),
}
# ... and cases that do not reach a defect: its emulation is the plain formula there and passes
NOT_REACHED = (("lane15_dropped", "rows21-tmult-ap1"), ("lane15_dropped", "leaf_rows-tmult-ap1"), ("rows_truncated_at_16", "rows13-tmult-ap1"),
               ("last_wave_dropped", "rows4-tmult-ap1"), ("last_wave_dropped", "row_lengths-tmult-ap1"), ("second_trip_dropped", "row_lengths-tmult-ap1"),
               ("xoff_borderless_not_skipped", "row_lengths-tmult-ap1"), ("val_p_not_val_src", "row_lengths-tmult-ap1"), ("alpha_dropped", "rows5-tmult-ap1"),
               ("alpha_twice", "rows5-mult-ap1"), ("shared_column_addend_missing", "rows5-tmult-ap1"), ("block0_offset_everywhere", "rows13-mult-ap1"))
