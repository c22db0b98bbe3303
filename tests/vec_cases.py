"""The cases of tests/test_vec_judged_gpu.py and tests/test_vec_reference_cpu.py: the vector kernels of csrc/vecops.hip on every path, with their
references, the predicates that judge a result, and host emulations of plausible defects (mutants).  Host-only, numpy only.

A case names its operands (immutable base vectors per length, `base(n, name)`, plus a few patched entries), says which of them lie at 8 mod 16
and gives the scalars.  `judge(case, backend)` builds the operands through the backend (HostBackend here, the device in the GPU module), makes
the call and judges what comes back against references computed here from the same FP64 inputs.  Nothing is compared with a device's output.

Operand layout.  An operand at 8 mod 16 is the view [1:n+1] of an allocation of n + 2 doubles, an aligned one the view [2:n+2] of n + 4; every
element outside the view holds SENTINEL.  After an element-wise call the whole allocation of y is compared, so a store past either end shows.

Predicates (u = 2^-53).
  exact          scale copy set mul div divide_some select_nonzeros safe_invert add_const gondzio_projection: one rounding at most, the same in
                 numpy's FP64 formula -> bit for bit through .view(uint64) (a -0.0 against +0.0 shows).  inf_norm min stepbound find_blocking:
                 fabs, fmin, fmax and the negation are exact and the one division rounds alike on both sides -> bit for bit as well.
  multiply-add   |got - ref| <= r u sum|parts|, ref in long double.  r = roundings of the uncontracted form: axpy y + (a x): 2; axpby (a x) +
                 (b y): 3; add_product y + ((a x) z): 3; add_quotient y + ((a x) / z): 3.  An error of an inner rounding is relative to its own
                 part, the last one to the result <= sum|parts|; the contracted (FMA) form rounds less often.  Masked-off entries: unchanged bits.
  sums           |got - ref| <= (d + r) u S.  d = depth of the summation tree of k_vec_reduce / k_vec_reduce_final: a lane adds its
                 T = ceil((n - skip) / (g 256)) terms one by one to 0 (T additions, the first of them exact), the workgroup's LDS tree has
                 log2(256) = 8 levels, a lane of the final kernel adds at most ceil(2048 / 256) = 8 partials one by one and its tree has 8 levels
                 again: d = T + 24.  r = roundings inside one term: one_norm |x|: 0; dot x y: 1; sumsq_scaled q = x a (1, and q enters
                 twice) and q q (1): 3; dot_shifted: a dx, x + ., the same for the other factor, the product: 5.  S = sum of the products of
                 the absolute values of a term's parts; for dot_shifted sum (|x| + |a dx|)(|y| + |b dy|), which pays for the cancellation
                 inside a factor.  skip >= n: the identity, +0.0, exactly.  The entries below skip hold NaN: a finite result has not read them.
                 The long-double reference's own error (numpy's pairwise sum, about 140 roundings of 2^-64 = u / 14) is covered by the two
                 additions counted above that do not round (0 + t in either kernel).
  two_norm       s sqrt(q), s = inf_norm, q = sumsq_scaled with a = fl(1 / s): relative to the long-double norm at most
                 ((d + 3) / 2 + 4) u - a: 1, the sum under the root: (d + 3) / 2, the root (pow, within an ulp, not correctly rounded): 2, the
                 product: 1.  Squares that underflow (1e-300 * O(1), squared) lose less than n 2^-1074 of a q >= 1.
  weighted       sign-coherent inputs (dx_i, cx_i both negative on the blocking entries, both non-negative elsewhere), so s = dx + w cx does
                 not cancel: relative to long double with a long-double w, step = (1 - wmin) / (nw - 1): 2, step k: 1, wmin + .: 1 (all terms
                 non-negative), w cx: 1, dx + .: 1, the ratio: 1 = 7 roundings; 8 u allowed.  A bound of 0 and an infinite one are exact.

Mutants (HostBackend(defect=...)): see DEFECTS and KILLERS; the CPU module asserts that each is rejected by the cases listed for it."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
SENTINEL = -7.25e77
TRIP = 2048 * 256          # elements per trip of the scalar path, the reductions and k_find_index; pairs per trip of the pair path
WS_TRIP = 1024 * 256       # k_weighted_stepbounds
MASK_VALUES = np.array([0.0, -0.0, 1.0, -1.0, 2.0, 1e-300])     # the two zeros mean off
SUM_ROUNDINGS = {"one_norm": 0, "dot": 1, "sumsq_scaled": 3, "dot_shifted": 5}
FMA_ROUNDINGS = {"axpy": 2, "axpby": 3, "add_product": 3, "add_quotient": 3}
EXACT_ELEM = ("scale", "copy", "set", "mul", "div", "divide_some", "select_nonzeros", "safe_invert", "add_const", "gondzio_projection")
WEIGHTED_ROUNDINGS = 8
DEFECTS = ("first_trip_only", "odd_tail_dropped", "last_partial_left_out", "skip_ignored", "mask_gt_zero", "float32_sum",
           "tie_highest_index", "store_past_n", "zero_times_y", "masked_off_divided")


def vgrid(n):
    return max(1, min(2048, (n + 255) // 256))


# ---- base vectors: per length and name, generated once, immutable -----------------------------------------------------------------------------
_GAUSS = ("g1", "g2", "g3", "g4")
_SPECIAL = np.array([0.0, -0.0, 5e-324, -1e-310, 1e308, -1e308])     # safe_invert: zeros, denormals, reciprocals that are denormal
_NAMES = _GAUSS + ("p1", "p2", "mask", "wB", "wB2")
_base = {}


def _make(n, name):
    if name in _NAMES:
        rng = np.random.default_rng([n, _NAMES.index(name)])
        if name in _GAUSS:
            v = rng.standard_normal(n)
            assert (v != 0).all()
            return v
        if name in ("p1", "p2"):
            return rng.random(n) + 0.05
        if name == "mask":
            v = MASK_VALUES[rng.integers(0, 6, n)]
            k = min(n, 6)
            v[:k] = MASK_VALUES[[3, 1, 5, 0, 2, 4]][:k]    # short vectors see -1 and -0.0 first
            v[6:][-1:] = 2.0                               # the last entry (the odd tail of the pair path) is on
            return v
        v = (rng.random(n) < 0.3).astype(np.float64)       # wB, wB2: the blocking entries of a sign-coherent triple
        v[min(n, 2) - 1 if name == "wB2" else 0:][:1] = 1.0
        return v
    off = lambda: base(n, "mask") == 0                                       # noqa: E731
    sign = lambda b: np.where(base(n, b) != 0, -1.0, 1.0)                    # noqa: E731
    derived = {
        "nan": lambda: np.full(n, np.nan),
        "zeros": lambda: np.where(np.arange(n) % 2 == 0, 0.0, -0.0),
        "a1": lambda: np.abs(base(n, "g1")), "a2": lambda: np.abs(base(n, "g2")),
        "neg": lambda: -base(n, "p1"),
        "xq": lambda: np.where(off(), np.inf, base(n, "g1")),                # add_quotient: masked-off entries are inf / 0
        "zq": lambda: np.where(off(), 0.0, base(n, "g2")),
        "xd": lambda: np.where(off(), 0.0, base(n, "g1")),                   # divide_some: a zero divisor behind the mask
        "ysel": lambda: np.where(off(), np.nan, base(n, "g3")),
        "yinv": lambda: np.where(np.arange(n) % 11 < 6, _SPECIAL[np.arange(n) % 11 % 6], base(n, "g3")),
        "big200": lambda: base(n, "g1") * 1e200, "small200": lambda: base(n, "g1") * 1e-200,
        "wdx": lambda: sign("wB") * np.abs(base(n, "g1")), "wcx": lambda: sign("wB") * np.abs(base(n, "g2")),
        "wdy": lambda: sign("wB2") * np.abs(base(n, "g3")), "wcy": lambda: sign("wB2") * np.abs(base(n, "g4")),
    }
    return derived[name]()


def base(n, name):
    """the base vector `name` of length n; the vectors of one long length at a time are kept"""
    if n not in _base:
        if n > 4096:
            for m in [m for m in _base if m > 4096]:
                del _base[m]
        _base[n] = {}
    if name not in _base[n]:
        v = _make(n, name)
        v.flags.writeable = False
        _base[n][name] = v
    return _base[n][name]


class Opd:
    """an operand: a base vector and the entries set after it was copied - patches = ((indices, values), ...)"""

    def __init__(self, name, *patches):
        self.name = name
        self.patches = tuple((np.atleast_1d(np.asarray(i, dtype=np.int64)), np.atleast_1d(np.asarray(v, dtype=np.float64))) for i, v in patches)


class Handle:
    """an operand as a backend holds it: the allocation, the guard width in front of the view, the length, whether the view is at 8 mod 16"""

    def __init__(self, buf, g, n, mis):
        self.buf, self.g, self.n, self.mis = buf, g, n, mis

    @property
    def view(self):
        return self.buf[self.g:self.g + self.n]


def host_operand(n, opd, mis):
    g = 1 if mis else 2
    buf = np.full(n + 2 * g, SENTINEL)
    buf[g:g + n] = base(n, opd.name)
    for idx, vals in opd.patches:
        buf[g + idx] = vals
    return Handle(buf, g, n, mis)


# ---- FP64 numpy formulas, with the structure of the kernels where a defect needs it ---------------------------------------------------------
def _elem(op, v, a, b, x, z, on, defect):
    if op == "axpy":
        return v + a * x
    if op == "scale":
        return v * a
    if op == "copy":
        return 0.0 * v + x if defect == "zero_times_y" else x.copy()
    if op == "set":
        return 0.0 * v + a if defect == "zero_times_y" else np.full_like(v, a)
    if op == "mul":
        return v * x
    if op == "div":
        return v / x
    if op == "add_product":
        return v + a * x * z
    if op == "add_quotient":
        return v + on * (a * x / z) if defect == "masked_off_divided" else np.where(on, v + a * x / z, v)
    if op == "divide_some":
        return v / x if defect == "masked_off_divided" else np.where(on, v / x, v)
    if op == "select_nonzeros":
        return np.where(on, v, 0.0)
    if op == "safe_invert":
        return np.where(v != 0.0, 1.0 / v, 0.0)
    if op == "add_const":
        return v + a
    if op == "axpby":
        return a * x + b * v
    assert op == "gondzio_projection", op
    t = np.where(v < a, a - v, np.where(v > b, b - v, 0.0))
    return np.where(t < -b, -b, t)


def _terms(op, a, b, x, y, dx, dy, on):
    if op == "dot":
        return x * y
    if op in ("one_norm", "inf_norm"):
        return np.abs(x)
    if op == "sumsq_scaled":
        q = x * a
        return q * q
    if op == "min":
        return x
    if op == "stepbound":
        return np.where((dx < 0.0) & on, -x / dx, np.inf)
    assert op == "dot_shifted", op
    return (x + a * dx) * (y + b * dy)


def _identity(op):
    return np.inf if op in ("min", "stepbound") else 0.0


class HostBackend:
    """The vector layer in FP64 numpy.  defect=None: the plain formulas (sums sequential or pairwise).  Otherwise one of DEFECTS, emulated with
    the grid and path rules of vecops.hip."""
    error = ValueError

    def __init__(self, defect=None, summation="pairwise"):
        assert defect is None or defect in DEFECTS
        self.defect, self.summation = defect, summation

    def operand(self, n, opd, mis):
        return host_operand(n, opd, mis)

    def fetch(self, h):
        return h.buf

    def _on(self, m):
        return True if m is None else (m > 0.0 if self.defect == "mask_gt_zero" else m != 0.0)

    def elem(self, op, a, b, x, z, mask, y):
        n, D = y.n, self.defect
        if n <= 0:
            return
        pair = n >= 2 and not any(h.mis for h in (x, z, mask, y) if h is not None)
        m = n + 1 if D == "store_past_n" and pair and n % 2 else n           # the last pair reaches one past n
        ext = lambda h: None if h is None else h.buf[h.g:h.g + m]            # noqa: E731
        yv = ext(y)
        with np.errstate(all="ignore"):
            r = _elem(op, yv.copy(), a, b, ext(x), ext(z), self._on(ext(mask)), D)
        done = np.ones(m, dtype=bool)
        if D == "first_trip_only":
            done[(2 if pair else 1) * 256 * vgrid((n + 1) // 2 if pair else n):] = False
            done[n - 1] |= pair and n % 2 == 1                               # lane 0's tail is outside the loop
        if D == "odd_tail_dropped" and pair and n % 2:
            done[n - 1] = False
        yv[done] = r[done]

    def reduce(self, op, skip, a, b, x, y=None, dx=None, dy=None, mask=None):
        n, D = x.n, self.defect
        if n - skip <= 0:
            return _identity(op)
        g = vgrid(n - skip)
        lo = 0 if D == "skip_ignored" else skip
        v = lambda h: None if h is None else h.view[lo:]                     # noqa: E731
        with np.errstate(all="ignore"):
            t = _terms(op, a, b, v(x), v(y), v(dx), v(dy), self._on(v(mask)))
        if D == "first_trip_only":
            t = t[:g * 256]
        if D == "last_partial_left_out":
            t = t[(np.arange(t.size) // 256) % g != g - 1]
        if t.size == 0:
            return _identity(op)
        if op in ("min", "stepbound"):
            return float(np.fmin.reduce(t))
        if op == "inf_norm":
            return float(np.fmax.reduce(t))
        if D == "float32_sum":
            return float(np.add.reduce(t, dtype=np.float32))
        return float(np.cumsum(t)[-1] if self.summation == "sequential" else t.sum())

    def two_norm(self, x):
        s = self.reduce("inf_norm", 0, 0.0, 0.0, x)
        return 0.0 if s == 0.0 else s * self.reduce("sumsq_scaled", 0, 1.0 / s, 0.0, x) ** 0.5

    def find_blocking(self, x, dx, y, dy):
        out = np.zeros(5)
        out[0] = self.reduce("stepbound", 0, 0.0, 0.0, x, dx=dx)
        if x.n <= 0 or not out[0] < np.inf:
            return out
        with np.errstate(all="ignore"):
            cand = np.flatnonzero((dx.view < 0.0) & (-x.view / dx.view == out[0]))
        if self.defect == "first_trip_only":
            cand = cand[cand < 256 * vgrid(x.n)]
        if cand.size:
            i = cand.max() if self.defect == "tie_highest_index" else cand.min()
            out[1:] = x.view[i], dx.view[i], y.view[i], dy.view[i]
        return out

    def weighted_stepbounds(self, x, dx, cx, y, dy, cy, wmin, nw):
        if not 1 <= nw <= 16:
            raise ValueError("1 <= nw <= 16")
        out = np.full(2 * nw, np.inf)
        lim = WS_TRIP if self.defect == "first_trip_only" else x.n
        step = (1.0 - wmin) / (nw - 1) if nw > 1 else 0.0
        for k in range(nw):
            w = min(1.0, wmin + step * k)
            for j, (p, dp, cp) in enumerate(((x, dx, cx), (y, dy, cy))):
                s = dp.view[:lim] + w * cp.view[:lim]
                m = s < 0.0
                if m.any():
                    out[j * nw + k] = np.min(-p.view[:lim][m] / s[m])
        return out[:nw], out[nw:]


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, cid, kind, op, n, opds, mis=(), **p):
        self.id, self.kind, self.op, self.n, self.opds, self.mis, self.p = cid, kind, op, n, opds, frozenset(mis), p


CASES = {}


def _add(cid, kind, op, n, opds, mis=(), **p):
    assert cid not in CASES, cid
    CASES[cid] = Case(cid, kind, op, n, opds, mis, **p)


# element-wise: op -> (operands by role, a, b)
ELEM = {
    "axpy": (dict(x="g1", y="g3"), 0.37, 0.0),
    "axpby": (dict(x="g1", y="g3"), 1.7, -0.3),
    "scale": (dict(y="g3"), -1.3, 0.0),
    "copy": (dict(x="g1", y="nan"), 0.0, 0.0),                   # y holds NaN before: the two that must not read y
    "set": (dict(y="nan"), 2.5, 0.0),
    "mul": (dict(x="g1", y="g3"), 0.0, 0.0),
    "div": (dict(x="g1", y="g3"), 0.0, 0.0),
    "add_product": (dict(x="g1", z="g2", y="g3"), -1.5, 0.0),
    "add_quotient": (dict(x="xq", z="zq", mask="mask", y="g3"), 1.9, 0.0),
    "divide_some": (dict(x="xd", mask="mask", y="g3"), 0.0, 0.0),
    "select_nonzeros": (dict(mask="mask", y="ysel"), 0.0, 0.0),
    "safe_invert": (dict(y="yinv"), 0.0, 0.0),
    "add_const": (dict(y="g3"), 0.1, 0.0),
    "gondzio_projection": (dict(y="g3"), 0.2, 0.9),
}
_FULL = ("axpy", "copy", "set", "add_quotient")      # these see every length of the issue's list on both paths
# pair path (every operand aligned): n = 1 goes the scalar way (n < 2); 2 * TRIP + 1: odd tail after a full trip; + 2: the first pair of the
# second trip; + 3: that and an odd tail.  Scalar path: TRIP + 1 is one element into the second trip, 2 * TRIP + 1 one into the third.
_LEN = {
    True: {"aligned": (1, 2, 3, 255, 256, 257, 512, 513, 2 * TRIP, 2 * TRIP + 1, 2 * TRIP + 2, 2 * TRIP + 3),
           "all8": (1, 2, 3, 255, 256, 257, 512, 513, TRIP, TRIP + 1, 2 * TRIP, 2 * TRIP + 1), "single": (513, TRIP + 1)},
    False: {"aligned": (1, 2, 3, 256, 257, 2 * TRIP + 2, 2 * TRIP + 3), "all8": (1, 2, 256, 257, TRIP + 1, 2 * TRIP + 1), "single": (513,)},
}


def _elem_opds(op, roles, n):
    if op == "select_nonzeros" and n >= 3:
        # its last entry - the odd tail of the pair path - is off, over NaN: an entry that is on keeps its value, which would hide a tail never written
        return dict(mask=Opd("mask", (n - 1, -0.0)), y=Opd("ysel", (n - 1, np.nan)))
    return {r: Opd(nm) for r, nm in roles.items()}


for _op, (_roles, _a, _b) in ELEM.items():
    _L = _LEN[_op in _FULL]
    for _n in _L["aligned"]:
        _add(f"{_op}-n{_n}-aligned", "elem", _op, _n, _elem_opds(_op, _roles, _n), (), a=_a, b=_b)
    for _n in _L["all8"]:
        _add(f"{_op}-n{_n}-all8", "elem", _op, _n, _elem_opds(_op, _roles, _n), tuple(_roles), a=_a, b=_b)
    if len(_roles) > 1:
        for _r in _roles:
            for _n in _L["single"]:
                _add(f"{_op}-n{_n}-{_r}8", "elem", _op, _n, _elem_opds(_op, _roles, _n), (_r,), a=_a, b=_b)
    _add(f"{_op}-n0", "elem", _op, 0, _elem_opds(_op, _roles, 0), (), a=_a, b=_b)

# sums: op -> (operands, a, b)
SUMS = {
    "dot": (dict(x="g1", y="g2"), 0.0, 0.0),
    "one_norm": (dict(x="g1"), 0.0, 0.0),
    "sumsq_scaled": (dict(x="g1"), 0.731, 0.0),
    "dot_shifted": (dict(x="p1", dx="g1", y="p2", dy="g2"), 0.3, 0.7),
}


def _skipped(roles, n, skip):
    """the entries below skip hold NaN in every operand"""
    k = min(skip, n)
    return {r: Opd(nm, (np.arange(k), np.full(k, np.nan))) if k else Opd(nm) for r, nm in roles.items()}


for _op, (_roles, _a, _b) in SUMS.items():
    for _n in (0, 1, 2, 3, 255, 256, 257, 512, 513, TRIP, TRIP + 1, 2 * TRIP + 1):
        _add(f"{_op}-n{_n}", "sum", _op, _n, _skipped(_roles, _n, 0), (), a=_a, b=_b, skip=0)
    _add(f"{_op}-n513-all8", "sum", _op, 513, _skipped(_roles, 513, 0), tuple(_roles), a=_a, b=_b, skip=0)
    for _s in (1, 255, 256, 257, 999, 1000, 1005):
        _add(f"{_op}-n1000-skip{_s}", "sum", _op, 1000, _skipped(_roles, 1000, _s), (), a=_a, b=_b, skip=_s)
    _add(f"{_op}-n{TRIP + 8}-skip7", "sum", _op, TRIP + 8, _skipped(_roles, TRIP + 8, 7), (), a=_a, b=_b, skip=7)   # second trip: one element

for _n in (1000, TRIP + 1):
    _add(f"two_norm-n{_n}-1e200", "two_norm", "two_norm", _n, dict(x=Opd("big200")))
    _add(f"two_norm-n{_n}-1e-200", "two_norm", "two_norm", _n, dict(x=Opd("small200")))
    _add(f"two_norm-n{_n}-spike1e300", "two_norm", "two_norm", _n, dict(x=Opd("g1", (_n // 2, 1e300))))
_add("two_norm-n0", "two_norm", "two_norm", 0, dict(x=Opd("g1")))

# minima and maxima
_NM = TRIP + 1
PLANTED = (0, 255, 256, TRIP - 1, TRIP)        # first and last lane of the first workgroup, the second one, the last entry of the first trip, n - 1
for _n in (0, 1, 2, 3, 257, 513):
    _add(f"min-n{_n}", "minmax", "min", _n, dict(x=Opd("g1")))
    _add(f"inf_norm-n{_n}", "minmax", "inf_norm", _n, dict(x=Opd("g1")))
    _add(f"stepbound-n{_n}", "minmax", "stepbound", _n, dict(x=Opd("p1"), dx=Opd("g1")))
    _add(f"stepbound-n{_n}-mask", "minmax", "stepbound", _n, dict(x=Opd("p1"), dx=Opd("g1"), mask=Opd("mask")))
for _i in PLANTED:
    _add(f"min-n{_NM}-at{_i}", "minmax", "min", _NM, dict(x=Opd("g1", (_i, -50.0))), expect=-50.0)
    _add(f"inf_norm-n{_NM}-at{_i}", "minmax", "inf_norm", _NM, dict(x=Opd("g1", (_i, -60.0))), expect=60.0)
    _add(f"stepbound-n{_NM}-at{_i}", "minmax", "stepbound", _NM, dict(x=Opd("p1", (_i, 1e-6)), dx=Opd("g1", (_i, -4.0))), expect=2.5e-7)
_add(f"inf_norm-n{_NM}-all-negative", "minmax", "inf_norm", _NM, dict(x=Opd("neg")))
_R = 300000      # the runner-up
# the planted entry on behind 1e-300 and behind -1: it wins; off behind -0.0: the runner-up (on behind -1) wins
_add(f"stepbound-n{_NM}-mask-tiny-on", "minmax", "stepbound", _NM,
     dict(x=Opd("p1", (256, 1e-6)), dx=Opd("g1", (256, -4.0)), mask=Opd("mask", (256, 1e-300))), expect=2.5e-7)
_add(f"stepbound-n{_NM}-mask-minus-one-on", "minmax", "stepbound", _NM,
     dict(x=Opd("p1", (TRIP, 1e-6)), dx=Opd("g1", (TRIP, -4.0)), mask=Opd("mask", (TRIP, -1.0))), expect=2.5e-7)
_add(f"stepbound-n{_NM}-mask-planted-off", "minmax", "stepbound", _NM,
     dict(x=Opd("p1", ([256, _R], [1e-6, 2e-6])), dx=Opd("g1", ([256, _R], [-4.0, -4.0])), mask=Opd("mask", ([256, _R], [-0.0, -1.0]))),
     expect=5e-7)
_add(f"stepbound-n{_NM}-mask-all-off", "minmax", "stepbound", _NM, dict(x=Opd("p1"), dx=Opd("g1"), mask=Opd("zeros")), expect=np.inf)
_add(f"stepbound-n{_NM}-x-zero", "minmax", "stepbound", _NM, dict(x=Opd("p1", (TRIP, 0.0)), dx=Opd("g1", (TRIP, -4.0))), expect=0.0)
_add(f"stepbound-n{_NM}-no-negative-dx", "minmax", "stepbound", _NM, dict(x=Opd("p1"), dx=Opd("a1")), expect=np.inf)

# find_blocking: 600 001 entries are two trips of k_find_index and of the step bound before it
_NF = 600001
_fb = lambda *px: dict(x=Opd("p1", *px[:1]), dx=Opd("g1", *px[1:]), y=Opd("p2"), dy=Opd("g2"))     # noqa: E731
for _n in (0, 1, 7, 1000):
    _add(f"find_blocking-n{_n}", "find", "find_blocking", _n, _fb())
# three entries with exactly the same ratio 0.000125 from different numbers (powers of two apart): the lowest index is reported
_add(f"find_blocking-n{_NF}-tie3", "find", "find_blocking", _NF,
     _fb(([300, 70000, 590000], [0.001, 0.002, 0.0005]), ([300, 70000, 590000], [-8.0, -16.0, -4.0])), expect=300)
_add(f"find_blocking-n{_NF}-last", "find", "find_blocking", _NF, _fb((_NF - 1, 0.001), (_NF - 1, -8.0)), expect=_NF - 1)
_add(f"find_blocking-n{_NF}-none", "find", "find_blocking", _NF, dict(x=Opd("p1"), dx=Opd("a1"), y=Opd("p2"), dy=Opd("g2")), expect=None)

# weighted_stepbounds: TRIP + 1 entries are three trips of its grid of 1024 workgroups
_W = dict(x="p1", dx="wdx", cx="wcx", y="p2", dy="wdy", cy="wcy")
for _n in (5, TRIP + 1):
    for _nw in (1, 2, 11, 16):
        for _wmin in (0.0, 0.37, 1.0):
            _add(f"weighted-n{_n}-nw{_nw}-wmin{_wmin}", "weighted", "weighted_stepbounds", _n, {r: Opd(nm) for r, nm in _W.items()},
                 wmin=_wmin, nw=_nw)
    _o = {r: Opd(nm) for r, nm in _W.items()}
    _o.update(dx=Opd("a1"), cx=Opd("a2"))
    _add(f"weighted-n{_n}-first-triple-unbounded", "weighted", "weighted_stepbounds", _n, _o, wmin=0.37, nw=11, expect="inf-finite")
    _o = {r: Opd(nm) for r, nm in _W.items()}
    _i = _n - 2      # in the last trip
    _o.update(x=Opd("p1", (_i, 0.0)), dx=Opd("wdx", (_i, -1.0)), cx=Opd("wcx", (_i, -1.0)))
    _add(f"weighted-n{_n}-x-zero", "weighted", "weighted_stepbounds", _n, _o, wmin=0.37, nw=11, expect="zero")
_add("weighted-n0", "weighted", "weighted_stepbounds", 0, {r: Opd(nm) for r, nm in _W.items()}, wmin=0.37, nw=11)
for _nw in (0, 17):
    _add(f"weighted-n5-nw{_nw}-raises", "bad_nw", "weighted_stepbounds", 5, {r: Opd(nm) for r, nm in _W.items()}, wmin=0.37, nw=_nw)

# the workspace between calls: partials [0, 2 nw) of weighted_stepbounds, slot 2048 of the reductions, 2049.. of find_blocking
_add("interleaved-workspace", "interleave", None, _NF, {}, seq=(
    f"weighted-n{TRIP + 1}-nw11-wmin0.37", f"dot-n{TRIP + 1}", f"find_blocking-n{_NF}-tie3", "min-n513", "weighted-n5-nw16-wmin0.0",
    "find_blocking-n1000"))

CASE_IDS = sorted(CASES, key=lambda c: (CASES[c].n, CASES[c].kind == "interleave"))     # a length's cases side by side


# ---- judging --------------------------------------------------------------------------------------------------------------------------------
class Verdict:
    def __init__(self, ok, group, ratio=0.0, why=""):
        self.ok, self.group, self.ratio, self.why = bool(ok), group, float(ratio), why

    def __repr__(self):
        return f"Verdict(ok={self.ok}, group={self.group}, ratio={self.ratio:.4g}, {self.why})"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return bool(np.array_equal(_bits(a), _bits(b)))


def _ratio(err, bound):
    """the largest err / bound; an error where the bound is 0 counts as infinite"""
    err, bound = np.atleast_1d(err), np.atleast_1d(bound)
    if err.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    return float(np.max(np.where(np.isnan(q), np.inf, q)))


def operands(case, be):
    return {r: be.operand(case.n, o, r in case.mis) for r, o in case.opds.items()}


def _judge_elem(case, be):
    op, a, b = case.op, case.p["a"], case.p["b"]
    h = operands(case, be)
    be.elem(op, a, b, h.get("x"), h.get("z"), h.get("mask"), h["y"])
    got = np.array(be.fetch(h["y"]))
    r = operands(case, HostBackend())
    y0 = r["y"].buf.copy()
    HostBackend().elem(op, a, b, r.get("x"), r.get("z"), r.get("mask"), r["y"])
    want, g, n = r["y"].buf, r["y"].g, case.n
    if got.shape != want.shape:
        return Verdict(False, "exact", np.inf, "the allocation changed its length")
    if not (_same_bits(got[:g], want[:g]) and _same_bits(got[g + n:], want[g + n:])):
        return Verdict(False, "exact", np.inf, f"a sentinel beside y changed: {got[:g]} {got[g + n:]}")
    if op in ("copy", "set") and np.isnan(got).any():
        return Verdict(False, "exact", np.inf, "NaN in the result: y was read")
    if op in EXACT_ELEM:
        bad = np.flatnonzero(_bits(got) != _bits(want))
        why = f"{bad.size} entries differ, the first at {bad[0] - g}: {got[bad[0]]!r} for {want[bad[0]]!r}" if bad.size else ""
        return Verdict(bad.size == 0, "exact", np.inf if bad.size else 0.0, why)
    # multiply-add: long double from the FP64 inputs
    x, y = r["x"].view.astype(LD), y0[g:g + n].astype(LD)
    on = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        if op == "axpy":
            parts = (y, LD(a) * x)
        elif op == "axpby":
            parts = (LD(a) * x, LD(b) * y)
        elif op == "add_product":
            parts = (y, LD(a) * x * r["z"].view.astype(LD))
        else:
            on = r["mask"].view != 0.0
            parts = (y, LD(a) * x / r["z"].view.astype(LD))
    if not _same_bits(got[g:g + n][~on], y0[g:g + n][~on]):
        return Verdict(False, "multiply_add", np.inf, "a masked-off entry of y changed")
    ref = (parts[0] + parts[1])[on]
    bound = FMA_ROUNDINGS[op] * LD(U) * (np.abs(parts[0]) + np.abs(parts[1]))[on]
    ratio = _ratio(np.abs(got[g:g + n][on].astype(LD) - ref), bound)
    return Verdict(ratio <= 1.0, "multiply_add", ratio, "|got - ref| / (r u sum|parts|)")


def sum_depth(n, skip):
    """d: the additions a term passes through in k_vec_reduce and k_vec_reduce_final (module docstring)"""
    return -(-(n - skip) // (vgrid(n - skip) * 256)) + 24


def sum_reference(op, a, b, skip, h):
    """(the sum, S) in long double from the FP64 operands"""
    v = {r: hh.view[skip:].astype(LD) for r, hh in h.items()}
    a, b = LD(a), LD(b)
    if op == "dot":
        t, s = v["x"] * v["y"], np.abs(v["x"]) * np.abs(v["y"])
    elif op == "one_norm":
        t = s = np.abs(v["x"])
    elif op == "sumsq_scaled":
        t = s = (v["x"] * a) ** 2
    else:
        t = (v["x"] + a * v["dx"]) * (v["y"] + b * v["dy"])
        s = (np.abs(v["x"]) + np.abs(a * v["dx"])) * (np.abs(v["y"]) + np.abs(b * v["dy"]))
    return t.sum(), s.sum()


def sum_bound(case, depth=None):
    """(ref, the bound (d + r) u S) of a sum case; depth: another tree's depth instead of the kernel's"""
    n, skip = case.n, case.p["skip"]
    if n - skip <= 0:
        return LD(0), LD(0)
    ref, S = sum_reference(case.op, case.p["a"], case.p["b"], skip, operands(case, HostBackend()))
    d = sum_depth(n, skip) if depth is None else depth
    return ref, (d + SUM_ROUNDINGS[case.op]) * LD(U) * S


def _judge_sum(case, be, depth=None):
    h = operands(case, be)
    got = be.reduce(case.op, case.p["skip"], case.p["a"], case.p["b"], **h)
    ref, bound = sum_bound(case, depth)
    if not np.isfinite(got):
        return Verdict(False, "sums", np.inf, f"{got!r}: a skipped entry was read")
    if case.n - case.p["skip"] <= 0:
        return Verdict(_same_bits(got, 0.0), "sums", 0.0 if _same_bits(got, 0.0) else np.inf, f"{got!r} for the identity")
    ratio = _ratio(abs(LD(got) - ref), bound)
    return Verdict(ratio <= 1.0, "sums", ratio, f"got {got!r}, ref {float(ref)!r}, |got - ref| / ((d + r) u S)")


def _judge_two_norm(case, be):
    h = operands(case, be)
    got = be.two_norm(h["x"])
    if case.n == 0:
        return Verdict(_same_bits(got, 0.0), "two_norm", 0.0, f"{got!r}")
    x = host_operand(case.n, case.opds["x"], False).view.astype(LD)
    ref = np.sqrt((x * x).sum())
    bound = ((sum_depth(case.n, 0) + 3) / 2 + 4) * LD(U) * ref
    ratio = _ratio(abs(LD(got) - ref), bound) if np.isfinite(got) else np.inf
    return Verdict(ratio <= 1.0, "two_norm", ratio, f"got {got!r}, ref {float(ref)!r}")


def _judge_minmax(case, be):
    h = operands(case, be)
    got = be.reduce(case.op, 0, 0.0, 0.0, **h)
    want = HostBackend().reduce(case.op, 0, 0.0, 0.0, **operands(case, HostBackend()))
    ok = _same_bits(got, want)
    return Verdict(ok, "exact", 0.0 if ok else np.inf, f"got {got!r}, want {want!r}")


def _judge_find(case, be):
    h = operands(case, be)
    got = np.asarray(be.find_blocking(h["x"], h["dx"], h["y"], h["dy"]))
    want = HostBackend().find_blocking(*[operands(case, HostBackend())[r] for r in ("x", "dx", "y", "dy")])
    ok = _same_bits(got, want)
    return Verdict(ok, "exact", 0.0 if ok else np.inf, f"got {got!r}, want {want!r}")


def weighted_reference(case):
    """the 2 nw bounds in long double, w in long double as well"""
    nw, wmin = case.p["nw"], LD(case.p["wmin"])
    h = operands(case, HostBackend())
    out = np.full(2 * nw, np.inf, dtype=LD)
    step = (LD(1) - wmin) / (nw - 1) if nw > 1 else LD(0)
    for j, (p, dp, cp) in enumerate((("x", "dx", "cx"), ("y", "dy", "cy"))):
        m = (h[dp].view < 0) | (h[cp].view < 0)        # sign-coherent: the only entries that can block, for every w
        pv, dv, cv = (h[r].view[m].astype(LD) for r in (p, dp, cp))
        for k in range(nw):
            s = dv + min(LD(1), wmin + step * k) * cv
            if (s < 0).any():
                out[j * nw + k] = np.min(-pv[s < 0] / s[s < 0])
    return out


def _judge_weighted(case, be):
    h = operands(case, be)
    bp, bd = be.weighted_stepbounds(*[h[r] for r in ("x", "dx", "cx", "y", "dy", "cy")], case.p["wmin"], case.p["nw"])
    got = np.concatenate([bp, bd])
    nw = case.p["nw"]
    if case.n == 0:
        return Verdict(got.size == 2 * nw and np.all(got == np.inf), "weighted", 0.0, f"{got!r}")
    ref = weighted_reference(case)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin) or not np.all(got[~fin] == np.inf) or np.signbit(got).any():
        return Verdict(False, "weighted", np.inf, f"got {got!r}, ref {ref!r}")
    ratio = _ratio(np.abs(got[fin].astype(LD) - ref[fin]), WEIGHTED_ROUNDINGS * LD(U) * ref[fin])
    return Verdict(ratio <= 1.0, "weighted", ratio, f"got {got!r}")


def _judge_bad_nw(case, be):
    h = operands(case, be)
    try:
        be.weighted_stepbounds(*[h[r] for r in ("x", "dx", "cx", "y", "dy", "cy")], case.p["wmin"], case.p["nw"])
    except be.error:
        after = judge(CASES["dot-n513"], be)      # the device (the backend) is usable afterwards
        return Verdict(after.ok, "exact", 0.0 if after.ok else np.inf, f"raised; a dot afterwards: {after!r}")
    return Verdict(False, "exact", np.inf, "no error")


def _judge_interleave(case, be):
    vs = [judge(CASES[c], be) for c in case.p["seq"]]
    return Verdict(all(v.ok for v in vs), "interleaved", max(v.ratio for v in vs), "; ".join(f"{c}: {v!r}" for c, v in zip(case.p["seq"], vs)))


_JUDGES = {"elem": _judge_elem, "sum": _judge_sum, "two_norm": _judge_two_norm, "minmax": _judge_minmax, "find": _judge_find,
           "weighted": _judge_weighted, "bad_nw": _judge_bad_nw, "interleave": _judge_interleave}


def judge(case, be, depth=None):
    """run `case` on the backend and judge the result: a Verdict (ratio: error / bound of the inexact groups, 0 or inf of the exact ones).
    depth: judge a sum by the bound of a summation tree of that depth instead of the kernel's (the CPU module's sequential sum)"""
    return _judge_sum(case, be, depth) if case.kind == "sum" else _JUDGES[case.kind](case, be)


# ---- which cases reject which mutant (asserted by tests/test_vec_reference_cpu.py) ------------------------------------------------------------
KILLERS = {
    "first_trip_only": (f"axpy-n{2 * TRIP + 2}-aligned", f"set-n{TRIP + 1}-all8", f"copy-n{TRIP + 1}-x8", f"dot-n{TRIP + 1}", f"one_norm-n{TRIP + 8}-skip7",
                        f"min-n{_NM}-at{TRIP}", f"stepbound-n{_NM}-at{TRIP}", f"find_blocking-n{_NF}-last", f"weighted-n{TRIP + 1}-x-zero"),
    "odd_tail_dropped": ("axpy-n3-aligned", "set-n257-aligned", f"copy-n{2 * TRIP + 1}-aligned", f"add_quotient-n{2 * TRIP + 3}-aligned",
                         "safe_invert-n257-aligned", "select_nonzeros-n3-aligned", f"select_nonzeros-n{2 * TRIP + 3}-aligned"),
    "last_partial_left_out": ("dot-n257", "one_norm-n513", f"sumsq_scaled-n{TRIP + 1}", "dot_shifted-n1000-skip255", f"min-n{_NM}-at{TRIP - 1}",
                              f"inf_norm-n{_NM}-at{TRIP - 1}"),
    "skip_ignored": ("dot-n1000-skip1", "one_norm-n1000-skip256", "sumsq_scaled-n1000-skip999", f"dot_shifted-n{TRIP + 8}-skip7"),
    "mask_gt_zero": ("add_quotient-n1-aligned", "divide_some-n256-all8", "select_nonzeros-n513-mask8", f"stepbound-n{_NM}-mask-minus-one-on",
                     f"stepbound-n{_NM}-mask-planted-off"),
    "float32_sum": ("dot-n2", "one_norm-n1", f"sumsq_scaled-n{TRIP + 1}", "dot_shifted-n1000-skip257", "two_norm-n1000-1e200"),
    "tie_highest_index": (f"find_blocking-n{_NF}-tie3", "interleaved-workspace"),
    "store_past_n": ("set-n3-aligned", "axpy-n257-aligned", f"set-n{2 * TRIP + 3}-aligned", "scale-n257-aligned", "gondzio_projection-n257-aligned"),
    "zero_times_y": ("set-n1-aligned", "copy-n2-aligned", f"set-n{TRIP + 1}-all8", "copy-n513-y8"),
    "masked_off_divided": ("add_quotient-n2-aligned", "add_quotient-n513-z8", "divide_some-n257-aligned", f"divide_some-n{TRIP + 1}-all8"),
}
