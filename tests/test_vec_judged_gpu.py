"""The vector kernels of csrc/vecops.hip judged on every path: the table of tests/vec_cases.py run through pa.capi.vec.

The references, the predicates and their derivations are in tests/vec_cases.py; tests/test_vec_reference_cpu.py proves on the host that plain
FP64 numpy passes every predicate and that the table rejects ten emulated defects.  Every assertion here is exact equality of bits or a bound
derived from the kernel's arithmetic; nothing is compared with the device's earlier output.  Case ids are <operation>-n<length>-<what>; TRIP =
2048 * 256 = 524 288 is one trip of a capped grid.

Path -> cases
  pair path k_vec_op<OP,true>       *-aligned: n in {2, 3, 255 .. 513} one trip, even and odd (the odd tail is lane 0's); 2 TRIP and 2 TRIP + 1 a
                                    full trip (and a tail); 2 TRIP + 2 the first pair of the second trip; 2 TRIP + 3 that and a tail.  n = 1
                                    aligned goes the scalar way (n < 2).
  scalar path k_vec_op<OP,false>    *-all8 (every operand at 8 mod 16): n up to 513 one trip; TRIP + 1 one element into the second trip;
                                    2 TRIP + 1 one into the third.  *-x8 / -z8 / -mask8 / -y8: that operand alone at 8 mod 16, n = 513 and,
                                    for axpy / copy / add_quotient, TRIP + 1.
  copy, set                         every length of both paths with y full of NaN before the call: a read of y gives NaN.
  writes past the ends              every element-wise case: the sentinels before and behind y (one each at 8 mod 16, two each aligned) keep
                                    their bits.
  masks                             add_quotient / divide_some / select_nonzeros / stepbound-*-mask*: values 0.0, -0.0 (off), 1, -1, 2, 1e-300
                                    (on).  Masked-off entries: add_quotient adds inf / 0.0 nowhere, divide_some divides by 0.0 nowhere (y keeps
                                    its bits), select_nonzeros turns NaN into +0.0.  safe_invert: +-0.0, denormals, +-1e308.
  k_vec_reduce, second / third trip dot / one_norm / sumsq_scaled / dot_shifted at n = TRIP + 1 and 2 TRIP + 1; min / inf_norm / stepbound at
                                    n = TRIP + 1 with the extremum planted at 0, 255, 256, TRIP - 1 and TRIP = n - 1.
  skip_root                         the four sums at n = 1000, skip in {1, 255, 256, 257, n - 1, n, n + 5} (skip 0: the plain cases), and
                                    n = TRIP + 8, skip 7 (a second trip of one element); the skipped entries hold NaN in every operand;
                                    skip >= n gives +0.0.
  stepbound                         the mask: planted entry on behind 1e-300 and behind -1, planted entry off behind -0.0 (the runner-up, on
                                    behind -1, wins), all off (inf); x_i = 0.0 at a blocking entry (+0.0); no negative dx (inf).
  two_norm                          Gaussian times 1e200, times 1e-200, one entry of 1e300 among O(1), n = 1000 and TRIP + 1.
  k_find_index, second trip         find_blocking-n600001-tie3 (the same ratio at 300, 70 000 and 590 000 from different numbers: 300), -last
                                    (n - 1, in the second trip), -none (inf and zeros).
  k_weighted_stepbounds             nw in {1, 2, 11, 16} x wmin in {0, 0.37, 1} at n = 5 and n = TRIP + 1 (three trips of its 1024 workgroups);
                                    -x-zero (+0.0 for every k, planted in the last trip), -first-triple-unbounded; nw = 0 and 17 raise and a dot
                                    afterwards is right.
  workspace between calls           interleaved-workspace: weighted_stepbounds, dot, find_blocking, min, weighted_stepbounds, find_blocking on
                                    one thread, vectors of different lengths with different answers, each judged.
  n = 0                             every wrapper on empty tensors; reductions give their identity.

NaN in min / inf_norm / stepbound is not asserted: fmin and fmax return the other operand, so the kernels pass over a NaN entry (read from
red_combine, not measured).

Measured on an MI355X, the largest error / bound per operation over its cases (the case it comes from).  A record of slack, not a tolerance:
the assertions use the derived bounds only.

    group          operation             error / bound
    multiply-add   axpy                  0.500   (axpy-n524288-all8)             one rounding of the FMA against the r = 2 allowed
                   axpby                 0.639   (axpby-n1048578-aligned)
                   add_product           0.660   (add_product-n1048577-all8)
                   add_quotient          0.892   (add_quotient-n1048577-all8)    the quotient is not contracted: three roundings, as counted
    sums           dot                   0.013   (dot-n1000-skip999)
                   one_norm              0.046   (one_norm-n1000-skip1)
                   sumsq_scaled          0.071   (sumsq_scaled-n1)               two of the 3 + 25 roundings allowed; 0.051 at n = 2 TRIP + 1
                   dot_shifted           0.012   (dot_shifted-n512)
    two_norm                             0.045   (two_norm-n1000-1e200)
    weighted       weighted_stepbounds   0.219   (weighted-n5-nw16-wmin0.37)
    interleaved                          0.185   (its weighted_stepbounds)
    exact          everything else       every bit equal

Seeded defects, each built apart into a library of its own and this module run against it (446 cases):
  (a) the `(n & 1)` tail of the pair path dropped: 54 cases fail - every aligned case of odd n >= 3 of all 14 operations.  A first run failed 51:
      select_nonzeros kept the value of a tail entry that was on; its last entry is now off over NaN.
  (b) k_vec_reduce starting at the lane's index without `skip`: 24 cases fail - the four sums at every 0 < skip < n (n = 1000 and n = TRIP + 8).
"""
import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import vec_cases as vc

pytestmark = pytest.mark.gpu

_ELEM = {
    "axpy": lambda V, a, b, x, z, m, y: V.axpy(a, x, y),
    "axpby": lambda V, a, b, x, z, m, y: V.axpby(a, x, b, y),
    "scale": lambda V, a, b, x, z, m, y: V.scale(a, y),
    "copy": lambda V, a, b, x, z, m, y: V.copy(x, y),
    "set": lambda V, a, b, x, z, m, y: V.set(a, y),
    "mul": lambda V, a, b, x, z, m, y: V.mul(x, y),
    "div": lambda V, a, b, x, z, m, y: V.div(x, y),
    "add_product": lambda V, a, b, x, z, m, y: V.add_product(a, x, z, y),
    "add_quotient": lambda V, a, b, x, z, m, y: V.add_quotient(a, x, z, m, y),
    "divide_some": lambda V, a, b, x, z, m, y: V.divide_some(x, m, y),
    "select_nonzeros": lambda V, a, b, x, z, m, y: V.select_nonzeros(m, y),
    "safe_invert": lambda V, a, b, x, z, m, y: V.safe_invert(y),
    "add_const": lambda V, a, b, x, z, m, y: V.add_const(a, y),
    "gondzio_projection": lambda V, a, b, x, z, m, y: V.gondzio_projection(a, b, y),
}
_REDUCE = {
    "dot": lambda V, k, a, b, x, y, dx, dy, m: V.dot(x, y, skip_root=k),
    "one_norm": lambda V, k, a, b, x, y, dx, dy, m: V.one_norm(x, skip_root=k),
    "sumsq_scaled": lambda V, k, a, b, x, y, dx, dy, m: V.sumsq_scaled(x, a, skip_root=k),
    "dot_shifted": lambda V, k, a, b, x, y, dx, dy, m: V.dot_shifted(x, a, dx, y, b, dy, skip_root=k),
    "inf_norm": lambda V, k, a, b, x, y, dx, dy, m: V.inf_norm(x),
    "min": lambda V, k, a, b, x, y, dx, dy, m: V.min(x),
    "stepbound": lambda V, k, a, b, x, y, dx, dy, m: V.stepbound(x, dx, m),
}


def _v(h):
    return None if h is None else h.view


class DeviceBackend:
    """vec_cases' backend on the device: a length's base vectors are uploaded once, every call gets fresh guarded copies made on the device"""
    error = pa.capi.PipsHipError

    def __init__(self):
        self._dev = {}

    def operand(self, n, opd, mis):
        import torch
        if (n, opd.name) not in self._dev:
            if n > 4096:      # one long length at a time (the cases come sorted by length)
                for k in [k for k in self._dev if k[0] > 4096 and k[0] != n]:
                    del self._dev[k]
            self._dev[n, opd.name] = torch.from_numpy(vc.base(n, opd.name).copy()).cuda()
        g = 1 if mis else 2
        buf = torch.full((n + 2 * g,), vc.SENTINEL, dtype=torch.float64, device="cuda")
        buf[g:g + n] = self._dev[n, opd.name]
        for idx, vals in opd.patches:
            buf[torch.from_numpy(g + idx).cuda()] = torch.from_numpy(np.broadcast_to(vals, idx.shape).copy()).cuda()
        h = vc.Handle(buf, g, n, mis)
        assert n == 0 or h.view.data_ptr() % 16 == (8 if mis else 0)
        return h

    def fetch(self, h):
        return h.buf.cpu().numpy()

    def elem(self, op, a, b, x, z, mask, y):
        _ELEM[op](pa.capi.vec, a, b, _v(x), _v(z), _v(mask), _v(y))

    def reduce(self, op, skip, a, b, x, y=None, dx=None, dy=None, mask=None):
        return _REDUCE[op](pa.capi.vec, skip, a, b, _v(x), _v(y), _v(dx), _v(dy), _v(mask))

    def two_norm(self, x):
        return pa.capi.vec.two_norm(x.view)

    def find_blocking(self, x, dx, y, dy):
        return pa.capi.vec.find_blocking(x.view, dx.view, y.view, dy.view)

    def weighted_stepbounds(self, x, dx, cx, y, dy, cy, wmin, nw):
        return pa.capi.vec.weighted_stepbounds(x.view, dx.view, cx.view, y.view, dy.view, cy.view, wmin, nw)


_largest = {}


@pytest.fixture(scope="module")
def device():
    be = DeviceBackend()
    yield be
    be._dev.clear()
    for (group, op), (ratio, cid) in sorted(_largest.items()):
        print(f"\nvec-group group={group} operation={op} largest error/bound={ratio:.4g} ({cid})")


@pytest.mark.parametrize("cid", vc.CASE_IDS)
def test_vector_kernel_case(cid, device):
    case = vc.CASES[cid]
    v = vc.judge(case, device)
    print(f"vec-ratio case={cid} group={v.group} error/bound={v.ratio:.4g}")
    if v.group != "exact" and v.ratio >= _largest.get((v.group, case.op), (0.0, None))[0]:
        _largest[v.group, case.op] = (v.ratio, cid)
    assert v.ok, (cid, v)
