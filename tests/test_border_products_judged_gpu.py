"""The border products of a leaf batch judged directly on every path: the table of tests/border_cases.py run through LeafBatch.border_tmult /
border_mult (pips_hip_batch_border_tmult_dev / _mult_dev), once on a handle with FP64 atomics and once on one with set_deterministic(True) before
analyze.  The reference (long double from the Csr objects), the derived bound |got - ref| <= gamma(n_i + 3) T_i, the rule for entries that receive
nothing and the cases are in tests/border_cases.py; tests/test_border_products_reference_cpu.py proves on the host that plain FP64 numpy passes in
shuffled orders and that the table rejects fourteen emulated defects.  Nothing is compared with the device's earlier output, the bit-identity rules
aside: two deterministic handles agree to the bit; on one handle tmult repeats to the bit in deterministic mode and mult in both modes (across other
calls and across factor()).  Results are read after LeafBatch.sync().

Mode -> kernels
  atomic          k_border_tmult (16 lanes per border row, shuffles, one FP64 atomic per non-zero row sum); k_border_mult_rows (a thread per leaf row
                  over the row-side lists of layout_border_csr)
  deterministic   k_border_rowdot / k_border_entry_products into d_bt_tmp, then k_gather_slots over g_btm / g_bm
k_border_mult, the atomic scatter form of Br x0, runs only where layout_border_csr builds no row-side lists - a batch with 2^31 or more border
entries - so no test reaches it.

Measured on an MI355X in one run, the largest error / bound per group (the case it comes from); a record of slack, not a tolerance:

    group            atomic                                   deterministic
    row_lengths      0.394  (row_lengths-mult-am1)            0.394  (row_lengths-mult-am1)
    last_wave        0.306  (rows21-mult-ap1)                 0.270  (rows21-mult-ap1)
    heterogeneous    0.363  (heterogeneous-mult-am1)          0.350  (heterogeneous-mult-ap1)
    leaf_rows        0.203  (leaf_rows-tmult-am1)             0.252  (leaf_rows-tmult-ap1)
    zeros            0.310  (heterogeneous-mult-zeros)        0.371  (heterogeneous-mult-zeros)
    sequence         0.382  (heterogeneous-sequence)          0.382  (heterogeneous-sequence)
    factor           0.271  (its one case)                    0.376
    second_trip      0.417  (second_trip-sequence)            0.417  (second_trip-sequence)

The atomic column's tmult figures move in their last digits from run to run (order of arrival).  The sign of a zero (counted, not asserted): in atomic
mode the output entry of each of the four tmult-zeros cases whose row sums are all exactly zero keeps its -0.0 (k_border_tmult adds nothing where
s == 0; the FP64 formula -0.0 + alpha 0.0 gives +0.0); in deterministic mode the gather adds its +0.0 sum there and no sign differs.  No untouched
entry changed its sign on either path.

Seeded defects, each built apart into a library of its own and this module run against it (183 tests):
  (a) k_border_mult_rows storing `t[i] = alpha * s`: 45 fail - every atomic case that calls mult (the 36 of the four alphas, the four mult-zeros, the
      three sequences, factor, second_trip-mult); deterministic mode does not run the kernel and passes.
  (b) k_border_tmult with `i_end = nrows / step * step` (rounded down to whole grid strides instead of up): 45 fail - every atomic case that calls
      tmult.  Below one stride (every small batch, rows4 included) nothing is added at all; second_trip loses exactly its rows past the first trip.
"""
import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import border_cases as bc

pytestmark = pytest.mark.gpu


class DeviceBackend:
    """border_cases' backend on the device: one analysed handle per batch, kept for the batch's cases"""

    def __init__(self, deterministic):
        self.deterministic = deterministic
        self.repeats = ("tmult", "mult") if deterministic else ("mult",)
        self._handles = {}

    def handle(self, name):
        if name not in self._handles:
            bt = bc.batch(name)
            h = pa.LeafBatch(len(bt.blocks), bt.S)
            if self.deterministic:
                h.set_deterministic(True)
            for b, (n, Bt) in enumerate(bt.blocks):
                h.set_block(b, bt.K(b), n, Bt)
            h.analyze(2)
            self._handles[name] = h
        return self._handles[name]

    def run(self, case, ops):
        import torch
        bt, h = bc.batch(case.batch_name), self.handle(case.batch_name)
        dev = [None if o is None else (torch.from_numpy(o[0]).cuda(), torch.from_numpy(o[1]).cuda()) for o in ops]
        torch.cuda.synchronize()
        for step, d in zip(case.steps, dev):      # enqueued back to back on the handle's stream
            if step.op == "factor":
                for b in range(len(bt.blocks)):
                    h.set_values(b, bt.K(b).val)
                h.factor()
            elif step.op == "tmult":
                h.border_tmult(d[0], d[1], step.alpha)
            else:
                h.border_mult(d[0], d[1], step.alpha)
        h.sync()
        return [None if d is None else d[1].cpu().numpy() for d in dev]

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles.clear()


_backends = {}
_largest = {}
_zero_signs = {}


@pytest.fixture(scope="module")
def backends():
    yield _backends
    for be in _backends.values():
        be.close()
    _backends.clear()
    for (mode, group), (ratio, cid) in sorted(_largest.items()):
        print(f"\nborder-group mode={mode} group={group} largest error/bound={ratio:.4g} ({cid})")
    for mode, cases in sorted(_zero_signs.items()):
        print(f"\nborder-zero-signs mode={mode} zeros whose sign differs from the FP64 formula's: {sum(cases.values())} in {len(cases)} cases {sorted(cases)[:6]}")


def _backend(backends, mode):
    if mode not in backends:
        backends[mode] = DeviceBackend(mode == "deterministic")
    return backends[mode]


@pytest.mark.parametrize("cid", bc.CASE_IDS)
@pytest.mark.parametrize("mode", ["atomic", "deterministic"])
def test_border_product_case(mode, cid, backends):
    case = bc.CASES[cid]
    v = bc.judge(case, _backend(backends, mode))
    print(f"border-ratio mode={mode} case={cid} group={v.group} error/bound={v.ratio:.4g} zero_signs={v.zero_signs}")
    if v.ratio >= _largest.get((mode, v.group), (0.0, None))[0]:
        _largest[mode, v.group] = (v.ratio, cid)
    if v.zero_signs:
        _zero_signs.setdefault(mode, {})[cid] = v.zero_signs
    assert v.ok and v.ratio <= 1.0, (mode, cid, v)


@pytest.mark.parametrize("name", bc.BATCH_NAMES)
def test_two_deterministic_handles_agree_to_the_bit(name, backends):
    """a second handle of its own analysis: every case of the batch, every result, the same bits"""
    first, second = _backend(backends, "deterministic"), DeviceBackend(True)
    try:
        for cid in (c for c in bc.CASE_IDS if bc.CASES[c].batch_name == name):
            case = bc.CASES[cid]
            ops = [bc.operands(case, k) for k in range(len(case.steps))]
            a, b = first.run(case, ops), second.run(case, ops)
            for k, (ra, rb) in enumerate(zip(a, b)):
                assert (ra is None and rb is None) or np.array_equal(ra.view(np.uint64), rb.view(np.uint64)), (cid, k)
    finally:
        second.close()
