"""The kernels of csrc/harness.hip judged directly: the table of tests/harness_cases.py run through pa.capi.harness (pips_ipm_probe_spmv,
pips_ipm_probe_reduce, pips_ipm_probe_step - the handle's own launch code on arrays given here), one test per group.

The references, the predicates and their derivations are in tests/harness_cases.py; tests/test_harness_kernels_reference_cpu.py proves on the
host that plain FP64 numpy passes every predicate and that the table rejects 26 emulated defects.  Every assertion here is equality of bits or a
bound derived from the kernel's arithmetic; nothing is compared with the device's earlier output.  A test runs every case of its group, prints
each ratio error / bound and fails with the list of the cases that failed.

Group -> what it reaches (the lane counts and long-row counts are the ones the probe reports, asserted case by case)
  products_8_lanes   k_spmv<MODE, 8>: 1, 7, 8, 9, 63, 64, 65 rows (one workgroup, lane groups without a row, at 65 rows a second row of the pair);
                     131 071 / 131 072 / 131 073 rows (the last: one short row alone in a second trip of the capped grid), 300 001 (third
                     trip).  Row lengths 0, 1, 7, 8, 9, 17, 511, 512 beside the long ones; l8-r7: short rows below eight entries at eight lanes.
  products_4_lanes   k_spmv<MODE, 4>: 1, 3, 4, 5 rows; 262 144 / 262 145 / 600 001 rows; lengths 0, 1, 3, 4, 5, 9, 511, 512.
  long_rows          k_spmv_long_part / k_spmv_long_finish under SP_QX, SP_RAC (J) and SP_RQ (J^T): 0, 1, 255, 256, 257 long rows (257: the
                     finishing kernel's second workgroup), every row long; rows of 513 (parts of 17: part 31 starts behind the row), 544 (every
                     part full), 8 191, 262 145 (parts of 8 193: 33 trips inside a part); pred 0 / 1 on the pair.
  epilogues          all seven modes on an eight-lane and a four-lane matrix; e3 NULL / given; lin 0, 1, 2 with replicated ranges [0, 3) and
                     [10, 14) (long rows 1 and 12 inside), empty ranges, and [60, 70) up to the last (long) row; SP_RAC split 0, 11, nrows;
                     pred 0 (out keeps its bits) and 1 (the bits of no predicate).  Replicated rows: NaN in what they must not read.
  reductions         k_multi_reduce / k_multi_reduce_final: every kind and variant at n = 0 .. 600 001 (the unrolled loop and its tail);
                     packs of 12 of mixed kinds and lengths (n = 0 beside 600 001) in both orders, one term at positions 0, 5, 11; pred 0 / 1;
                     extrema planted at 0, 255, 256, 65 535, 65 536, inside the unrolled zone and at n - 1; masks 0.0, -0.0, 1e-300, -1; step
                     bounds beside b = +-0.0.
  step_kernels       the nine element-wise kernels at (nx, my, mz) with each of the three the largest, one entry into a second trip (524 289),
                     mz = 0, my = 0; masks mixed / all off / all on with -0.0 as off; zero_lin with NaN residuals; the three k_compl_rhs modes.
  probe = handle     pips_ipm_mult, its transpose and pips_ipm_hessian_mult give the bits of the probe on the layout's arrays.

NaN in an R_ABSMAX operand (reported by test_reductions, not asserted; nothing changes here): fabs(NaN) is NaN and fmax returns its other
operand, so the kernel passes over the entry - a vector of 1000 Gaussians with NaN at 0, 500 and 999 gives the maximum of the other 997, and a
vector of NaN alone gives 0.0.  The reference's DenseVector<double>::inf_norm is fabs(v[idamax(v) - 1]) (DenseVector.cpp:256-262): what it
returns is the BLAS's choice - the reference idamax keeps its first candidate when no comparison succeeds, i.e. NaN for a NaN at entry 0 and
otherwise the maximum of the entries it could compare; its generic template (:239-253, "if (!(temp <= norm)) norm = temp") takes the NaN and
then replaces it by the next entry, forgetting the maximum so far.  Read from the reference's source, not run.

Measured on an MI355X, the largest error / bound per group (the case it comes from).  A record of slack, not a tolerance:

    group              error / bound
    products_8_lanes   0.779   (l8-r131073-qx)            rows of a few entries under SP_QX: len u sum|v in| is all there is
    products_4_lanes   0.9965  (l4-r600001-qx)            rows of ONE entry: one rounding of the product against len = 1
    long_rows          0.819   (long256-qx)               its short rows; where every row is long (all-long-*): 0.001
    epilogues          0.877   (epi4-qx-lin2-empty)
    reductions         0.056   (dot_onesigned-n255)       sums; the extrema are equal to the bit
    step_kernels       1.000   (recover-524289x10x17-mixed-zero_lin0)   dv = dx - rG: one rounding against k = 1 among 524 289 entries (0.99996)
"""
import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import harness_cases as hc

pytestmark = pytest.mark.gpu


class DeviceBackend:
    """harness_cases' backend on the device: the probe entries through pa.capi.harness"""

    def spmv(self, mode, nrows, ncols, rp, ci, v, x, out, **kw):
        return pa.capi.harness.spmv(mode, nrows, ncols, rp, ci, v, x, out, **kw)

    def reduce(self, terms, out, pred=-1):
        return pa.capi.harness.reduce(terms, out, pred=pred)

    def step(self, kernel, nx, my, mz, ins, outs, n=0, flag=0, scalars=(), idx=None, case=None):
        pa.capi.harness.step(kernel, nx, my, mz, ins, outs, n=n, flag=flag, scalars=scalars, idx=idx)


def _run_group(ids, group):
    be = DeviceBackend()
    live = pa.capi.device_allocs_live()
    failed, worst = [], (0.0, None)
    for cid in ids:
        v = hc.judge(hc.CASES[cid], be)
        print(f"harness-ratio case={cid} group={group} error/bound={v.ratio:.4g}")
        if not v.ok:
            failed.append((cid, v))
        elif v.ratio >= worst[0]:
            worst = (v.ratio, cid)
    print(f"harness-group group={group} cases={len(ids)} largest error/bound={worst[0]:.4g} ({worst[1]})")
    assert pa.capi.device_allocs_live() == live, "a probe entry left an allocation behind"
    assert ids and not failed, failed


@pytest.mark.parametrize("group", ["products_8_lanes", "products_4_lanes", "long_rows", "epilogues"])
def test_products(group):
    _run_group([c for c in hc.SP_IDS if hc.SP_CASES[c].group == group], group)


def test_reductions():
    _run_group(hc.RED_IDS, "reductions")
    # NaN in R_ABSMAX: reported, not asserted (module docstring)
    a = hc.vec(1000, "g1").copy()
    a[[0, 500, 999]] = np.nan
    out = np.zeros(2)
    pa.capi.harness.reduce([dict(kind=hc.R_ABSMAX, n=1000, a=a), dict(kind=hc.R_ABSMAX, n=1000, a=np.full(1000, np.nan))], out)
    print(f"harness-nan R_ABSMAX with NaN at 0, 500, 999: {out[0]!r} (the maximum of the others: {np.nanmax(np.abs(a))!r}); all NaN: {out[1]!r}")


def test_step_kernels():
    _run_group(hc.STEP_IDS, "step_kernels")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_probe_runs_what_the_handle_runs():
    """pips_ipm_mult is SP_KYZ / SP_KX with zero e0, e1 on the handle's J / J^T, pips_ipm_hessian_mult SP_QX on its Q: the probe, given the
    layout's arrays, returns the same bits (sums in a fixed order, no atomics), chooses its long rows as the layout does"""
    from tests.general_lp_gen import random_block_lp
    from tests.qp_ref import long_row_case
    H = pa.capi.harness
    blocks = random_block_lp(300, 4, 7, 30, 9, 5, 3, 2)
    lay = pa.ipm_layout_probe(blocks)
    nx, nr = lay["nx"], lay["my"] + lay["mz"]
    rng = np.random.default_rng(300)
    x, yz = rng.standard_normal(nx), rng.standard_normal(nr)
    ipm = pa.GeneralIpmSolver(blocks)
    for tr, pre, mode, vin, nrows, ncols in ((False, "J", H.SP_KYZ, x, nr, nx), (True, "Jt", H.SP_KX, yz, nx, nr)):
        out = np.full(nrows, hc.SENTINEL)
        lanes, long_rows = H.spmv(mode, nrows, ncols, lay[pre + "_rp"], lay[pre + "_ci"], lay[pre + "_v"], vin, out, e0=np.zeros(nrows), e1=np.zeros(nrows))
        want = ipm.mult(vin, transposed=tr)
        print(f"harness-handle {pre}: {nrows} rows, {lanes} lanes per row, {long_rows.size} long rows")
        assert np.array_equal(_bits(out), _bits(want)), pre
        assert np.array_equal(long_rows, lay[pre + "_long"]), pre
    del ipm
    blocks, hs, _ = long_row_case()
    lay = pa.ipm_layout_probe(blocks, hs)
    nx = lay["nx"]
    x = rng.standard_normal(nx)
    ipm = pa.GeneralIpmSolver(blocks, hessians=hs)
    out = np.full(nx, hc.SENTINEL)
    lanes, long_rows = H.spmv(H.SP_QX, nx, nx, lay["Q_rp"], lay["Q_ci"], lay["Q_v"], x, out)
    print(f"harness-handle Q: {nx} rows, {lanes} lanes per row, {long_rows.size} long rows")
    assert long_rows.size == 520 and np.array_equal(long_rows, lay["Q_long"])
    assert np.array_equal(_bits(out), _bits(ipm.hessian_mult(x)))
