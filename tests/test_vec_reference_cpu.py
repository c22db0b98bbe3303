"""The table of tests/vec_cases.py judged on the host, without a device and without the library: plain FP64 numpy passes every predicate, and
every mutant (a host emulation of a plausible defect of csrc/vecops.hip) is rejected by the cases listed for it.

Sums are tried in two orders.  numpy's pairwise sum must stay inside the kernel's bound (d + r) u S at every case.  The sequential sum is a tree
of depth n - skip - 1: it must stay inside (n - skip - 1 + r) u S at every case, and inside the kernel's bound wherever its depth is no larger than
the kernel's d (n - skip <= 26).  Beyond that the kernel's bound is not the sequential sum's: over 10^6 terms of one sign its error grows like
sqrt(n) u S, which is what the tree of the kernels avoids."""
import numpy as np
import pytest

from tests import vec_cases as vc

_HOST = vc.HostBackend()


@pytest.mark.parametrize("cid", vc.CASE_IDS)
def test_plain_fp64_numpy_passes_every_predicate(cid):
    case = vc.CASES[cid]
    v = vc.judge(case, _HOST)
    assert v.ok, (cid, v)
    if case.kind == "sum" and case.n - case.p["skip"] > 0:
        seq = vc.HostBackend(summation="sequential")
        m = case.n - case.p["skip"]
        own = vc.judge(case, seq, depth=m - 1)
        assert own.ok, (cid, own)
        if m - 1 <= vc.sum_depth(case.n, case.p["skip"]):
            v = vc.judge(case, seq)
            assert v.ok, (cid, v)


def test_the_table_plants_what_it_says():
    """the expectations written beside the cases hold for the FP64 reference: the planted entry is the extremum, the tie reports index 300"""
    for cid in vc.CASE_IDS:
        case = vc.CASES[cid]
        want = case.p.get("expect", "none")
        if case.kind == "minmax" and want != "none":
            assert _HOST.reduce(case.op, 0, 0.0, 0.0, **vc.operands(case, _HOST)) == want, cid
        elif case.kind == "find":
            h = vc.operands(case, _HOST)
            out = _HOST.find_blocking(h["x"], h["dx"], h["y"], h["dy"])
            if want is None:
                assert out[0] == np.inf and not out[1:].any(), cid
            elif want != "none":
                i = int(want)
                assert np.array_equal(out, [-h["x"].view[i] / h["dx"].view[i], h["x"].view[i], h["dx"].view[i], h["y"].view[i], h["dy"].view[i]]), cid
                r = np.where(h["dx"].view < 0, -h["x"].view / np.where(h["dx"].view < 0, h["dx"].view, -1.0), np.inf)
                assert int(np.argmin(r)) == i and (r == r[i]).sum() == (3 if "tie3" in cid else 1), cid
        elif case.kind == "weighted" and want != "none":
            h = vc.operands(case, _HOST)
            bp, bd = _HOST.weighted_stepbounds(*[h[r] for r in ("x", "dx", "cx", "y", "dy", "cy")], case.p["wmin"], case.p["nw"])
            assert np.isfinite(bd).all(), cid
            assert (bp == np.inf).all() if want == "inf-finite" else (not bp.any() and not np.signbit(bp).any()), cid


def test_masked_cases_hold_zero_divisors_behind_the_mask():
    for n in (2, 513, vc.TRIP + 1):
        off = vc.base(n, "mask") == 0
        assert off.any() and (~off).any()
        assert (vc.base(n, "zq")[off] == 0).all() and np.isinf(vc.base(n, "xq")[off]).all() and (vc.base(n, "xd")[off] == 0).all()
        assert np.isnan(vc.base(n, "ysel")[off]).all() and np.isfinite(vc.base(n, "ysel")[~off]).all()
    assert set(np.abs(vc.base(513, "mask"))) == {0.0, 1.0, 2.0, 1e-300} and np.signbit(vc.base(513, "mask")[vc.base(513, "mask") == 0]).any()


def test_every_operation_sees_the_lengths_and_alignments_it_must():
    """n = 1, n = 2, an even and an odd length of one trip, one length one unit past a trip on each path, every alignment configuration"""
    for op, (roles, _, _) in vc.ELEM.items():
        mine = [c for c in vc.CASES.values() if c.kind == "elem" and c.op == op]
        pair = {c.n for c in mine if not c.mis}
        scalar = {c.n for c in mine if c.mis == frozenset(roles)}
        assert {1, 2, 256, 257} <= pair and {1, 2, 256, 257} <= scalar, op
        assert pair & {2 * vc.TRIP + 2, 2 * vc.TRIP + 3} and vc.TRIP + 1 in scalar and 2 * vc.TRIP + 1 in scalar, op
        if len(roles) > 1:
            assert {tuple(c.mis) for c in mine if len(c.mis) == 1} == {(r,) for r in roles}, op
    for op in vc.SUMS:
        mine = [c for c in vc.CASES.values() if c.kind == "sum" and c.op == op]
        assert {1, 2, 256, 257, vc.TRIP + 1, 2 * vc.TRIP + 1} <= {c.n for c in mine if c.p["skip"] == 0}, op
        assert {0, 1, 255, 256, 257, 999, 1000, 1005} <= {c.p["skip"] for c in mine if c.n == 1000} | {0}, op
        assert any(c.n == vc.TRIP + 8 and c.p["skip"] == 7 for c in mine), op


@pytest.mark.parametrize("defect", vc.DEFECTS)
def test_every_mutant_is_rejected_by_its_cases(defect):
    assert vc.KILLERS[defect], defect
    be = vc.HostBackend(defect=defect)
    for cid in vc.KILLERS[defect]:
        v = vc.judge(vc.CASES[cid], be)
        assert not v.ok, (defect, cid, v)


def test_mutants_pass_where_their_defect_is_not_reached():
    """the emulation is the plain formula apart from its defect: a mutant passes cases that do not reach it"""
    for defect, cid in (("odd_tail_dropped", "axpy-n256-aligned"), ("odd_tail_dropped", "axpy-n257-all8"), ("store_past_n", "set-n257-all8"),
                        ("first_trip_only", "axpy-n513-aligned"), ("skip_ignored", "dot-n513"), ("mask_gt_zero", "axpy-n513-aligned"),
                        ("tie_highest_index", "find_blocking-n1000"), ("last_partial_left_out", "axpy-n257-aligned"),
                        ("zero_times_y", "axpy-n3-aligned"), ("masked_off_divided", "select_nonzeros-n513-mask8"), ("float32_sum", "min-n513")):
        v = vc.judge(vc.CASES[cid], vc.HostBackend(defect=defect))
        assert v.ok, (defect, cid, v)
