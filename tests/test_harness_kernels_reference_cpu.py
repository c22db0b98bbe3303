"""The table of tests/harness_cases.py judged on the host, without a device: plain FP64 numpy passes every predicate, every named defect (a host
emulation of a plausible fault of csrc/harness.hip) is rejected by the cases listed for it, and the table holds the sizes and edges it is meant to.

Sums are tried in two orders, as tests/test_vec_reference_cpu.py does.  numpy's pairwise sum must stay inside the kernel's bound (d + r) u S at
every case.  The sequential sum is a tree of depth n - 1: it must stay inside (n - 1 + r) u S everywhere, and inside the kernel's bound wherever
its depth is no larger than the kernel's d (n <= 20).  Beyond that the kernel's bound is not the sequential sum's: over 600 001 terms of one sign
(dot_onesigned) its error grows like sqrt(n) u S, which is what the tree of the kernels avoids.

Without a device the three probe entries refuse bad arguments with PIPS_ERR_ARG (code 1) and good ones with PIPS_ERR_NO_DEVICE (code 5)."""
import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import harness_cases as hc

_HOST = hc.HostBackend()


@pytest.mark.parametrize("cid", hc.SP_IDS + hc.RED_IDS + hc.STEP_IDS)
def test_plain_fp64_numpy_passes_every_predicate(cid):
    case = hc.CASES[cid]
    v = hc.judge(case, _HOST)
    assert v.ok, (cid, v)
    if isinstance(case, hc.RedCase) and case.pred != 0:
        sums = [t for t in case.terms if t.kind in (hc.R_DOT, hc.R_DOT_SHIFTED) and t.n > 0]
        if sums:
            seq = hc.HostBackend(summation="sequential")
            m = max(t.n for t in sums)
            own = hc.judge(case, seq, depth=m - 1)
            assert own.ok, (cid, own)
            if m - 1 <= hc.sum_depth(m):
                v = hc.judge(case, seq)
                assert v.ok, (cid, v)


@pytest.mark.parametrize("defect", hc.DEFECTS)
def test_every_defect_is_rejected_by_its_cases(defect):
    assert hc.KILLERS[defect], defect
    be = hc.HostBackend(defect=defect)
    for cid in hc.KILLERS[defect]:
        v = hc.judge(hc.CASES[cid], be)
        assert not v.ok, (defect, cid, v)


def test_defects_pass_where_they_are_not_reached():
    """an emulation is the plain formula apart from its defect"""
    for defect, cid in (("later_trips_dropped", "l8-r131072-qx"), ("second_row_dropped", "l8-r9-qx"), ("first_lpr_entries_only", "l4-r1-qx"),
                        ("threshold_off_by_one", "l4-r5-qx"), ("last_long_part_dropped", "long1-qx"), ("long_rows_past_256_unfinished", "long256-rq"),
                        ("replicated_full_epilogue", "epi8-rq-lin0-both"), ("e3_ignored", "epi8-kyz-lin2-both"), ("lin2_as_lin1", "epi8-rq-e3-lin1-both"),
                        ("split_off_by_one", "epi8-rac-split70-lin0"), ("pred_ignored", "epi8-kyz-pred1"), ("tail_dropped", "dot-n262144"),
                        ("last_partial_left_out", "dot-n255"), ("mask_gt_zero", "min_masked-tiny-on"), ("stepbound_le_zero", "stepbound-n257"),
                        ("weight_ignored", "dot-n257"), ("q_ignored", "dot_w-n257"), ("neighbour_partials", "dot-n257"), ("float32_sum", "absmax_d-n257"),
                        ("second_trip_dropped", "recover-300x100x200-mixed-zero_lin0"), ("rows_beyond_min_dropped", "compl_rhs-5x3x0-mixed-mode2"),
                        ("my_rows_dropped", "rhs_reduce-2x1x7-mixed-zero_lin0"), ("mask_ignored", "recover-3x5x2-allon-zero_lin0"),
                        ("zero_lin_ignored", "rhs_reduce-3x5x2-mixed-zero_lin0"), ("upper_at_lower_offset", "reg_operator-3x5x2"),
                        ("dz_sign", "rhs_reduce-2x1x7-mixed-zero_lin0")):
        v = hc.judge(hc.CASES[cid], hc.HostBackend(defect=defect))
        assert v.ok, (defect, cid, v)


def test_the_product_table_holds_the_rows_lengths_and_lists_it_must():
    rows8 = {m["nrows"] for n, m in hc.MATS.items() if n.startswith("l8-")}
    rows4 = {m["nrows"] for n, m in hc.MATS.items() if n.startswith("l4-")}
    assert rows8 == {1, 7, 8, 9, 63, 64, 65, 131071, 131072, 131073, 300001} and rows4 == {1, 3, 4, 5, 262144, 262145, 600001}
    for name in hc.MATS:
        if hc.MATS[name]["nrows"] > 1000:
            continue
        M = hc.matrix(name)
        if name.startswith("l8-"):
            assert M.lanes == 8, name
        if name.startswith("l4-"):
            assert M.lanes == 4, name
    short7 = hc.matrix("l8-r7")
    assert short7.lanes == 8 and (short7.lens[short7.lens <= hc.CSR_LONG_ROW] < 8).sum() >= 3      # short rows below eight entries at eight lanes
    small8 = set().union(*[set(hc.matrix(f"l8-r{n}").lens) for n in (7, 8, 9, 63, 64, 65)])
    small4 = set().union(*[set(hc.matrix(f"l4-r{n}").lens) for n in (1, 3, 4, 5)])
    assert {0, 1, 7, 8, 9, 17, 511, 512, 513, 544, 8191} <= small8 and {0, 1, 3, 4, 5, 9} <= small4
    for name, lengths in (("l8-r131073", (0, 1, 7, 8, 9, 17, 511, 512, 513, 544, 8191, 262145)), ("l4-r262145", (0, 1, 3, 4, 5, 9, 511, 512, 513, 544, 8191))):
        M = hc.matrix(name)
        assert set(lengths) <= set(M.lens) and M.lanes == (8 if name[1] == "8" else 4), name
        assert M.lens[-1] <= hc.CSR_LONG_ROW       # the row alone in the last trip is a short one
        assert M.nnz < 4.3e6
    assert -(-262145 // hc.LONG_PARTS) == 8193 and -(-513 // hc.LONG_PARTS) * 31 > 513        # parts of 33 trips; a part that starts behind its row
    assert [hc.matrix(f"long{k}").long.size for k in (1, 255, 256, 257)] == [1, 255, 256, 257] and hc.matrix("l4-r5").long.size == 0
    al = hc.matrix("all-long")
    assert al.long.size == al.nrows
    for cid, c in hc.SP_CASES.items():
        assert np.array_equal(hc.matrix(c.mat).long, np.flatnonzero(hc.matrix(c.mat).lens > 512)) if hc.MATS[c.mat]["nrows"] < 1000 else True
    epi = [c for c in hc.SP_CASES.values() if c.group == "epilogues"]
    assert {c.mode for c in epi} == set(range(7)) and {c.lin for c in epi} == {0, 1, 2}
    for mode in hc.X_MODES:
        assert {(c.e3, c.lin) for c in epi if c.mode == mode} >= {(False, 0), (True, 0), (False, 1), (True, 1), (True, 2)}
    assert {c.split for c in epi if c.mode == hc.SP_RAC and c.mat == "epi8"} >= {0, 11, 70}
    assert {c.pred for c in hc.SP_CASES.values()} == {-1, 0, 1}
    # replicated ranges with rows on both sides of r0e, r1b, r1e, an empty pair, and long rows inside
    e8 = hc.matrix("epi8")
    assert e8.lens[1] > 512 and e8.lens[12] > 512 and e8.lens[69] > 512 and hc._RANGES == {"both": (3, 10, 14), "empty": (0, 5, 5), "tail": (0, 60, 70)}
    c = hc.SP_CASES["epi8-rq-e3-lin1-both"]
    e = hc.sp_operands(c)
    rep = hc.sp_rep(c, 70)
    assert rep.sum() == 7 and all(np.isnan(a[rep]).all() and np.isfinite(a[~rep]).all() for a in e)
    e = hc.sp_operands(hc.SP_CASES["epi8-rq-e3-lin2-both"])
    assert np.isfinite(e[3]).all() and np.isnan(e[0][rep]).all()


def test_the_reduction_table_holds_the_lengths_kinds_and_edges_it_must():
    single = {(c.terms[0].variant, c.terms[0].n) for c in hc.RED_CASES.values() if len(c.terms) == 1 and c.pred == -1}
    assert {(v, n) for v in hc.RED_VARIANTS for n in hc.RED_N} <= single
    assert hc.RED_N == (0, 1, 255, 256, 257, 65535, 65536, 65537, 262143, 262144, 262145, 600001) and 600001 > 3 * hc.RED_STRIDE
    kinds = {(k, "w" in r, "d" in r) for k, r, _, _ in hc.RED_VARIANTS.values()}
    assert {(hc.R_DOT, False, False), (hc.R_DOT, True, False), (hc.R_DOT_SHIFTED, False, True), (hc.R_DOT_SHIFTED, True, True),
            (hc.R_ABSMAX, False, False), (hc.R_ABSMAX, True, False), (hc.R_ABSMAX, False, True), (hc.R_MIN_MASKED, False, False),
            (hc.R_STEPBOUND, False, False)} <= kinds
    p12 = hc.RED_CASES["pack12-mixed"]
    assert len(p12.terms) == 12 and {0, 600001} <= {t.n for t in p12.terms} and len({t.kind for t in p12.terms}) == 5
    assert {c.pred for c in hc.RED_CASES.values()} == {-1, 0, 1}
    assert {0, 255, 256, 65535, 65536, 600000} <= set(hc.PLANTED) and any(3 * hc.RED_STRIDE <= i < 4 * hc.RED_STRIDE for i in hc.PLANTED)
    m = hc.vec(600001, "mask")
    assert {0.0, 1.0, 1e-300, 2.0} == set(np.abs(m)) and np.signbit(m[m == 0]).any() and (m == -1.0).any()
    t = hc.RED_CASES["stepbound-zero-b"].terms[0].opds()
    assert t["a"][7] == 0 and np.signbit(t["b"][7]) and t["b"][300] == 0 and not np.signbit(t["b"][300]) and t["a"][70000] == 0 and t["b"][70000] > 0
    assert (hc.vec(600001, "p1") > 0).all() and (hc.vec(600001, "p2") > 0).all()       # dot_onesigned: S is the sum itself
    assert hc.sum_depth(1) == 19 and hc.sum_depth(600001) == 2 + 2 + 2 + 16


def test_the_step_table_holds_the_sizes_masks_and_modes_it_must():
    assert hc.STEP_DIMS == ((1, 0, 0), (5, 3, 0), (3, 5, 2), (2, 1, 7), (300, 100, 200), (524289, 10, 17), (10, 524289, 17), (10, 17, 524289))
    for kern in hc.STEP_KERNELS:
        assert {c.dims for c in hc.STEP_CASES.values() if c.kernel == kern} == set(hc.STEP_DIMS), kern
    for kern in ("bound_residuals", "diagonals", "rhs_reduce", "recover", "compl_rhs", "masked_const"):
        assert {c.masks for c in hc.STEP_CASES.values() if c.kernel == kern} == {"mixed", "alloff", "allon"}, kern
    assert {c.flag for c in hc.STEP_CASES.values() if c.kernel == "compl_rhs"} == {0, 1, 2}
    assert {c.flag for c in hc.STEP_CASES.values() if c.kernel in ("rhs_reduce", "recover")} == {0, 1}
    assert {c.flag for c in hc.STEP_CASES.values() if c.kernel in ("masked_const", "gather")} == {0, 1}
    assert {c.variant for c in hc.STEP_CASES.values() if c.kernel == "leaf_diag"} == {"", "qdiag"}
    d = hc.step_data(300, 100, 200, "mixed")
    on, M = d["on"], d["M"]
    pairs = set(zip(on[:200], on[200:400])) | set(zip(on[400:700], on[700:]))
    assert len(pairs) == 4 and set(M[on]) == {1.0} and not M[~on].any() and np.signbit(M[~on]).any() and not np.signbit(M[~on]).all()
    assert not d["G"][~on].any() and all(np.isnan(d[k][~on]).all() for k in ("L", "rG", "rL")) and (d["Bd"][~on] == 1e150).all()
    assert all(np.isfinite(d[k]).all() for k in ("Gm", "Lm", "dGm", "dLm", "Bd"))
    ins, _, _, _ = hc.step_args(hc.STEP_CASES["rhs_reduce-300x100x200-mixed-zero_lin1"])
    assert all(np.isnan(a).all() for a in ins[:4])
    code = d["code"]
    assert (code >= 0).any() and (code == -1).any() and (code <= -2).any() and code.max() == 299 and code.min() == -201
    # the Gondzio projection meets each of its four branches
    _, ap, ad, rmin, rmax = hc.GONDZIO
    p = ((d["Gm"] + ap * d["dGm"]) * (d["Lm"] + ad * d["dLm"]))[on]
    assert (p < rmin).any() and ((p >= rmin) & (p <= rmax)).any() and ((p > rmax) & (p <= 2 * rmax)).any() and (p > 2 * rmax).any()
    # the table of rounding counts is what the reference's statements carry (dyz of k_diagonals: its k depends on the data)
    deepest = {}
    for c in hc.STEP_CASES.values():
        if c.dims == (300, 100, 200):
            ins, _, n, idx = hc.step_args(c)
            for _, _, _, k, _ in hc.step_formula(hc.LD, c, ins, hc.step_outs(c), n, idx):
                if np.ndim(k) == 0:
                    deepest[c.kernel] = max(deepest.get(c.kernel, 0), k)
    assert deepest == hc.STEP_ROUNDINGS
    for dims in hc.STEP_DIMS[-3:]:
        assert max(dims) > hc.TRIP and hc.step_data(*dims, "mixed")["nleaf"] > hc.TRIP


def test_the_entries_refuse_bad_arguments_and_a_missing_device():
    H = pa.capi.harness
    rp, ci, v = np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1)
    out = np.zeros(1)
    for kw in (dict(mode=7), dict(ci=np.array([3], np.int32)), dict(lin=3), dict(split=2), dict(mode=H.SP_KX)):
        with pytest.raises(pa.capi.PipsHipError, match=r"code 1\)"):
            H.spmv(kw.get("mode", H.SP_QX), 1, 1, rp, kw.get("ci", ci), v, np.ones(1), out, lin=kw.get("lin", 0), split=kw.get("split", 0))
    with pytest.raises(pa.capi.PipsHipError, match=r"code 1\)"):
        H.reduce([dict(kind=H.R_DOT, n=3, a=np.ones(3))], np.zeros(1))
    with pytest.raises(pa.capi.PipsHipError, match=r"code 1\)"):
        H.reduce([dict(kind=H.R_ABSMAX, n=1, a=np.ones(1))] * 13, np.zeros(13))
    with pytest.raises(pa.capi.PipsHipError, match=r"code 1\)"):
        H.step("gather", 0, 0, 0, [np.ones(2)], [np.zeros(2)], n=2, idx=[0, 2])
    with pytest.raises(pa.capi.PipsHipError, match=r"code 1\)"):
        H.step("masked_const", 0, 0, 0, [np.ones(2)], [np.zeros(1)], n=2)
    with pytest.raises(pa.capi.PipsHipError, match=r"code 1\)"):
        H.step("leaf_diag", 2, 0, 1, [np.ones(2), np.ones(1), None], [np.zeros(3)], n=3, idx=[0, -1, -4], scalars=(0, 0, 0))
    if pa.device_count() == 0:
        live = pa.capi.device_allocs_live()
        with pytest.raises(pa.capi.PipsHipError, match=r"code 5\)"):
            H.spmv(H.SP_QX, 1, 1, rp, ci, v, np.ones(1), out)
        with pytest.raises(pa.capi.PipsHipError, match=r"code 5\)"):
            H.reduce([dict(kind=H.R_ABSMAX, n=1, a=np.ones(1))], np.zeros(1))
        with pytest.raises(pa.capi.PipsHipError, match=r"code 5\)"):
            H.step("masked_const", 0, 0, 0, [np.ones(2)], [np.zeros(2)], n=2)
        assert pa.capi.device_allocs_live() == live
