"""The table of tests/border_cases.py judged on the host, without a device: the two border products in plain FP64 numpy pass the predicate on every
case in both forms and over several orders of summation, and every emulated defect is rejected by the cases listed for it (border_cases.KILLERS).

Which case rejects which defect (all of KILLERS is asserted; the cases that bear on the defect's reason):
  store_instead_of_add          every case: every initial output is non-zero (row_lengths-mult-ap1, rows1-tmult-ap1, second_trip-mult-am1 ...)
  alpha_dropped, alpha_twice    every case with alpha in {-1, 0.37, -2^-20} (alpha = 1 cannot see either)
  lane15_dropped                row_lengths and heterogeneous: rows of 16, 17, 33, 531 (20, 300, 31, 64) entries; not rows of 15 or fewer
  rows_truncated_at_16          the same batches: rows of 17 and more
  last_row_dropped              every batch whose last border row is not empty: rows1 .. rows21, row_lengths, heterogeneous, second_trip
  last_wave_dropped             border-row counts 1, 3, 5, 13, 21, 27 (heterogeneous), 74 (leaf_rows); not 4 (rows4) and 24 (row_lengths)
  second_trip_dropped           second_trip alone: rows >= 1 048 576 hold Schur columns 511 and 1023 and the last block's four leaf rows
  xoff_borderless_not_skipped   heterogeneous alone: blocks without a border before and between the bordered ones
  block0_offset_everywhere      every batch with more than one bordered block
  val_p_not_val_src             mult on every batch where the row-side order differs from the order of the values
  shared_column_addend_missing  batches where a Schur column has entries in several blocks: row_lengths, rows21, heterogeneous, leaf_rows, second_trip
  row_added_twice, colidx_row_sc_exchanged   every batch"""
import numpy as np
import pytest

from tests import border_cases as bc


@pytest.mark.parametrize("cid", bc.CASE_IDS)
def test_plain_fp64_numpy_passes_every_predicate(cid):
    case = bc.CASES[cid]
    for form in ("sum_then_alpha", "alpha_then_product"):
        for seed in range(3):
            v = bc.judge(case, bc.HostBackend(form=form, seed=seed))
            assert v.ok and v.ratio <= 1.0 and v.group == case.group, (cid, form, seed, v)
    # a backend that draws a new order for every call is held to the predicate alone, not to the bit-equality of repeated calls
    v = bc.judge(case, bc.HostBackend(seed=7, reshuffle=True))
    assert v.ok, (cid, v)


def test_repeated_calls_are_compared_bit_for_bit():
    """a backend that claims to repeat a product to the bit and does not is rejected by the sequence cases"""
    be = bc.HostBackend(seed=7, reshuffle=True)
    be.repeats = ("tmult", "mult")
    for cid in ("row_lengths-sequence", "heterogeneous_factor-before-and-after", "second_trip-sequence"):
        v = bc.judge(bc.CASES[cid], be)
        assert not v.ok and v.ratio <= 1.0 and "differ" in v.why, (cid, v)


@pytest.mark.parametrize("defect", bc.DEFECTS)
def test_every_defect_is_rejected_by_its_cases(defect):
    assert bc.KILLERS[defect], defect
    for form in ("sum_then_alpha", "alpha_then_product"):
        be = bc.HostBackend(defect=defect, form=form)
        for cid in bc.KILLERS[defect]:
            v = bc.judge(bc.CASES[cid], be)
            assert not v.ok, (defect, form, cid, v)


def test_defects_pass_where_they_are_not_reached():
    assert set(bc.KILLERS) == set(bc.DEFECTS)
    for defect, cid in bc.NOT_REACHED:
        v = bc.judge(bc.CASES[cid], bc.HostBackend(defect=defect))
        assert v.ok, (defect, cid, v)


def test_untouched_entries_must_keep_their_value():
    """NaN must stay NaN and a value its value where no product arrives; the sign of a zero is counted, not judged"""
    case = bc.CASES["heterogeneous-mult-ap1"]
    x, y0 = bc.operands(case, 0)
    good = bc.HostBackend().run(case, [(x, y0)])[0]
    n_out = bc.batch("heterogeneous").structure("mult")[3]
    un = np.flatnonzero(n_out == 0)
    assert np.isnan(y0[un]).any() and (y0[un] == 0).any() and np.isfinite(y0[un][y0[un] != 0]).any()
    assert bc.judge_step(case, 0, good)[0]
    for i, value in ((un[np.isnan(y0[un])][0], 0.0), (un[np.isfinite(y0[un]) & (y0[un] != 0)][0], np.nan), (un[np.isfinite(y0[un]) & (y0[un] != 0)][-1], 0.0)):
        bad = good.copy()
        bad[i] = value
        assert not bc.judge_step(case, 0, bad)[0], i
    flipped = good.copy()
    z = un[y0[un] == 0][0]
    flipped[z] = 0.0 if np.signbit(good[z]) else -0.0
    ok, _, _, signs = bc.judge_step(case, 0, flipped)
    assert ok and signs == 1


def test_the_bound_sees_a_relative_error_of_2_to_the_minus_40():
    """the bound is a few units of roundoff of T_i: an output entry off by 2^-40 of its value is rejected"""
    for cid in ("row_lengths-tmult-ap1", "leaf_rows-mult-a0.37", "second_trip-tmult-a0.37"):
        case = bc.CASES[cid]
        x, y0 = bc.operands(case, 0)
        got = bc.HostBackend().run(case, [(x, y0)])[0]
        n_out = bc.reference(case, 0)[2]
        i = int(np.flatnonzero(n_out > 0)[-1])
        got[i] *= 1 + 2.0 ** -40
        assert not bc.judge_step(case, 0, got)[0], cid


def test_the_table_plants_what_it_says():
    lens = lambda name, b: np.diff(bc.batch(name).blocks[b][1].rowptr)     # noqa: E731
    assert {0, 1, 15, 16, 17, 33, 531} <= set(lens("row_lengths", 0)) and bc.batch("row_lengths").S == 12
    assert lens("row_lengths", 0)[7] == lens("row_lengths", 1)[7] == 0 and lens("row_lengths", 0)[1] > 0 and lens("row_lengths", 1)[1] == 0
    assert all(lens("row_lengths", b)[c] > 0 for b in (0, 1) for c in (3, 6))
    assert [bc.batch(f"rows{r}").rows for r in (1, 3, 4, 5, 13, 21)] == [1, 3, 4, 5, 13, 21]
    for r in (1, 3, 4, 5, 13, 21):
        bt = bc.batch(f"rows{r}")
        assert all((np.diff(Bt.rowptr) > 0).all() for _, Bt in bt.blocks)       # the last wave's rows and the last row are not empty
    h = bc.batch("heterogeneous")
    assert [n for n, _ in h.blocks] == [7, 5, 11, 300, 64, 6] and [Bt is None for _, Bt in h.blocks] == [True, False, True, False, False, True]
    assert h.rows == 27 and all(lens("heterogeneous", b)[4] == 0 for b in h.bordered) and [lens("heterogeneous", b)[2] > 0 for b in h.bordered] == [False, True, False]
    assert all(lens("heterogeneous", b)[0] > 0 and lens("heterogeneous", b)[8] > 0 for b in h.bordered)
    lr = bc.batch("leaf_rows")
    n_leaf = lr.structure("mult")[3]
    assert n_leaf[7] == lr.S == 37 and not n_leaf[13:25].any() and n_leaf[:13].all()
    st = bc.batch("second_trip")
    assert st.rows == 1025 * 1024 == bc.TRIP_ROWS + 1024 and len(st.blocks) == 1025 and all(n == 4 for n in st.n)
    blk, sc, col, val = st.entries()
    assert all(2 <= np.diff(Bt.rowptr).sum() <= 4 for _, Bt in st.blocks)
    last = blk == 1024
    assert set(sc[last]) == {0, 511, 1023} and not np.isin(sc[~last], (511, 1023)).any() and (sc[~last] == 0).any()
    # zeros: the chosen output entry has several addends, all of them exactly zero, and -0.0 before the call
    for cid in (c for c in bc.CASE_IDS if c.endswith("-zeros")):
        case = bc.CASES[cid]
        x, y0 = bc.operands(case, 0)
        tgt, inp, _, n_out, read = bc.batch(case.batch_name).structure(case.steps[0].op)
        t = int(np.flatnonzero((y0 == 0) & (n_out > 0))[0])
        assert n_out[t] > 1 and np.signbit(y0[t]) and not x[inp[tgt == t]].any() and (x[read] != 0).any(), cid
    # every input entry no border entry reads holds NaN; every output entry nothing reaches holds NaN, -0.0 or a Gaussian
    for cid in bc.CASE_IDS:
        case = bc.CASES[cid]
        for k, s in enumerate(case.steps):
            if s.op != "factor":
                x, y0 = bc.operands(case, k)
                _, _, _, n_out, read = bc.batch(case.batch_name).structure(s.op)
                assert np.isnan(x[~read]).all() and np.isfinite(x[read]).all() and np.isfinite(y0[n_out > 0]).all(), cid
    assert {s.alpha for c in bc.CASES.values() for s in c.steps if s.op != "factor"} == set(bc.ALPHAS.values())
