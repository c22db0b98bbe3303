"""The regrouping of the leaf tails' column plan by groups of four tile columns (csrc/tileplan.cpp GroupPlan), on the host:
pips_tail_plan_probe lists the tasks of the column launches and the lists of the groups - deep update, the side chain of the diagonal
block, the strips of the panel launch - for the shapes of tests/tail_panel_cases.py.  Together the group lists hold every update and trsm
task of the column plan exactly once, with the same block, tile and K range; a tile meets its tasks in the column plan's order; a strip
runs in column order; no launch holds two tasks of one tile."""
import ctypes as C
from collections import Counter, defaultdict

import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import tail_panel_cases as pc

lib = pa.capi.lib
lib.pips_tail_plan_probe.restype = C.c_int
P = 4
DEEP, PRE, BLOCK_DEEP, UPD_IN, TRSM_IN, STRIP = range(6)
UPDATE, TRSM = 0, 1


def probe(case):
    blocks, S, n_head = pc.batch(case)
    nb = len(blocks)
    ip = C.POINTER(C.c_int)
    keep = []

    def arr(seq):
        a = (ip * nb)()
        for i, v in enumerate(seq):
            if v is not None:
                v = np.ascontiguousarray(v, dtype=np.int32)
                keep.append(v)
                a[i] = v.ctypes.data_as(ip)
        return a

    n = np.array([K.nrows for K, _, _ in blocks], np.int32)
    npr = np.array([p for _, p, _ in blocks], np.int32)
    args = (nb, n.ctypes.data_as(ip), npr.ctypes.data_as(ip), arr(K.rowptr for K, _, _ in blocks), arr(K.colidx for K, _, _ in blocks), S,
            arr(None if B is None else B.rowptr for _, _, B in blocks), arr(None if B is None else B.colidx for _, _, B in blocks), n_head)
    counts = np.zeros(6, np.int64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int64))
    rc = lib.pips_tail_plan_probe(*args, None, C.c_longlong(0), None, C.c_longlong(0), cp)
    assert rc == 0, lib.pips_hip_last_error().decode()
    col, grp = np.zeros((counts[0], 6), np.int32), np.zeros((counts[1], 9), np.int32)
    rc = lib.pips_tail_plan_probe(*args, col.ctypes.data_as(ip), C.c_longlong(len(col)), grp.ctypes.data_as(ip), C.c_longlong(len(grp)), cp)
    assert rc == 0, lib.pips_hip_last_error().decode()
    assert counts[0] == len(col) and counts[1] == len(grp)
    return col, grp, dict(ntc=int(counts[2]), groups=int(counts[3]), launches_col=int(counts[4]), launches_grp=int(counts[5]))


@pytest.fixture(scope="module", params=list(pc.CASES))
def plan(request):
    return (request.param,) + probe(request.param)


def task_of(row):   # (kind, block, ti, tj, k0, k1) of a row of the group lists
    return (UPDATE if row[8] else TRSM,) + tuple(int(v) for v in row[4:9])


def test_the_groups_hold_every_task_of_the_column_plan_once(plan):
    _, col, grp, info = plan
    want = Counter(tuple(int(v) for v in r) for r in col)
    got = Counter(task_of(r) for r in grp)
    assert len(col) > 0 and max(want.values()) == 1 and max(got.values()) == 1
    assert got == want
    assert all(r[4] < r[5] if r[0] == UPDATE else (r[4] == 0 and r[5] == 0) for r in col)   # a K range tells an update from a trsm
    assert info["groups"] == -(-info["ntc"] // P) and info["launches_grp"] < info["launches_col"]


def test_a_tile_meets_its_tasks_in_the_order_of_the_column_plan(plan):
    _, col, grp, _ = plan
    seq_col, seq_grp = defaultdict(list), defaultdict(list)
    for r in col:
        seq_col[tuple(r[1:4])].append(tuple(int(v) for v in r))
    for r in grp:
        seq_grp[tuple(r[4:7])].append(task_of(r))
    assert seq_col == seq_grp


def test_where_a_task_goes_and_no_launch_has_two_tasks_of_a_tile(plan):
    _, _, grp, info = plan
    launches = defaultdict(list)
    for r in grp:
        lst, g, idx = int(r[0]), int(r[1]), int(r[2])
        kind, _, ti, tj, k0, k1 = task_of(r)
        below = ti >= (g + 1) * P
        if lst == DEEP:
            assert kind == UPDATE and below and k1 == g * P
        elif lst == PRE:                   # the diagonal tile (g, g) with the columns of the group before, its own trsm done
            assert kind == UPDATE and ti == tj == g * P and (g - 1) * P <= k0 and k1 == g * P - 1
        elif lst == BLOCK_DEEP:
            assert kind == UPDATE and not below and g * P <= tj <= ti and k1 == g * P
        elif lst == UPD_IN:
            assert kind == UPDATE and not below and g * P <= k0 and k1 == idx and idx // P == g and tj >= idx
        elif lst == TRSM_IN:
            assert kind == TRSM and not below and tj == idx and idx // P == g and ti > tj
        else:
            assert lst == STRIP and below and g * P <= tj < (g + 1) * P and (kind == TRSM or g * P <= k0 < k1 <= tj)
        launches[(lst, g, idx if lst in (UPD_IN, TRSM_IN) else 0)].append((lst, g, idx) + tuple(int(v) for v in r[4:7]))
    for key, tasks in launches.items():
        if key[0] == STRIP:                # one workgroup per strip: the strips of a launch have tile rows of their own
            rows = {(t[2], t[3], t[4]) for t in tasks}
            assert len(rows) == len({(t[3], t[4]) for t in tasks}), key
        else:
            assert len({t[3:] for t in tasks}) == len(tasks), key
    assert info["groups"] == 1 + max(int(r[1]) for r in grp)


def test_a_strip_runs_in_column_order(plan):
    _, _, grp, _ = plan
    strips = defaultdict(list)
    for r in grp:
        if r[0] == STRIP:
            assert int(r[3]) == len(strips[(int(r[1]), int(r[2]))])   # positions count up from 0
            strips[(int(r[1]), int(r[2]))].append(task_of(r))
    assert strips
    for (g, _), tasks in strips.items():
        assert len({(t[1], t[2]) for t in tasks}) == 1                # one block, one tile row
        done = []                                                     # tile columns whose trsm ran
        for kind, _, ti, tj, k0, k1 in tasks:
            if kind == TRSM:
                assert not done or tj > done[-1]
                done.append(tj)
            else:   # its L(ti, k0 .. k1 - 1) is what the strip's trsm stored; the tile's own trsm is still to come
                assert set(range(k0, k1)) <= set(done) and (not done or done[-1] < tj)
        assert done and done == sorted(done)
        steps = [2 * k1 if kind == UPDATE else 2 * tj + 1 for kind, _, _, tj, _, k1 in tasks]
        assert steps == sorted(steps)


def test_the_shapes_are_what_the_cases_say():
    shapes = {c: probe(c) for c in pc.CASES}
    assert [shapes[c][2]["ntc"] for c in pc.CASES] == [6, 9, 9, 8, 9]
    assert [shapes[c][2]["groups"] for c in pc.CASES] == [2, 3, 3, 2, 3]

    def tile_rows(case):   # per block the tile rows that take a trsm
        rows = defaultdict(set)
        for r in shapes[case][0]:
            if r[0] == TRSM:
                rows[int(r[1])].add(int(r[2]))
        return rows
    assert {b: max(r) for b, r in tile_rows("a_all_tail_750").items()} == {0: 6, 1: 6}      # six tail tile rows and one of the border
    assert {b: max(r) for b, r in tile_rows("b_head_tail_1100").items()} == {0: 10, 1: 10}  # nine and two
    assert {b: max(r) for b, r in tile_rows("c_no_border").items()} == {0: 8, 1: 8}         # nine, none
    assert {b: max(r) for b, r in tile_rows("f_mixed_sizes").items()} == {0: 6, 1: 9}       # six and nine tile columns, a border row each
    # the envelope of case d: strips of a group start at different columns, and a tile inside a group's diagonal block takes no trsm
    _, grp, info = shapes["d_banded_envelope"]
    first = {(int(r[1]), int(r[2])): int(r[6]) for r in grp if r[0] == STRIP and r[3] == 0}
    assert any(len({c for (g, _), c in first.items() if g == gg}) > 1 for gg in range(info["groups"]))
    in_block = {(int(r[4]), int(r[5]), int(r[6])) for r in grp if r[0] == TRSM_IN and r[5] < info["ntc"]}
    nblk = 1 + max(b for b, _, _ in in_block)
    full = {(b, ti, tj) for b in range(nblk) for g in range(info["groups"]) for tj in range(g * P, min((g + 1) * P, info["ntc"]))
            for ti in range(tj + 1, min((g + 1) * P, info["ntc"]))}
    assert in_block < full
