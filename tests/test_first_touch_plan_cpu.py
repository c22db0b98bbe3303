"""The first-touch plan of the leaf tails (csrc/layout.cpp layout_first_touch), on the host: pips_first_touch_probe hands
out the layout of a batch as the analysis decides it and the layout with the first touch refused.  Under the plan every tail column is
written once by k_tail_first_touch - from the column's init entries (entries of K and of the border), the padding diagonal and its pieces
of the root fronts' update matrices - instead of k_arena_clear + k_scatter + k_tail_pad_diag + the tail chunks of k_root_assemble.  Checked
here, without a device: the pieces are exactly the entries k_root_assemble's rule ("an entry belongs to the column of the smaller of its
two indices") sends to the tail, each once, at that rule's target and ascending by front inside a column; the init entries are exactly the
tail targets of the old scatter lists, which become -1; the deferred leaves are the simple leaves without a front above them; a NumPy
execution of the plan on integer values equals the plain scatter of the same sources; and the path is refused in deterministic mode, for a
column taller than the LDS budget, without the multifrontal head and with PIPS_HIP_TAIL_FIRST_TOUCH=0."""
import ctypes as C

import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests.util import Problem, TimeCoupledProblem, schur_problem

lib = pa.capi.lib
lib.pips_first_touch_probe.restype = C.c_int
TILE = 128
N_SECTIONS = 14
(SEC_BLK, SEC_COLBASE, SEC_INIT_OFF, SEC_INIT, SEC_PIECE_OFF, SEC_PIECE, SEC_LEAVES, SEC_KDST_OLD, SEC_KDST, SEC_BDST_OLD, SEC_BDST, SEC_ROOTS,
 SEC_ROWIDX, SEC_SIMPLE) = range(N_SECTIONS)
WIDTH = {SEC_BLK: 12, SEC_INIT: 2, SEC_PIECE: 4, SEC_ROOTS: 6, SEC_SIMPLE: 5}


def blocks_of(prob):
    return [(b["K"], prob.n_i, b["Bt"] if prob.S else None) for b in prob.blocks]


# id: builder of (problems, force_n_head); the problems' blocks form one batch.  The tail's m is forced (force_n_head = n - m): 130 and 257
# leave a padded last tile column, 384 none; the border widths sit at 0, 1, the tile (127, 129) and beyond the border split's 176 (200: the
# update matrices hold a border x border part).  The head holds fronts where it is larger than the n_i primal columns (simple leaves); in
# NO_FRONTS it is not: blocks without a root front.  NO_LEAVES: 30 entries per primal column, more than a simple leaf may have - every
# column of the head is a front, no leaf is deferred, and a tail column takes some 25 pieces.
NO_FRONTS, NO_LEAVES = "random_n600_m384_nb1", "dense_columns_no_simple_leaf"


def _random(n_i, m, nb):
    # schur_problem: every one of the nb border columns holds an entry
    prob = Problem(300, 2, n_i, n_i // 2, 0, 0, 8.0 / n_i) if nb == 0 else schur_problem(n_i, nb, 2, "full")
    return [prob], prob.n_leaf - m


def _mixed():   # two and three tile columns in one batch (force_n_head is one number: tails of 130 and of 370 rows)
    return [schur_problem(400, 129, 1, "full"), schur_problem(560, 129, 1, "full")], 600 - 130


CASES = {f"random_n{n_i + n_i // 2}_m{m}_nb{nb}": (lambda n_i=n_i, m=m, nb=nb: _random(n_i, m, nb))
         for n_i, m, nb in [(400, 130, 0), (600, 257, 1), (800, 384, 127), (600, 130, 129), (600, 257, 200), (800, 384, 200), (400, 384, 1)]}
CASES[NO_LEAVES] = lambda: ([Problem(300, 2, 400, 200, 40, 30, 0.15)], 600 - 257)
CASES["mixed_tile_columns"] = _mixed
CASES["time_coupled_border_split"] = lambda: ([TimeCoupledProblem(41, 2, 600, 300, 40, 30, 12)], 900 - 257)
_made = {}


def problems(case):
    """(problems, force_n_head) of a case, built once"""
    if case not in _made:
        _made[case] = CASES[case]()
    return _made[case]


def make(case):
    """(blocks, S, force_n_head) - blocks: [(K, n_i, Bt or None)]"""
    probs, n_head = problems(case)
    return [blk for p in probs for blk in blocks_of(p)], probs[0].S, n_head


def probe(blocks, S, n_head, deterministic=0, lds_bytes=0, free_device_bytes=0):
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
            arr(None if B is None else B.rowptr for _, _, B in blocks), arr(None if B is None else B.colidx for _, _, B in blocks), n_head,
            deterministic, C.c_longlong(lds_bytes), C.c_longlong(free_device_bytes))
    counts = np.zeros(8 + N_SECTIONS, np.int64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int64))
    rc = lib.pips_first_touch_probe(*args, None, C.c_longlong(0), cp)
    assert rc == 0, lib.pips_hip_last_error().decode()
    out = np.zeros(int(counts[7]), np.int64)
    rc = lib.pips_first_touch_probe(*args, out.ctypes.data_as(C.POINTER(C.c_longlong)), C.c_longlong(len(out)), cp)
    assert rc == 0, lib.pips_hip_last_error().decode()
    assert counts[7] == len(out) == counts[8:].sum()
    sec, at = [], 0
    for k in range(N_SECTIONS):
        a = out[at:at + int(counts[8 + k])]
        at += int(counts[8 + k])
        sec.append(a.reshape(-1, WIDTH[k]) if k in WIDTH else a)
    head = dict(first_touch=int(counts[0]), mf=int(counts[1]), tail_single=int(counts[2]), schur_mode=int(counts[3]), n_u=int(counts[4]),
                nnzK=int(counts[5]), nnzB=int(counts[6]))
    return head, sec


@pytest.fixture(scope="module", params=list(CASES))
def plan(request):
    blocks, S, n_head = make(request.param)
    head, sec = probe(blocks, S, n_head)
    assert head["first_touch"] == 1 and head["mf"] == 1 and head["tail_single"] == 0
    return request.param, head, sec


def blk_fields(sec, b):
    return dict(zip(("n", "n_head", "m", "m_pad", "nb", "ldT", "mf_split", "T_in", "k0", "nnzB", "roots", "ntc"), (int(v) for v in sec[SEC_BLK][b])))


def tail_row(d, row):
    return row - d["n_head"] if row < d["n"] else d["m_pad"] + (row - d["n"])


def rule_entries(sec):
    """(front, target, source) of every entry k_root_assemble adds into a tail: fronts in its order, b < rb, a >= b, the column of the entry
    is that of the smaller index cb = rows[b]"""
    rowidx, out = sec[SEC_ROWIDX], []
    for blk, front, r, rb, U, rows in (tuple(int(v) for v in q) for q in sec[SEC_ROOTS]):
        d = blk_fields(sec, blk)
        r = rb if d["mf_split"] == 2 else r
        for b in range(min(rb, r)):
            cb = int(rowidx[rows + b])
            for a in range(b, r):
                out.append((front, d["T_in"] + tail_row(d, int(rowidx[rows + a])) + (cb - d["n_head"]) * d["ldT"], U + b * r - b * (b - 1) // 2 + a - b))
    return out


def columns(sec):
    """(block, c, global column) of every tail column"""
    base = sec[SEC_COLBASE]
    for b in range(len(base) - 1):
        for c in range(int(base[b + 1] - base[b])):
            yield b, c, int(base[b]) + c


def plan_entries(sec):
    rowidx, out = sec[SEC_ROWIDX], []
    for b, c, g in columns(sec):
        d = blk_fields(sec, b)
        for front, u, rows, cnt in (tuple(int(v) for v in p) for p in sec[SEC_PIECE][sec[SEC_PIECE_OFF][g]:sec[SEC_PIECE_OFF][g + 1]]):
            assert int(rowidx[rows]) - d["n_head"] == c                       # the piece's first row is the column itself
            for i in range(cnt):
                out.append((front, d["T_in"] + tail_row(d, int(rowidx[rows + i])) + c * d["ldT"], u + i))
    return out


def test_the_shapes_are_what_the_cases_say(plan):
    case, _, sec = plan
    blks = [blk_fields(sec, b) for b in range(len(sec[SEC_BLK]))]
    _, S, _ = make(case)
    want_m = int(case.split("_m")[1].split("_")[0]) if case.startswith("random") else None
    for d in blks:
        assert d["m_pad"] % TILE == 0 and d["m"] <= d["m_pad"] < d["m"] + TILE and d["nb"] == S and d["ldT"] >= d["m_pad"] + d["nb"]
        if want_m:
            assert d["m"] == want_m and 600 <= d["n"] <= 1500
    assert sec[SEC_COLBASE][-1] == sum(d["m_pad"] for d in blks)
    if case == "mixed_tile_columns":
        assert [d["ntc"] for d in blks] == [2, 3] and [d["m"] for d in blks] == [130, 370]
    if case == "time_coupled_border_split":
        assert all(d["mf_split"] for d in blks)
    if "_nb200" in case:
        assert not any(d["mf_split"] for d in blks)
    assert (len(sec[SEC_ROOTS]) > 0 and len(sec[SEC_PIECE]) > 0) != (case == NO_FRONTS)
    assert len(sec[SEC_INIT]) > 0


def test_the_pieces_are_the_tail_entries_of_the_root_fronts_each_once(plan):
    _, head, sec = plan
    want, got = rule_entries(sec), plan_entries(sec)
    assert len(set(want)) == len(want) and len(set(got)) == len(got)
    assert set(got) == set(want)
    assert all(0 <= s < head["n_u"] for _, _, s in got)
    for _, _, g in columns(sec):   # ascending fronts inside a column
        fronts = sec[SEC_PIECE][sec[SEC_PIECE_OFF][g]:sec[SEC_PIECE_OFF][g + 1], 0]
        assert np.all(np.diff(fronts) > 0)
    assert sec[SEC_PIECE_OFF][0] == 0 and sec[SEC_PIECE_OFF][-1] == len(sec[SEC_PIECE])


def test_the_init_entries_are_the_tail_targets_of_the_old_scatter(plan):
    _, head, sec = plan
    for old, new, border in ((sec[SEC_KDST_OLD], sec[SEC_KDST], False), (sec[SEC_BDST_OLD], sec[SEC_BDST], True)):
        in_tail = np.zeros(len(old), bool)
        for b in range(len(sec[SEC_BLK])):
            d = blk_fields(sec, b)
            in_tail |= (old >= d["T_in"]) & (old < d["T_in"] + d["m_pad"] * d["ldT"])
        assert np.all(new[in_tail] == -1) and np.array_equal(new[~in_tail], old[~in_tail])      # head targets stay
        got = {}
        for b, c, g in columns(sec):
            d = blk_fields(sec, b)
            for row, src in sec[SEC_INIT][sec[SEC_INIT_OFF][g]:sec[SEC_INIT_OFF][g + 1]]:
                if (src < 0) == border:
                    p = int(~src if border else src)
                    assert p not in got and c // TILE * TILE <= row < d["ldT"]
                    got[p] = d["T_in"] + int(row) + c * d["ldT"]
        assert got == {int(p): int(old[p]) for p in np.nonzero(in_tail)[0]}
    assert sec[SEC_INIT_OFF][0] == 0 and sec[SEC_INIT_OFF][-1] == len(sec[SEC_INIT])


def test_the_deferred_leaves_are_the_simple_leaves_without_a_front_above_them(plan):
    case, _, sec = plan
    want = []
    for sn, blk, r, n_useg, rows in (tuple(int(v) for v in q) for q in sec[SEC_SIMPLE]):
        d = blk_fields(sec, blk)
        if n_useg == 0 and r > 0:
            assert np.all(sec[SEC_ROWIDX][rows:rows + r] >= d["n_head"])     # all its rows lie in the tail or the border
            want.append(sn)
    assert list(sec[SEC_LEAVES]) == want
    if case.startswith("random"):
        below_a_front = sum(1 for q in sec[SEC_SIMPLE] if q[3] > 0)
        assert want and (below_a_front > 0) != (case == NO_FRONTS)
    if case == NO_LEAVES:
        assert len(sec[SEC_SIMPLE]) == 0 and max(np.diff(sec[SEC_PIECE_OFF])) > 16


def test_a_numpy_execution_of_the_plan_equals_the_plain_scatter(plan):
    _, head, sec = plan
    rng = np.random.default_rng(5)
    kval, bval, U = (rng.integers(-8, 9, max(k, 1)).astype(np.float64) for k in (head["nnzK"], head["nnzB"], head["n_u"]))
    blks = [blk_fields(sec, b) for b in range(len(sec[SEC_BLK]))]
    size = max(max(d["T_in"] + d["m_pad"] * d["ldT"] for d in blks), int(sec[SEC_KDST_OLD].max()) + 1)
    border = head["schur_mode"] == 1

    def scatter(A, kdst, bdst):
        A[kdst[kdst >= 0]] = kval[:len(kdst)][kdst >= 0]
        if border and len(bdst):
            A[bdst[bdst >= 0]] = bval[:len(bdst)][bdst >= 0]

    # as before: clear, scatter, padding diagonal, the root fronts' entries one after the other
    A = np.zeros(size)
    scatter(A, sec[SEC_KDST_OLD], sec[SEC_BDST_OLD])
    for d in blks:
        t = np.arange(d["m"], d["m_pad"])
        A[d["T_in"] + t + t * d["ldT"]] = 1.0
    ent = rule_entries(sec)
    if ent:
        np.add.at(A, [t for _, t, _ in ent], U[[s for _, _, s in ent]])
    # the plan: the head's entries scattered, every tail column built on its own and written once, rows r0 .. ldT - 1
    P = np.zeros(size)
    scatter(P, sec[SEC_KDST], sec[SEC_BDST])
    written = np.zeros(size, bool)
    rowidx = sec[SEC_ROWIDX]
    for b, c, g in columns(sec):
        d = blks[b]
        r0 = c // TILE * TILE
        col = np.zeros(d["ldT"] - r0)
        for row, src in sec[SEC_INIT][sec[SEC_INIT_OFF][g]:sec[SEC_INIT_OFF][g + 1]]:
            col[row - r0] = kval[src] if src >= 0 else bval[~src]
        if c >= d["m"]:
            col[c - r0] = 1.0
        for _, u, rows, cnt in sec[SEC_PIECE][sec[SEC_PIECE_OFF][g]:sec[SEC_PIECE_OFF][g + 1]]:
            slots = np.array([tail_row(d, int(r)) - r0 for r in rowidx[rows:rows + cnt]])
            assert len(set(slots)) == cnt and slots.min() >= 0 and slots.max() < len(col)      # distinct rows inside a piece, inside the LDS column
            col[slots] += U[u:u + cnt]
        lo = d["T_in"] + c * d["ldT"] + r0
        assert not written[lo:lo + len(col)].any()
        written[lo:lo + len(col)] = True
        P[lo:lo + len(col)] = col
    assert np.array_equal(A, P)
    assert np.abs(A[written]).sum() > 0


def test_single_launch_tails_assemble_in_their_scratch_region():
    blocks, S, n_head = make("random_n900_m257_nb1")
    head, sec = probe(blocks, S, n_head, free_device_bytes=1 << 40)
    head0, sec0 = probe(blocks, S, n_head)
    assert head["first_touch"] == 1 and head["tail_single"] == 1 and head0["tail_single"] == 0
    assert all(np.array_equal(sec[k], sec0[k]) for k in range(SEC_COLBASE, SEC_LEAVES + 1))      # the plan names rows and columns, no addresses
    assert set(plan_entries(sec)) == set(rule_entries(sec))
    for b in range(len(blocks)):
        d, d0 = blk_fields(sec, b), blk_fields(sec0, b)
        assert d["T_in"] > d0["T_in"]      # a region behind the panels
        old = sec[SEC_KDST_OLD][(sec[SEC_KDST] == -1) & (sec[SEC_KDST_OLD] >= 0)]
        assert len(old) and all(any(e["T_in"] <= t < e["T_in"] + e["m_pad"] * e["ldT"] for e in (blk_fields(sec, q) for q in range(len(blocks)))) for t in old)


@pytest.mark.parametrize("how", ["deterministic", "small_budget", "no_multifrontal_head", "switched_off"])
def test_the_path_is_refused(how, monkeypatch):
    blocks, S, n_head = make("random_n900_m257_nb1")
    kw = {}
    if how == "deterministic":
        kw["deterministic"] = 1
    elif how == "small_budget":
        ldT = blk_fields(probe(blocks, S, n_head)[1], 0)["ldT"]
        assert probe(blocks, S, n_head, lds_bytes=8 * ldT)[0]["first_touch"] == 1      # the tallest column just fits
        kw["lds_bytes"] = 8 * ldT - 8
    elif how == "no_multifrontal_head":
        monkeypatch.setenv("PIPS_HIP_MF", "0")
    else:
        monkeypatch.setenv("PIPS_HIP_TAIL_FIRST_TOUCH", "0")
    head, sec = probe(blocks, S, n_head, **kw)
    assert head["first_touch"] == 0 and head["mf"] == (0 if how == "no_multifrontal_head" else 1)
    assert all(len(sec[k]) == 0 for k in range(SEC_COLBASE, SEC_LEAVES + 1))
    assert np.array_equal(sec[SEC_KDST], sec[SEC_KDST_OLD]) and np.array_equal(sec[SEC_BDST], sec[SEC_BDST_OLD])
    assert (sec[SEC_KDST_OLD] >= 0).any()
