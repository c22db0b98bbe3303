"""The host plans of deterministic mode (csrc/detplan.cpp) on the CPU: pips_det_plan_probe runs the layout of a deterministic analysis
and then the planners the engine uploads from - block -> group map, the rounds of the Schur SYRK, of k_root_assemble and of
k_border_schur_add, the gather lists of the border products and of Br^T z per group, the record of the augmented factor's forward sweep,
the Schur SYRK's row panels.  Asserted: the properties the bit-for-bit guarantees rest on - contiguous groups, every task
once, at most one block per group in a launch of a round, sorted gather lists, and lists on 2 / 4 / 8 ranks that are the one-rank lists
restricted to the rank's blocks.  The problems are those of the deterministic GPU tests' generators at 8 and 16 blocks, and one with a
border of 600 columns (several border tile rows, two row panels).  The two classifiers of the recorded scatters need a device: the GPU
tests' bit comparisons cover them."""
from collections import Counter

import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests.test_sparse_root_gpu import TwoLinkProblem
from tests.util import Problem

TILE = 128
CASES = {
    "random8": lambda: Problem(7, 8, 600, 300, 30, 20, 0.02),
    "random16": lambda: Problem(7, 16, 600, 300, 30, 20, 0.02),
    "twolink8": lambda: TwoLinkProblem(94, 8, 600, 300, 5, 16, 5.0 / 600),
    "twolink16": lambda: TwoLinkProblem(94, 16, 600, 300, 5, 16, 5.0 / 600),
    "wide8": lambda: Problem(11, 8, 600, 300, 300, 300, 0.02),       # S = 600: five border tile rows, two row panels
}
_cache = {}


def problem(case):
    if case not in _cache:
        _cache[case] = CASES[case]()
    return _cache[case]


def probe(case, mine=None, rank=0, n_ranks=1, n_panels=1):
    key = (case, None if mine is None else tuple(mine), rank, n_ranks, n_panels)
    if key not in _cache:
        prob = problem(case)
        blocks = [(prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"]) for b in (range(prob.N) if mine is None else mine)]
        _cache[key] = pa.capi.det_plan_probe(blocks, prob.S, rank, n_ranks, n_panels)
    return _cache[key]


def tile_tasks(plan):
    """every (block, ti, tj <= ti) of every block with tail tile columns and a border"""
    return Counter((b, ti, tj) for b, (ntc, nb, nb_pad, _, _, _) in enumerate(plan["blocks"].tolist()) if ntc > 0 and nb > 0
                   for ti in range(nb_pad // TILE) for tj in range(ti + 1))


def pairs(g):
    """a gather list as (target, slot) pairs in list order"""
    return list(zip(np.repeat(g["tgt"], np.diff(g["off"])).tolist(), g["slots"].tolist()))


def check_gather(g, name):
    tgt, off, slots = g["tgt"], g["off"], g["slots"]
    assert len(tgt) > 0 and len(slots) > 0, name
    assert len(off) == len(tgt) + 1 and off[0] == 0 and off[-1] == len(slots), name
    assert np.all(np.diff(tgt) > 0) and np.all(np.diff(off) > 0), name
    inside = np.ones(len(slots), bool)
    inside[off[:-1]] = False                              # (the first slot of every target has no predecessor in its target)
    assert np.all(np.diff(slots)[inside[1:]] > 0), name


@pytest.mark.parametrize("case", list(CASES))
def test_the_shapes_reach_what_the_planners_are_for(case):
    plan = probe(case)
    assert plan["schur_mode"] == 1 and plan["mf"] == 1
    # the sweeps of the augmented factor: the layout's cost rule takes them everywhere but under the 600 border columns of wide8
    assert plan["layout_aug_sweeps_ok"] == plan["aug_ready"] == plan["aug_sweeps_ok"] == (0 if case == "wide8" else 1)
    assert sum(tile_tasks(plan).values()) > 0             # a dense tail with border tiles
    if case.startswith("twolink"):                        # a multifrontal head with root fronts, and the border split
        assert plan["n_roots"] > 0 and plan["n_bb"] > 0 and np.all(plan["blocks"][:, 3] > 0) and np.all(plan["blocks"][:, 4] > 0)
    if case == "wide8":
        assert plan["blocks"][:, 2].max() == 5 * TILE


@pytest.mark.parametrize("nblk,case", [(8, "random8"), (16, "twolink16"), (5, "twolink8"), (11, "random16"), (1, "random8")])
@pytest.mark.parametrize("n_ranks", [1, 2, 3, 4, 8])
def test_group_map(case, nblk, n_ranks):
    rank = n_ranks - 1
    plan = probe(case, mine=list(range(nblk)), rank=rank, n_ranks=n_ranks)
    slots = 8 // n_ranks if 8 % n_ranks == 0 else 8
    gs = -(-nblk // slots)
    assert plan["slots"] == slots and plan["first_slot"] == (0 if slots == 8 else rank * slots)
    assert plan["global"] == (1 if n_ranks > 1 and slots < 8 else 0)
    assert plan["n_groups"] == -(-nblk // gs) <= slots
    assert plan["grp"].tolist() == [b // gs for b in range(nblk)]            # contiguous runs of gs blocks
    assert plan["grp"].max() == plan["n_groups"] - 1


@pytest.mark.parametrize("nblk,case", [(8, "random8"), (16, "random16"), (8, "twolink8"), (16, "twolink16"), (11, "twolink16"), (8, "wide8")])
@pytest.mark.parametrize("n_ranks", [1, 4])
def test_rounds_hold_every_task_once_and_one_block_per_group(case, nblk, n_ranks):
    plan = probe(case, mine=list(range(nblk)), rank=0, n_ranks=n_ranks)
    grp = plan["grp"]
    blocks = plan["blocks"]
    want = {"syrk_rounds": tile_tasks(plan),
            "root_rounds": Counter((b,) for b in range(nblk) if blocks[b, 3] > 0),
            "bb_rounds": Counter((b,) for b in range(nblk) if blocks[b, 4] > 0)}
    for name in ("syrk_rounds", "root_rounds", "bb_rounds"):
        rows = plan[name]
        if name != "syrk_rounds" and not case.startswith("twolink") and not want[name]:
            assert len(rows) == 0, name                  # (no block has root fronts / border-split batches)
            continue
        assert len(rows) > 0, name
        assert Counter(tuple(r[1:]) for r in rows.tolist()) == want[name], name
        assert max(want[name].values()) == 1
        for k in np.unique(rows[:, 0]):
            blks = np.unique(rows[rows[:, 0] == k, 1])
            assert len(np.unique(grp[blks])) == len(blks), (name, k)        # no two blocks of a launch write the same group buffer
        # the blocks of a group arrive in their order: a later round holds a later block of the group
        first_round = {}
        for k, b in zip(rows[:, 0].tolist(), rows[:, 1].tolist()):
            first_round.setdefault(b, k)
        order = sorted(first_round, key=lambda b: (grp[b], first_round[b]))
        assert order == sorted(first_round), name


@pytest.mark.parametrize("case", ["random8", "twolink8", "random16", "twolink16"])
@pytest.mark.parametrize("n_ranks", [1, 2, 4, 8])
def test_rank_independence(case, n_ranks):
    prob = problem(case)
    N, S = prob.N, prob.S
    one = probe(case)
    owner = pa.map_children_to_ranks(N, n_ranks)
    one_pairs = pairs(one["g_btm_grp"])
    assert len(one_pairs) > 0
    seen = 0
    for rank in range(n_ranks):
        mine = [int(b) for b in np.nonzero(owner == rank)[0]]
        plan = probe(case, mine=mine, rank=rank, n_ranks=n_ranks)
        # the same global block sits in the same one of the eight group slots whatever the number of ranks
        assert (plan["first_slot"] + plan["grp"]).tolist() == one["grp"][mine].tolist()
        # Br^T z per (group, Schur column): the one-rank list restricted to this rank's rows (S per block, every block has a border),
        # targets shifted by the rank's first slot, rows by its row offset; the order inside a target is kept
        row0, row1, shift = mine[0] * S, (mine[-1] + 1) * S, plan["first_slot"] * S
        want = [(t - shift, i - row0) for t, i in one_pairs if row0 <= i < row1]
        assert len(want) > 0 and pairs(plan["g_btm_grp"]) == want
        seen += len(want)
    assert seen == len(one_pairs)


@pytest.mark.parametrize("case", list(CASES))
def test_every_gather_list_is_sorted(case):
    for n_ranks, mine in ((1, None), (4, [2, 3])):
        plan = probe(case, mine=mine, rank=1 if mine else 0, n_ranks=n_ranks)
        for name in ("g_btm_grp", "g_btm", "g_bm") + (("g_bslot_grp",) if plan["aug_ready"] else ()):
            check_gather(plan[name], (case, n_ranks, name))
        prob = problem(case)
        nrows = (len(mine) if mine else prob.N) * prob.S
        # Br^T z: every non-empty border row once, by Schur column / by (group, Schur column); the border entries once by leaf row
        btm, grp_list = plan["g_btm"], plan["g_btm_grp"]
        assert sorted(btm["slots"].tolist()) == sorted(grp_list["slots"].tolist()) and len(set(btm["slots"].tolist())) == len(btm["slots"])
        assert btm["slots"].max() < nrows and np.all(btm["tgt"] == btm["slots"][btm["off"][:-1]] % prob.S)
        assert np.all(grp_list["tgt"] % prob.S == grp_list["slots"][grp_list["off"][:-1]] % prob.S)
        assert np.all(grp_list["tgt"] // prob.S == plan["grp"][grp_list["slots"][grp_list["off"][:-1]] // prob.S])
        nnz = sum(len(prob.blocks[b]["Bt"].colidx) for b in (mine if mine else range(prob.N)))
        assert sorted(plan["g_bm"]["slots"].tolist()) == list(range(nnz))


def test_no_augmented_sweep_record_where_the_layout_does_not_take_the_sweeps():
    plan = probe("wide8")
    assert plan["layout_aug_sweeps_ok"] == 0 and plan["aug_ready"] == 0 and plan["aug_sweeps_ok"] == 0 and plan["head_border_rows"] > 0
    assert plan["aug_entries"] == plan["aug_targets"] == 0
    assert all(len(plan[k]) == 0 for k in ("aug_ent", "aug_ptr", "aug_idx", "aug_slot")) and len(plan["g_bslot_grp"]["slots"]) == 0


@pytest.mark.parametrize("case", [c for c in CASES if c != "wide8"])
def test_augmented_sweep_record(case):
    plan = probe(case)
    prob = problem(case)
    ent, ptr, idx, slot = plan["aug_ent"], plan["aug_ptr"], plan["aug_idx"], plan["aug_slot"]
    n_ent, nt = len(ent), int(plan["blocks"][:, 1].sum())
    assert n_ent > 0 and n_ent == plan["aug_entries"] == plan["head_border_rows"]        # one entry per (head supernode, border row)
    assert plan["aug_targets"] == nt == len(slot) == len(ptr) - 1
    assert ptr[0] == 0 and ptr[-1] == n_ent and np.all(np.diff(ptr) >= 0)
    assert sorted(idx.tolist()) == list(range(n_ent))                                    # every entry belongs to exactly one target
    for t in range(nt):
        assert np.all(np.diff(idx[ptr[t]:ptr[t + 1]]) > 0)                               # ... whose entries are added in ascending order
    assert len(set(slot.tolist())) == nt and np.all(ent[:, 3] >= 1) and np.all(ent[:, 2] >= ent[:, 3])
    # the border slots of the work vector go group-wise into the 8 x S scratch matrix: block b's g-th slot to (group of b, bmap_b[g])
    nb = plan["blocks"][:, 1]
    assert np.array_equal(plan["blocks"][:, 5], nb) and len(plan["bmap"]) == nt
    want = sorted(zip((np.repeat(plan["grp"], nb) * prob.S + plan["bmap"]).tolist(), slot.tolist()))
    assert pairs(plan["g_bslot_grp"]) == want


@pytest.mark.parametrize("n_panels,groups", [(1, 0), (2, 2), (3, 2), (4, 2), (64, 2)])
def test_panel_plan(n_panels, groups):
    plan = probe("wide8", n_panels=n_panels)
    S = problem("wide8").S
    assert S == 600 and max(1, S // 256) == 2                # n_panels is clamped to max(1, S / 256) = 2; one panel: no groups
    assert plan["panel_groups"] == groups
    if groups == 0:
        assert len(plan["panel_tasks"]) == 0 and len(plan["panel_row_begin"]) == 0
        return
    rb = plan["panel_row_begin"]
    assert rb.tolist() == [0, 256, 600]                      # (S q / 2 rounded down to the tile)
    rows = plan["panel_tasks"]
    assert len(rows) > 0 and Counter(tuple(r[1:]) for r in rows.tolist()) == tile_tasks(plan)          # every task once
    nb = plan["blocks"][:, 1]
    base = np.concatenate([[0], np.cumsum(plan["blocks"][:, 5])])
    for g, b, ti, tj in rows.tolist():
        first = plan["bmap"][base[b] + min(ti * TILE, nb[b] - 1)]                                      # the tile row's first Schur column
        assert g == min(max(int(np.searchsorted(rb, first, side="right")) - 1, 0), groups - 1)
    assert set(rows[:, 0].tolist()) == {0, 1}


def test_no_panels_below_two_tiles_of_schur_rows():
    assert probe("random8", n_panels=4)["panel_groups"] == 0          # S = 50: max(1, S / 256) = 1
