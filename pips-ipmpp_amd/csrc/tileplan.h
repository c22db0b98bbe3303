// Host task plans of the tiled dense LDL^T (engine.hip: tail_factor, tail_fwd / tail_bwd): which tile meets which kernel in which launch,
// as lists of TileTask.  Plain C++ like layout.h: no device call, no environment read; the engine's wrappers (TailPlan, PanelPlan, SweepRt,
// TailSingle) build here and upload.  Tested without a GPU (pips_tail_plan_probe, tests/test_tail_panel_plan_cpu.py;
// tools/asan_plan_driver.cpp states the invariants of every list).
#pragma once
#include <vector>

#include "records.h"

namespace pips {

// per block the tile-row envelope of its tail (BlockSym::tile_first): tiles left of it hold structural zeros and get no task, update
// depths start at the envelope (a banded tail costs band^2 per column instead of column^2)
using TileFirst = std::vector<const std::vector<int>*>;

// The column plan: per tile column j the lists of the launch-per-step factorisation (tail_columns) and of the launch-per-column solve
// sweeps, then the Schur SYRK; all of them ranges of h_tasks.  An update task carries its K range in TileTask::pad = k0 | k1 << 16 (tile
// columns).
struct ColumnPlan {
   int ntc_max = 0;
   std::vector<TaskList> upd, upd_diag, diag, trsm, fwd, bwd, trail, trail_next;
   TaskList schur;
   std::vector<TileTask> h_tasks;

   // Leaf batch - many blocks share every launch: left-looking (tile column j is updated once, with everything to its left: minimal
   // traffic on C) inside the envelopes `first`, with the diagonal tiles ahead and the tile columns in groups of `group`.
   //   upd_diag[j]  the last step of the diagonal tile (j, j), with column j - 1: the side stream then has a K = TILE product and the
   //                tile factorisation on the path to trsm(j), not a product as deep as the matrix done by one workgroup per block.  The
   //                tile took the columns before that inside the launch of column j - 1 (same depth as the other tiles of that launch).
   //   upd[j]       the tile columns of a group g .. g + group - 1 share the launch of column g for everything left of the group - the
   //                tiles of a tile row read the same rows of L, side by side in the task list (one XCD, one after the other) - and
   //                column g + q takes the rest, the q columns of its own group, in the launch of its own (q tiles deep).  The diagonal
   //                tiles up to the next group's first ride along the same way, so that the short launches hold no deep task.
   // trail and trail_next stay empty.
   void build_leaf(const std::vector<BlkDesc>& blks, const TileFirst& first, int group);
   // Dense root - a single block, where a left-looking column launch has at most ntr workgroups with a K as deep as the matrix: blocked
   // right-looking with panels of `panel` tile columns.  The column update upd[j] only reaches back to the start of its panel, and each
   // finished panel is applied to the whole trailing matrix in one launch of (ntr - p1)^2 / 2 tiles with K = panel * TILE: trail[j],
   // listed where j ends a panel.  lookahead: the next tile column is listed separately (trail_next[j]) so that the driver can finish it
   // first and overlap the next diagonal tile with the rest.  No envelope; upd_diag stays empty.  (panel == 0: no panels, every column
   // reaches back to the first.)
   void build_root(const std::vector<BlkDesc>& blks, int panel, bool lookahead);
};

// The update and trsm tasks of a leaf column plan (groups of P tile columns) regrouped by those groups (tail_panels): the same tasks, each
// exactly once, in lists of their own array.  With g the first column of a group and a task's launch column j = its k1 (updates) or tile
// column (trsm), a task of a tile row >= g + P belongs to the main stream -
//   deep[g / P]    the updates of launch column g (K left of the group), one launch;
//   strips[g / P]  the rest per (block, tile row) in column order - trsm(ti, g), update(ti, g + 1; K = [g, g + 1)), trsm(ti, g + 1), ... - one
//                  workgroup each of one k_tile_panel launch;
// and a task of a tile row inside the group to the chain on the side stream that finishes the group's diagonal block beside the deep launch -
//   pre[g / P]         the diagonal tile (g, g) with the columns g - P .. g - 2 (the column plan has it ride in the launch of column g - 1),
//   block_deep[g / P]  the block's tiles with everything left of the group (for (g, g): its last step, with column g - 1),
//   upd_in[j], trsm_in[j]  per column of the group the block's short updates before, and its trsm after, the diagonal tile of column j.
// No list holds two tasks of one tile, and a tile meets its tasks in the column plan's order: the sums keep their order.
struct GroupPlan {
   int P = 0, n_groups = 0;
   std::vector<TaskList> deep, pre, block_deep, strips;   // per group (strips: a range of h_strips)
   std::vector<TaskList> upd_in, trsm_in;                 // per tile column
   std::vector<TileTask> h_tasks;
   std::vector<TileStrip> h_strips;                       // (offsets into h_tasks)
   void build(const ColumnPlan& p, int P_);
};

// Single-launch tail sweeps (kernels.hip.h k_tail_rows_fwd / _bwd): one task per (block, tile row of the tail) sorted by row, where a
// block's flags start, and - with an envelope - per tile row where its sweep starts: min(i, first[i]) for the tail rows and, behind them,
// first[i] for the border tile rows (border-backward sweep)
struct SweepLists {
   std::vector<TileTask> tasks;
   std::vector<long long> flag_off, tfirst_off;   // per block
   std::vector<int> tfirst;                       // (empty without an envelope)
   long long n_flags = 0;                         // sum of ntc
   void build(const std::vector<BlkDesc>& blks, const TileFirst* first);
};

// Host side of k_tail_ldl (tailkernel.hip.h): the tasks of the column launches of a leaf column plan as ONE list in the driver's order
// (tail_columns), the kind in TileTask::blk bits 24 and up, dealt to eight lists by runs of one (block, tile row); the flags and the
// template they start from.
struct TailSingleLists {
   std::vector<TileTask> tasks;   // the eight lists back to back: list x is [xoff[x], xoff[x + 1])
   int xoff[9] = {0};
   std::vector<long long> foff;   // nblk + 1: a block's flags (ntr * ntc tiles' prog, then per tile row and per tile column one)
   std::vector<int> init;         // prog of every tile before the launch, max(n_flags, 1) entries
   long long n_flags = 0;
   int n_tasks = 0;
   void build(const ColumnPlan& p, const std::vector<BlkDesc>& blks);
};

}  // namespace pips
