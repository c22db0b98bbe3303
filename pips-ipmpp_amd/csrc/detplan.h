// Host plans of deterministic mode and of the Schur SYRK in row panels: which block goes to which of the eight group slots, the rounds
// in which the group buffers are written (a launch of a round touches at most one block per group: plain read-modify-writes are safe,
// and the blocks of a group arrive in their order), the gather lists "target -> its contributions, in fixed order".  Plain C++ like
// layout.h: no device call, no environment read; the engine plans here and uploads one line per buffer.  Tested without a GPU
// (pips_det_plan_probe, tests/test_det_plan_cpu.py).  DESIGN.md "analysis pipeline" and section 4.4.
#pragma once
#include <vector>

#include "layout.h"

namespace pips {

// A gather list: the recorded contributions (target, slot) sorted by (target, slot), then the CSR "target -> its slots"
struct SlotEntry { long long target, slot; };
struct HostGather {
   std::vector<long long> tgt, off, slots;   // off: tgt.size() + 1 entries, the last = slots.size()
};
HostGather make_gather(std::vector<SlotEntry>& e);   // (sorts e)

// ---- the two recordings of the head's scatters (Engine::build_deterministic), classified
// Schur targets of the factorisation scatter as they were recorded, unsorted, with their blocks: the group-wise list is built from them
struct ScKept {
   std::vector<SlotEntry> e;
   std::vector<int> blk;
};
struct FactorSlotPlan {
   std::vector<HostGather> levels;   // targets inside the head panels, per elimination-tree level
   HostGather tail, sc;
   ScKept kept;
};
// rec[slot] = recorded target of the factorisation scatter (-1: none; SCATTER_SC_FLAG: inside the Schur complement)
int classify_factor_slots(const std::vector<long long>& rec, long long sc_flag, const BatchLayout& lay, const std::vector<BlockSym>& sym,
                          FactorSlotPlan& out);
struct SolveSlotPlan {
   std::vector<HostGather> levels;
   HostGather tail;
};
// vrec[slot] = recorded target of the forward-substitution scatter, an entry of the permuted work vector
void classify_solve_slots(const std::vector<long long>& vrec, const BatchLayout& lay, const std::vector<BlockSym>& sym, SolveSlotPlan& out);

// ---- gather lists of the border products (k_border_rowdot): rows per Schur column, entries per leaf row.  Needs the border CSR of the
// layout: before BatchLayout::drop_uploaded
struct BorderGathers { HostGather btm, bm; };
BorderGathers border_product_gathers(const BatchLayout& lay);

// ---- the groups
// Deterministic forward sweep of the augmented factor (forward_augmented_det).  Per (block, border id): the head supernodes that hold that
// border row, in the order of the supernode array - entry = where its w factors L_b(a, 0 .. w-1) lie (the border-row arena of a front
// under the border split, else the panel) and the first of its w columns in the work vector.  And the gather of the blocks' border slots
// into the group slots of the 8 x S scratch matrix.
struct DetAugPlan {
   bool ready = false;                // false: a layout this sweep does not read - the refined path stays
   long long n_targets = 0, n_ent = 0;
   std::vector<BgEntry> ent;          // in the order of the supernode array (a supernode's border rows side by side)
   std::vector<long long> ptr, slot;  // per target: its entries [ptr[t], ptr[t + 1]) inside idx, its slot of the work vector
   std::vector<int> idx;              // per target the indices of its entries, ascending
   HostGather bslot_grp;
};
// packed blocked solves (Schur mode 2 into the sparse Schur complement): the per-row tables (layout.h PackRows) and the position tables
struct PackedTables {
   const PackRows* rows = nullptr;
   const std::vector<int>* tab = nullptr;
};
// Groups for the deterministic Schur accumulation: the global problem has eight group slots; this rank (rank of n_ranks, blocks sharded
// contiguously and evenly) fills 8 / n_ranks of them (all eight when n_ranks does not divide 8: reproducible run to run only).  Where
// the rank count divides eight the same global block sits in the same slot whatever the count: equal bits for 1, 2, 4 and 8 ranks
// (DESIGN.md 4.4).
struct DetGroupPlan {
   int n_groups = 0, first_slot = 0;
   int slots = 8;                     // group slots of this rank among the global eight (8 / n_ranks where that divides)
   // Several ranks whose count divides eight: every rank's group buffers travel to every rank (an all-reduce in which the others hold
   // zeros at these slots: exact) and ALL eight slots are added in the one fixed tree of k_reduce_groups on every rank - the sums
   // associate the same way for 1, 2, 4 and 8 ranks (pips_hip_kkt_factorize / the deterministic Lsolve), at eight times the bytes of
   // the plain reduction of the Schur complement
   bool global = false;
   std::vector<int> grp;              // block -> group: contiguous runs of ceil(nblk / slots) blocks
   // round k of the Schur SYRK handles the k-th block of every group
   std::vector<TaskList> rounds;
   std::vector<TileTask> tasks;
   // multifrontal head: the blocks of round k of k_root_assemble at [round_off[k], round_off[k + 1]) of round_blk, and the same over the
   // blocks whose border x border part k_border_schur forms (both empty without the multifrontal head; a list without blocks holds one 0)
   std::vector<int> round_blk, round_off, bb_round_blk, bb_round_off;
   HostGather sc_grp;                 // Schur targets of the head inside the group buffers
   HostGather btm_grp;                // border rows per (group, Schur column): Br^T z summed group-wise, then in the fixed tree
   HostGather pk_grp;                 // packed blocked solves: contributions per (group, position of the value array)
   DetAugPlan aug;
   bool aug_sweeps_ok = false;        // the layout's decision, taken off where the lists of the sweep cannot be built
   void drop_uploaded();              // the arrays the device now holds; the counts and offsets the launches read stay
};
// gstride: length of one group buffer (S x S, or the value array of the sparse Schur complement)
DetGroupPlan build_det_group_plan(const BatchLayout& lay, const std::vector<BlockSym>& sym, int S, int rank, int n_ranks, long long gstride,
                                  const ScKept& kept, const PackedTables& packed);

// ---- Schur SYRK in row-panel groups, so that a multi-rank root can reduce panel p while the leaves still compute p + 1 ..: group p
// holds the tile rows whose first Schur row lies in panel p.  No groups for one panel (n_panels is clamped to S / 256) or Schur mode 2.
struct ScPanelPlan {
   std::vector<int> row_begin;        // panel p = Schur rows [row_begin[p], row_begin[p + 1])
   std::vector<TaskList> groups;
   std::vector<TileTask> tasks;
};
ScPanelPlan sc_panel_plan(const BatchLayout& lay, const std::vector<BlockSym>& sym, int S, int n_panels);

}  // namespace pips
