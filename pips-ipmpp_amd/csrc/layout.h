// Host pass of a batch analysis: from the blocks' symbolic analyses (symbolic.cpp) to everything the engine uploads or keeps -
// offsets, supernode order, launch lists, index arrays.  Plain C++: no device call, and the pass itself reads no environment (the switches
// come in as LayoutKnobs; read_layout_knobs fills them), so it runs and is tested without a GPU (pips_layout_probe, tests/test_layout_cpu.py).
// Pipeline (DESIGN.md "analysis pipeline"): analyze_symbolic -> build_batch_layout -> Engine::analyze uploads -> task plans.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "common.h"
#include "records.h"

namespace pips {

struct BlockInput {
   int n = 0, n_primal = -1;
   std::vector<int> krow, kcol;
   std::vector<int> btrow, btcol;  // S+1 / nnz ; empty if no border
   std::vector<double> btval;
};

// The head solve sweeps use the register-lean "chain" kernels (k_head_fwd_chain / k_head_bwd_chain: all loads up front, partial sums in
// registers, one LDS transpose) at every launch size (round 2 drew a line at 1024 waves; with supernodes capped at 16 columns they win
// everywhere: configs[3] share, leaf solve 13.5 -> 11.6 ms).  Deterministic mode takes k_head_fwd (it writes slots) forward, the chain
// kernel backward.
struct LevelRange {
   int simple_begin, simple_cnt, small_begin, small_cnt, large_begin, large_cnt;
   int small_lds = 0, large_lds = 0;   // doubles of LDS the widest L21 panel of the class needs (r * (w | 1)), capped at the kernel's capacity
};

// Multifrontal head: one launch per (level, front class); class = (workgroup size, width bound) of k_front.
struct MfLaunch { int level, cls, begin, cnt, lds_doubles; };
constexpr long long MF_LDS_MAX = 20352;   // doubles of LDS a front launch may ask for: 159 KB of the 160

// One definition of "simple leaf": one thread each on the device (k_head_factor_simple)
inline bool is_simple(const HeadSupernode& s) { return s.w == 1 && s.r <= SIMPLE_RMAX && s.level == 0; }
// rows a front holds below its pivot block: all, or (fronts on the rows of K only, BlockSym::mf_konly) its rows of K
inline int mf_rows(const BlockSym& bs, const HeadSupernode& s) { return bs.mf_konly ? s.rb : s.r; }

// LDS need of the front of supernode l, in doubles: the packed panel (or the aligned copy of L21, whichever is larger), the packed update
// matrix, and - as ints, two per double - the children's position lists and the leaf part of the front record plus the leaves' values
// (common.h "Front record").  The update matrix stays in device memory where panel + update + 8 doubles of slack exceed the budget.
struct FrontLds {
   long long panel, upd, extra;
   bool resident(long long lds_budget) const { return panel + upd + 8 <= lds_budget; }
   long long doubles(long long lds_budget) const { return panel + (resident(lds_budget) ? upd : 0) + 8 + extra; }
};
FrontLds front_lds(const BlockSym& bs, int l);
// kernel variant of k_front: 0 .. 5 = (rows <= 64 | more) x (width <= 16 | more), 6 / 7 the device-memory variants (rows <= 256 | more)
int mf_class(const BlockSym& bs, int l, long long lds_budget);

// k_border_schur's LDS need, from the symbolic analysis alone: staging area, most row positions of a batch, widest border.  Evaluated
// at analyze time: a block set whose border rows do not fit (nb near 176 under wide fronts that are nearly all border rows) goes back to
// whole update matrices there instead of failing in every factor()
struct BbPlanSize { int stage = 3072, poscap = 0, nbmax = 0; bool two_per_cu = false; };
BbPlanSize bb_plan_size(const std::vector<BlockSym>& sym);
size_t bb_lds_bytes(const BbPlanSize& z);
inline bool bb_fits(const BbPlanSize& z) { return bb_lds_bytes(z) <= 160 * 1024 && z.poscap <= 4 * 512 && z.stage <= 2 * 6 * 512; }

// k_tail_first_touch keeps one tail column (8 ldT bytes) per wave in LDS: half of a compute unit's 160 KB, so that at least two
// columns are resident per compute unit
constexpr long long FT_LDS_BUDGET = 80 * 1024;
constexpr long long FT_LDS_MAX = 160 * 1024;   // what a workgroup can have at all: a larger budget (LayoutKnobs::ft_lds_bytes) counts as this

// Every switch the layout depends on, as values (read_layout_knobs).  A switch with "-1: not set" takes the layout's own rule.
struct LayoutKnobs {
   bool deterministic = false;
   int schur_mode = 0;          // requested: 0 auto, 1 augmented partial factorisation, 2 blocked solves
   bool mf_wanted = true;       // multifrontal head (taken if every block's fronts fit)
   long long mf_lds_doubles = 19200;   // LDS budget of one front (AnalyzeOptions::mf_lds_doubles)
   int spine = -1;              // 0: no spine kernels
   int tail_single = -1;        // 0 / 1 forces one side of the single-launch tail factorisation
   int border_backward = -1, aug_sweeps = -1;   // 0 / 1 instead of the cost rules of the sweeps of the augmented factor
   bool sweep_launches = false; // the launch-per-tile-column solve sweeps are selected (the single-launch sweeps are off)
   long long free_device_bytes = 0;   // the one runtime input: free device memory, decides tail_single
   int tail_first_touch = -1;   // 0: the tails are cleared and added to (k_arena_clear, k_root_assemble) whatever the batch looks like
   long long ft_lds_bytes = FT_LDS_BUDGET;   // LDS a column of k_tail_first_touch may take (tests: a small value forces the fallback)
   // settled by analyze_symbolic
   bool mf = false;             // multifrontal head taken
   int schur_mode_eff = 1;
};

// What one analyze() call reads from the environment: the layout's switches, and the two of the single-launch tail factorisation
struct AnalyzeKnobs : LayoutKnobs {
   long long tail_poll_limit = 0;
   int tail_diag_blocked = 1;
};
// the settings of an engine that an analysis reads beside the environment
struct EngineSettings { int sn_width; bool deterministic; int schur_mode; };
// Every switch an analysis depends on, read in one place at every analyze() call through the accessors of knobs.h (DESIGN.md section 10;
// tests set them before analysing).  e == nullptr: the CPU probes - no engine settings, no deterministic mode.
void read_layout_knobs(const EngineSettings* e, AnalyzeOptions& opt, AnalyzeKnobs& knobs);
// sums and maxima over the blocks' symbolic analyses: the first 13 entries of pips_hip_batch_info (include/pips_hip.h)
void sym_info(const std::vector<BlockSym>& sym, int64_t* what, int n_what);

// Every block's non-empty border columns from the border's row pointers alone - the column sets the sparse root's pattern, its position
// tables and the packed blocked solves (Schur mode 2 with the sparse root: right-hand side q carries, in every block, that block's q-th
// column) are built on.  Equal to BlockSym::bmap where the border took part in the symbolic analysis; filled in Schur mode 2 as well.
struct SchurPack {
   std::vector<int> nb;          // per block: non-empty border columns
   std::vector<long long> off;   // nblk + 1 offsets into cols
   std::vector<int> cols;        // the blocks' column sets (Schur column ids), ascending, block after block
   int nb_max = 0;               // right-hand sides of the packed solves
   const int* block_cols(int b) const { return cols.data() + off[b]; }
};
// one block: local_of_row[s] = position of Schur column s among the block's non-empty columns, -1 for an empty one (bt_rowptr == nullptr:
// no border, all -1); returns their number
int schur_pack_block(int S, const int* bt_rowptr, int* local_of_row);
void build_schur_pack(const std::vector<BlockInput>& in, int S, SchurPack& out);
// The per-row tables of the packed blocked solves, per row of the global border CSR (S rows per block with a border): la = the row's
// local index in its block, -1 for an empty row; tabrow = where its row of the block's nb x nb position table starts (off[b]: the
// block's table inside the tab_size entries of all tables; PIPS_ERR_ARG where a table would end behind them)
struct PackRows {
   std::vector<int> la;
   std::vector<long long> tabrow;
};
int schur_pack_rows(const std::vector<BlockInput>& in, int S, const std::vector<long long>& off, long long tab_size, PackRows& out);

// Everything Engine::analyze() computes on the host.  The engine keeps this record; the arrays under "uploaded, then dropped" are
// cleared after their upload (drop_uploaded).
struct BatchLayout {
   bool mf = false;            // multifrontal head (k_front): update matrices go from child to parent front, no FP64 atomics in the head
   int schur_mode_eff = 1;     // what the analysis settled on
   std::vector<BlkDesc> h_blks;
   std::vector<long long> kptr;     // nblk+1 offsets into kval
   std::vector<long long> x_off;    // nblk+1 offsets into flat vectors
   long long n_total = 0, nnzK_total = 0, nnzB_total = 0, arena_total = 0, xw_total = 0, bt_rows_total = 0, uarena_total = 0;
   long long winv_total = 0, dtail_total = 0;
   long long mfU_total = 0, mfLV_total = 0;
   int nsn_total = 0;
   std::vector<SnDesc> h_sns;       // supernodes sorted by (level, class, LDS need)
   std::vector<LevelRange> levels;
   std::vector<LevelRange> levels_top;   // the spine's levels, for the multi-vector sweeps (which are level-scheduled throughout)
   std::vector<MfLaunch> mf_launches;
   int spine_total = 0, n_levels_all = 0;   // supernodes handled by the per-block spine kernels; tree height before the cut
   int head_wcap = HEAD_WMAX;   // widest head supernode of this analysis (picks the register-lean variants of the chain kernels)
   long long slots_total = 0, vslots_total = 0;   // deterministic mode: contribution slots of the factorisation / forward substitution
   std::vector<int> h_roots, h_root_off;    // fronts without a head parent, per block (k_root_assemble)
   int n_roots = 0;
   // border split (k_border_schur): batches of supernodes with border rows, block after block
   std::vector<BbBatch> h_bb_batches;
   std::vector<BbMeta> h_bb_meta;
   std::vector<int> h_bb_pos, h_bb_off;     // compressed border ids of the staged rows; batches of block b: [h_bb_off[b], h_bb_off[b + 1])
   int n_bb = 0;
   long long bb_doubles = 0;            // doubles of the border-row arena (behind the panels inside the arena)
   int bb_stage = 3072, bb_nbmax = 0, bb_poscap = 0;
   bool bb_two_per_cu = false;   // k_border_schur: staging area sized for two workgroups per compute unit (bb_plan_size)
   // fronts on the rows of K only (BlockSym::mf_konly): records and lists of k_border_rows / k_border_tail
   bool kb_any = false;
   std::vector<int> h_kb_rec, h_kb_list, h_kb_tail;
   std::vector<long long> h_kb_off;     // per supernode (sorted id): offset of its record, -1 none
   std::vector<int> kb_level_off;       // offsets into h_kb_list per level (size levels + 1)
   std::vector<int> kb_level_pairs, kb_level_lds;   // per level: most pairs of one front, bytes of the largest border-row block (LDS of k_border_rows)
   int n_kb_tail = 0;
   std::vector<int> h_spine, h_spine_off;
   bool tail_single = false;    // the tails as one launch: they are then assembled in a scratch region (BlkDesc::T_in)
   long long tail_scratch = 0;  // doubles of that region, behind the panels and the border-row arena
   // First-touch plan of the tails (layout_first_touch): every tail column c < m_pad is written once, assembled, by one wave of
   // k_tail_first_touch instead of being cleared (k_arena_clear) and added to (k_scatter, k_tail_pad_diag, k_root_assemble).  Column c of
   // block b is global column ft_colbase[b] + c; its init entries (entries of K and of the border whose scatter target lies in it; their
   // targets in h_kdst / h_bdst are -1 then) and its front pieces (the (front, b) pairs with b < rb whose row b is column c - what
   // k_root_assemble's rule "the column of an entry is the smaller of its two indices" assigns to it - in ascending front order) lie at
   // [off[g], off[g + 1]).  ft_leaves: the simple leaves without a front above them; their rank-one products into the tail and the
   // Schur complement wait until the columns are written (k_leaf_products).
   bool tail_first_touch = false;
   int ft_ld_max = 0, ft_cols_max = 0;   // tallest column (max ldT: the kernel's LDS) and most columns of a block (max m_pad)
   int n_ft_leaves = 0;
   std::vector<long long> h_ft_colbase;            // nblk + 1
   std::vector<int> h_ft_init_off, h_ft_piece_off; // columns + 1 each
   std::vector<FtInit> h_ft_init;
   std::vector<FtPiece> h_ft_piece;
   std::vector<int> h_ft_leaves;
   std::vector<int> schur_cols;   // non-empty Schur columns (any block), ascending
   std::vector<int> h_bt_rowsc, h_bt_rownnz, h_bt_rowblk;   // per row of the global border CSR: Schur column, entries, block
   int n_flong = 0;
   long long lf_rows = 0, lf_entries = 0;
   int n_lb = 0, nb_pad_max = 0;
   // whether the border-backward sweep / both sweeps of the augmented factor pay, and the two entry counts the rules rest on
   bool border_backward_ok = false, aug_sweeps_ok = false;
   double fwd_entries = 0.0, border_entries = 0.0;
   // ---- uploaded, then dropped
   std::vector<int> h_rowidx, h_sncol, h_bmap, h_perm, h_upd, h_mfint, h_nprimal;
   std::vector<signed char> h_psign;
   std::vector<long long> h_psign_off, h_perm_off, h_kdst, h_bdst, h_kdiag, h_rowbase;
   std::vector<int> h_krowptr, h_kcolidx;
   std::vector<int> h_frowptr, h_fcol, h_fsrc;    // both triangles of K row by row (refinement residual)
   std::vector<long long> h_flong;                // its rows longer than FULL_LONG_ROW
   std::vector<int> h_bt_rowptr, h_bt_colidx;     // border CSR by (block, Schur column) ...
   std::vector<long long> h_bt_xoff;
   std::vector<double> h_bval;
   std::vector<int> h_br_rowptr, h_br_sc, h_br_src;   // ... and by leaf row (k_border_mult_rows)
   std::vector<int> h_schur_slot;
   std::vector<LeafDesc> h_leafdesc;              // the level-0 simple leaves, in the order of h_sns (k_leaf_bwd)
   std::vector<int> h_lf_rows, h_lf_ptr, h_lf_src, h_lf_pos;   // their L entries by target row (k_leaf_fwd_gather)
   std::vector<int> h_lb_list;                    // the simple leaves that own border rows (k_leaf_border)
   std::vector<const std::vector<int>*> tile_first;   // per block BlockSym::tile_first (pointers into sym)
   void drop_uploaded();
};

// Symbolic analysis of every block (threads over analyze_block); with_border: the border rows ride in the panels
int analyze_blocks(const std::vector<BlockInput>& in, int S, const AnalyzeOptions& opt, int n_threads, bool with_border, std::vector<BlockSym>& sym);
// Schur contribution by the augmented partial factorisation or by blocked solves with the plain factor: which is cheaper
bool blocked_solves_cheaper(const std::vector<BlockSym>& sym, int S, const AnalyzeOptions& opt);
// every block is multifrontal and every front, with its staged leaf data, fits the LDS
bool fronts_fit(const std::vector<BlockSym>& sym, const AnalyzeOptions& opt);
// the border split has to go: taken by some block, but the head is not multifrontal or k_border_schur's LDS need does not fit
bool border_split_must_go(const std::vector<BlockSym>& sym, bool mf);
// analyze_blocks with the two retries (blocked solves cheaper: without border; border split must go: back to full panels);
// settles knobs.schur_mode_eff and knobs.mf, may take opt.mf_split_nb_max off
int analyze_symbolic(const std::vector<BlockInput>& in, int S, int n_threads, AnalyzeOptions& opt, LayoutKnobs& knobs, std::vector<BlockSym>& sym);

int build_batch_layout(const std::vector<BlockInput>& in, const std::vector<BlockSym>& sym, int S, const LayoutKnobs& knobs,
                       BatchLayout& out);
// the properties of a layout the kernels rely on (include/pips_hip.h, pips_layout_probe); PIPS_ERR_STATE names the first that fails
int check_batch_layout(const std::vector<BlockInput>& in, const std::vector<BlockSym>& sym, int S, const LayoutKnobs& knobs,
                       const BatchLayout& lay);

}  // namespace pips
