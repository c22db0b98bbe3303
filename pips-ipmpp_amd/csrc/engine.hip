// Device engine of the MI355X KKT backend: batched numeric factorisation / solves for all leaf blocks of one GPU,
// and the C ABI declared in include/pips_hip.h.  Three layers of this translation unit have files of their own, included where they
// stand: the dense root solver (denseroot.hip.h), the fused KKT system (kkt.hip.h), the per-leaf handles (ldlhandle.hip.h).
//
// Reference call sites replaced (see include/pips_hip.h for the per-entry citations):
//   DistributedLeafLinearSystem::factor2 -> solver->matrixChanged()          (DistributedLeafLinearSystem.C:74-86)
//   addTermToSchurComplBlocked + addBiTLeftKiBiRightToResBlockedParallelSolvers (DistributedLinearSystem.C:766-1175)
//   DeSymIndefSolver::matrixChanged/solve                                      (DeSymIndefSolver.C:56-129)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "devmem.h"
#include "layout.h"
#include "detplan.h"
#include "tileplan.h"
#include "multiplan.h"
#include "knobs.h"
#include "schurtarget.h"
#include "kernels.hip.h"
#include "rootkernel.hip.h"
#include "tailkernel.hip.h"
#include "pips_hip.h"

namespace pips {

static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }
std::atomic<long long> g_host_waits{0};
// per call site: a small open-addressed table keyed by (file, line) - the literals' addresses are stable, a site is entered once
struct WaitSite { std::atomic<const char*> file{nullptr}; std::atomic<int> line{0}; std::atomic<long long> n{0}; };
static WaitSite g_wait_sites[128];
void note_host_wait(const char* file, int line) {
   g_host_waits.fetch_add(1, std::memory_order_relaxed);
   size_t h = ((size_t)(uintptr_t)file / 8 + (size_t)line * 31) % 128;
   for (int probe = 0; probe < 128; ++probe, h = (h + 1) % 128) {
      WaitSite& w = g_wait_sites[h];
      const char* f = w.file.load(std::memory_order_acquire);
      if (!f) {
         const char* expect = nullptr;
         if (w.file.compare_exchange_strong(expect, file)) { w.line.store(line); f = file; }
         else f = expect;
      }
      if (f == file) {
         while (w.line.load() == 0) {}   // (the entering thread stores the line right after the file)
         if (w.line.load() == line) { w.n.fetch_add(1, std::memory_order_relaxed); return; }
      }
   }
}
const char* last_error() { return g_last_error.c_str(); }

#define HIP_TRY(expr)                                                                              \
   do {                                                                                            \
      hipError_t _e = (expr);                                                                      \
      if (_e != hipSuccess) PIPS_FAIL(PIPS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
   } while (0)
#define PIPS_TRY(expr)                    \
   do {                                   \
      if (int _rc = (expr)) return _rc;   \
   } while (0)

// deterministic mode by the environment: the default of the batches (pips_hip_batch_create) and of the leaf handles' sparse Schur calls
static bool env_deterministic() { return knob_int<K_DETERMINISTIC>() != 0; }

static inline int grid_for(long long n, int block, int cap = 4096) {
   long long g = (n + block - 1) / block;
   if (g < 1) g = 1;
   if (g > cap) g = cap;
   return (int)g;
}

// ---------------------------------------------------------------------------------------------------------------
// tiled dense LDL^T driver shared by the leaf tails and the dense root
// ---------------------------------------------------------------------------------------------------------------
// The task plans are made on the host (tileplan.h); the four structs here add the device copies.
// The column plan (ColumnPlan) and its tasks on the device
struct TailPlan : ColumnPlan {
   DevBuf<TileTask> d_tasks;
   int build_leaf(const std::vector<BlkDesc>& blks, const TileFirst& first, int group) {
      ColumnPlan::build_leaf(blks, first, group);
      return d_tasks.upload(h_tasks);
   }
   int build_root(const std::vector<BlkDesc>& blks, int panel, bool lookahead) {
      ColumnPlan::build_root(blks, panel, lookahead);
      return d_tasks.upload(h_tasks);
   }
};

// A leaf column plan regrouped by groups of P tile columns (GroupPlan), tasks and strips on the device
struct PanelPlan : GroupPlan {
   DevBuf<TileTask> d_tasks;
   DevBuf<TileStrip> d_strips;
   int build(const TailPlan& p, int P_) {
      *this = PanelPlan();
      GroupPlan::build(p, P_);
      if (h_tasks.empty()) h_tasks.push_back({-1, 0, 0, 0});
      if (h_strips.empty()) h_strips.push_back({0, 0});
      PIPS_TRY(d_tasks.upload(h_tasks));
      return d_strips.upload(h_strips);
   }
};

// Single-launch tail sweeps (kernels.hip.h k_tail_rows_fwd / _bwd): task list (block, tile row) sorted by row, ticket and flag
// storage.  PIPS_HIP_SWEEP_LAUNCHES (set to any value) keeps the launch-per-tile-column kernels.
struct SweepRt {
   DevBuf<TileTask> d_tasks;
   int n_tasks = 0;
   DevBuf<int> d_ints;             // [0 .. 2 NRHS) ticket / finished per right-hand side, then the error word, then the flags
   long long n_flags = 0;
   DevBuf<long long> d_flag_off, d_tfirst_off;
   DevBuf<int> d_tfirst;
   int epoch = 0;
   bool enabled = false;
   long long poll_limit = SWEEP_POLL_LIMIT;
   // A wait that gave up poisoned its output with NaN and raised the error word; the host learns of it at its next synchronisation
   // point (batch sync, inertia queries, host-side solves): the word is read, cleared and turned into an error return.
   int take_error(const char* who) {
      if (!d_ints) return PIPS_OK;
      int w = 0;
      HIP_TRY(hipMemcpy(&w, d_ints + 2 * SWEEP_NRHS_MAX, sizeof(int), hipMemcpyDeviceToHost));
      if (!w) return PIPS_OK;
      HIP_TRY(hipMemset(d_ints + 2 * SWEEP_NRHS_MAX, 0, sizeof(int)));
      PIPS_FAIL(PIPS_ERR_HIP, "%s: a single-launch solve sweep gave up waiting for a piece of the solution after %lld polls (its output is NaN); "
                              "another process holding the device for seconds can cause that - PIPS_HIP_SWEEP_LAUNCHES (set to any value) selects the launch-per-column sweeps",
                who, poll_limit);
   }
   int build(const std::vector<BlkDesc>& blks, const TileFirst* first) {
      *this = SweepRt();
      static_assert(KNOBS[K_SWEEP_POLL_LIMIT].dflt == SWEEP_POLL_LIMIT, "the table's default is the kernels' limit");
      poll_limit = knob_int<K_SWEEP_POLL_LIMIT>();
      SweepLists l;
      l.build(blks, first);
      n_tasks = (int)l.tasks.size();
      int rc;
      if ((rc = d_tasks.upload(l.tasks))) return rc;
      if ((rc = d_flag_off.upload(l.flag_off))) return rc;
      if (first) {
         if ((rc = d_tfirst.upload(l.tfirst))) return rc;
         if ((rc = d_tfirst_off.upload(l.tfirst_off))) return rc;
      }
      n_flags = std::max<long long>(l.n_flags, 1);
      const size_t ints = (size_t)(2 * SWEEP_NRHS_MAX + 2 + n_flags * SWEEP_NRHS_MAX);
      PIPS_TRY(d_ints.alloc_zero(ints));
      epoch = 0;
      enabled = n_tasks > 0 && !knob_set<K_SWEEP_LAUNCHES>();
      return PIPS_OK;
   }
   SweepArgs args(long long xw_stride, hipStream_t st) {
      int* ep = d_ints + 2 * SWEEP_NRHS_MAX + 1;
      hipLaunchKernelGGL(k_sweep_bump, dim3(1), dim3(1), 0, st, ep);
      return SweepArgs{d_tasks, n_tasks, d_ints, d_ints + 2 * SWEEP_NRHS_MAX + 2, d_flag_off, d_tfirst, d_tfirst_off, ep,
                       d_ints + 2 * SWEEP_NRHS_MAX, n_flags, xw_stride, poll_limit};
   }
};

struct PhaseTimer {
   bool on = false;
   struct Rec { hipEvent_t a, b; int phase; };
   std::vector<Rec> recs;
   std::vector<hipEvent_t> pool;
   size_t used = 0;
   static constexpr int NPHASE = 16;
   double ms[NPHASE] = {0};
   long long cnt[NPHASE] = {0};
   hipEvent_t get() {
      if (used == pool.size()) {
         hipEvent_t e;
         (void)hipEventCreate(&e);
         pool.push_back(e);
      }
      return pool[used++];
   }
   void reset() { recs.clear(); used = 0; }
   void begin(hipStream_t s, int phase) {
      if (!on) return;
      Rec r{get(), get(), phase};
      (void)hipEventRecord(r.a, s);
      recs.push_back(r);
   }
   void end(hipStream_t s) {
      if (!on) return;
      (void)hipEventRecord(recs.back().b, s);
   }
   // a record that stays open across others: begin_i returns its index (-1 when off)
   int begin_i(hipStream_t s, int phase) {
      if (!on) return -1;
      begin(s, phase);
      return (int)recs.size() - 1;
   }
   void end_i(int idx, hipStream_t s) {
      if (on && idx >= 0) (void)hipEventRecord(recs[idx].b, s);
   }
   // a record over a lexical scope: begins where it is declared, ends where the scope is left, an error return included.  t may be null
   struct Scope {
      PhaseTimer* t; hipStream_t s; int idx;
      Scope(PhaseTimer* t_, hipStream_t s_, int phase) : t(t_), s(s_), idx(t_ ? t_->begin_i(s_, phase) : -1) {}
      ~Scope() { if (t) t->end_i(idx, s); }
      Scope(const Scope&) = delete;
      Scope& operator=(const Scope&) = delete;
   };
   void collect() {
      for (int i = 0; i < NPHASE; ++i) { ms[i] = 0; cnt[i] = 0; }
      for (auto& r : recs) {
         float t = 0;
         if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { ms[r.phase] += t; ++cnt[r.phase]; }
      }
   }
   ~PhaseTimer() { for (auto e : pool) (void)hipEventDestroy(e); }
};

// Device side of the single tail launch k_tail_ldl (tailkernel.hip.h): the eight task lists (TailSingleLists), the flags, the template
// they start from and the tickets
struct TailSingle {
   TailLdlArgs args{};
   DevBuf<TileTask> d_tasks;
   DevBuf<int> d_flags, d_flags_init, d_ctl;
   DevBuf<long long> d_flag_off;
   long long n_flags = 0;
   int n_tasks = 0, n_blocks = 0;
   int build(const TailPlan& p, const std::vector<BlkDesc>& blks, hipStream_t stream) {
      *this = TailSingle();
      TailSingleLists l;
      l.build(p, blks);
      n_blocks = (int)blks.size();
      n_flags = l.n_flags;
      n_tasks = l.n_tasks;
      std::copy(l.xoff, l.xoff + 9, args.xoff);
      if (l.tasks.empty()) l.tasks.push_back({0, 0, 0, 0});
      int rc;
      if ((rc = d_tasks.upload(l.tasks)) || (rc = d_flags_init.upload(l.init)) || (rc = d_flag_off.upload(l.foff))) return rc;
      PIPS_TRY(d_flags.alloc(l.init.size()));
      PIPS_TRY(d_ctl.alloc(16));
      HIP_TRY(hipMemsetAsync(d_ctl, 0, 16 * sizeof(int), stream));
      args.tasks = d_tasks; args.flags = d_flags; args.flag_off = d_flag_off; args.ctl = d_ctl;
      return PIPS_OK;
   }
};

// Plain data, built per call and filled by name (Engine::ctx, DenseLdl::ctx): what only one of the two owners has keeps its default with the other
struct TailCtx {
   const BlkDesc* d_blks = nullptr;
   const TailPlan* plan = nullptr;
   double* d_arena = nullptr;
   double* d_uarena = nullptr;          // scaled copies U = L D of the tail rows (BlkDesc::U), B operand of the updates
   double* d_dtail = nullptr;
   double* d_winv = nullptr;
   const signed char* d_psign = nullptr;
   const long long* d_psign_off = nullptr;
   int* d_inertia = nullptr;
   const double* d_pref = nullptr;
   hipStream_t stream = nullptr;
   hipStream_t side = nullptr;          // second stream for the lookahead of the right-looking root factorisation
   hipEvent_t ev_panel = nullptr;       // main -> side: panel j is final (trsm done)
   hipEvent_t ev_rest = nullptr;        // side -> main: trailing update of panel j is done
   SweepRt* sweep = nullptr;            // single-launch solve sweeps
   PhaseTimer* timer = nullptr;         // leaf batch: where the factorisation books its tail phases (Engine::factor_tail sets it, the solves do not)
   const int* d_bmap = nullptr;         // leaf batch: compressed border ids of the blocks
   bool is_root = false;                // dense root: same update kernel under its own name (k_tile_gemm<3>)
   const int* d_sctab = nullptr;        // sparse Schur complement: per-block position tables (kernels.hip.h sc_entry)
   // Schur SYRK in row-panel groups (several ranks): group p holds the tile rows whose first Schur row lies in panel p; after
   // its launch ev_sc[p] is recorded and rows of panel p are final on this rank (Engine::set_sc_panels)
   const std::vector<TaskList>* sc_groups = nullptr;
   const TileTask* d_sc_tasks = nullptr;
   const std::vector<hipEvent_t>* ev_sc = nullptr;
   // k_tile_gemm_bal (tasks drawn from per-XCD counters, an eighth more workgroups than tasks): pool of 8-counter slots, zeroed at the
   // start of a factorisation; every such launch takes the next slot
   int* d_ctr_pool = nullptr;
   int* ctr_cursor = nullptr;
   // deterministic Schur accumulation (DetGroupPlan, detplan.h): the blocks are cut into at most eight contiguous groups with a
   // buffer each; round k of the SYRK handles the k-th block of every group, so a launch never has two workgroups on the same
   // entry of a buffer and the blocks of a group arrive in their order; k_reduce_groups then adds the buffers in a fixed tree
   const std::vector<TaskList>* det_rounds = nullptr;
   const TileTask* d_det_tasks = nullptr;
   double* d_gbuf = nullptr;
   long long gstride = 0;
   const int* d_blk_group = nullptr;
   int n_groups = 0, first_slot = 0;
   long long sc_len = 0;                // sparse Schur complement: length of its value array (one group buffer)
   bool det_defer_reduce = false;       // several ranks: the group buffers are added over ALL ranks' groups in one fixed tree by the caller
   bool det_reduce_later = false;       // Schur mode 2: the blocked solves fill the group buffers after the tail; Engine::factor adds them then
   bool bunch_kaufman = false;          // diagonal tiles with 1 x 1 / 2 x 2 pivoting (k_tile_diag_bk) instead of the static pivot order
   int *d_pert_cnt = nullptr, *d_pert_list = nullptr;   // ... and where they record the indices no pivot was found for inside the tile
   const double* bk_orig = nullptr;                     // the matrix being factorised as the caller holds it (partner search), its layout, the order
   int bk_orig_ld = 0, bk_orig_rowmajor = 0;
   const int* d_bk_perm = nullptr;
   int bk_isolate = 0;
   const TailSingle* single = nullptr;   // the leaf tails as one dependency-driven launch (tailkernel.hip.h) instead of the column loop
   const PanelPlan* panels = nullptr;    // the leaf tails group by group: diagonal block on the side stream, one panel launch below it (tail_panels)
};
constexpr int GEMM_CTR_SLOTS = 4096;
constexpr int GEMM_BAL_MIN_TASKS = 1024;   // below two full rounds of the chip a static one-task-per-workgroup launch does as well

// deterministic mode: the group buffers into SC in the fixed tree of k_reduce_groups (unless the caller adds all ranks' groups itself)
static void reduce_det_groups(const TailCtx& c, double* SC, int ldSC) {
   const int S_ = ldSC;
   if (c.det_defer_reduce) {
   } else if (c.d_sctab)   // sparse Schur complement: the value array as one column
      hipLaunchKernelGGL(k_reduce_groups, dim3((unsigned)std::max(1LL, std::min(1024LL, (c.sc_len + 255) / 256)), 1), dim3(256), 0, c.stream, SC, 0, (int)c.sc_len,
                         c.d_gbuf, c.gstride, c.n_groups, c.first_slot);
   else
      hipLaunchKernelGGL(k_reduce_groups, dim3(std::max(1, std::min(64, (S_ + 255) / 256)), S_), dim3(256), 0, c.stream, SC, ldSC, S_, c.d_gbuf,
                         c.gstride, c.n_groups, c.first_slot);
}

// The launch sites of the tile kernels (kernels.hip.h), one per kernel: list l of the task array `tasks` on stream st.  k_tile_gemm (MODE 0 / 3 / 4
// updates, 1 / 5 trsm, 2 the Schur SYRK) deals its tasks to eight shares, one per XCD: a multiple of eight workgroups.  Only the SYRK takes SC, the
// position tables of a sparse SC and, in deterministic rounds, the group buffers
static inline int tile_grid(int n) { return (n + 7) / 8 * 8; }
template <int MODE>
static void launch_tile_gemm(const TailCtx& c, const TileTask* tasks, const TaskList& l, hipStream_t st, double* SC = nullptr, int ldSC = 0) {
   const bool rounds = MODE == 2 && c.det_rounds;
   hipLaunchKernelGGL(k_tile_gemm<MODE>, dim3(tile_grid(l.cnt)), dim3(512), 0, st, tasks + l.off, l.cnt, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, c.d_bmap, SC, ldSC,
                      MODE == 2 ? c.d_sctab : nullptr, c.d_uarena, rounds ? c.d_gbuf : nullptr, rounds ? c.gstride : 0, rounds ? c.d_blk_group : nullptr);
}
// k_tile_gemm_bal (MODE 0 and 2): an eighth more workgroups than tasks, which they draw from the next eight-counter slot of the pool
static bool tile_gemm_bal_ready(const TailCtx& c) { return c.d_ctr_pool && *c.ctr_cursor < GEMM_CTR_SLOTS; }
template <int MODE>
static void launch_tile_gemm_bal(const TailCtx& c, const TileTask* tasks, const TaskList& l, hipStream_t st, double* SC = nullptr, int ldSC = 0) {
   const int wgs = tile_grid(l.cnt) / 8 * 9;
   hipLaunchKernelGGL(k_tile_gemm_bal<MODE>, dim3(tile_grid(wgs)), dim3(512), 0, st, tasks + l.off, l.cnt, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, c.d_bmap, SC, ldSC,
                      MODE == 2 ? c.d_sctab : nullptr, c.d_uarena, c.d_ctr_pool + 8 * (*c.ctr_cursor)++);
}
// the diagonal tiles of a column, one workgroup each: Bunch-Kaufman or the static pivot order
static void launch_tile_diag(const TailCtx& c, const TileTask* tasks, const TaskList& l, hipStream_t st) {
   if (c.bunch_kaufman)
      hipLaunchKernelGGL(k_tile_diag_bk, dim3(l.cnt), dim3(256), 0, st, tasks + l.off, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, c.d_inertia, c.d_pert_cnt, c.d_pert_list,
                         c.bk_orig, c.bk_orig_ld, c.bk_orig_rowmajor, c.d_bk_perm, c.bk_isolate);
   else
      hipLaunchKernelGGL(k_tile_diag, dim3(l.cnt), dim3(256), 0, st, tasks + l.off, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, c.d_psign, c.d_psign_off, c.d_inertia, c.d_pref);
}
// leaf tails: launches of two rounds of the chip or more draw their tiles from per-XCD counters with an eighth more workgroups than
// tiles (k_tile_gemm_bal); smaller ones one tile per workgroup.  (A persistent work-stealing variant, static shares, the root's bulk
// in chunks or as a persistent launch with fewer workgroups than the chip holds: measured, no gain - docs/HISTORY_r4.md.)
static void launch_tile_update(const TailCtx& c, const TaskList& l, hipStream_t st, const TileTask* tasks = nullptr) {
   if (!tasks) tasks = c.plan->d_tasks;
   if (!c.is_root && l.cnt >= GEMM_BAL_MIN_TASKS && tile_gemm_bal_ready(c))
      launch_tile_gemm_bal<0>(c, tasks, l, st);
   else if (c.is_root)
      // The bulk update of the trailing matrix runs on the side stream beside the diagonal-tile chain of the next column.  Stream
      // priorities only order the launches the command processor has not started yet: once a launch of thousands of workgroups is
      // running, the single workgroup of k_tile_diag gets no slot until that launch drains (rocprofv3 trace at S = 16000: the diagonal
      // kernel "takes" 270 - 1140 us beside the bulk and 70 us alone - it is waiting): the lookahead overlaps only the drain.
      launch_tile_gemm<3>(c, tasks, l, st);
   else
      launch_tile_gemm<0>(c, tasks, l, st);
}

// PIPS_HIP_TAIL_TRACE: the per-task clocks of a k_tail_ldl launch into a file (tools/tail_trace.py); waits for the launch
static int dump_tail_trace(const TailCtx& c, DevBuf<long long>& d_trace, size_t n_trace, const char* trace_file) {
   const TailSingle& ts = *c.single;
   std::vector<long long> h(n_trace);
   std::vector<TileTask> ht((size_t)ts.n_tasks);
   HIP_TRY(hipStreamSynchronize(c.stream));
   HIP_TRY(hipMemcpy(h.data(), d_trace, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
   HIP_TRY(hipMemcpy(ht.data(), ts.d_tasks, ht.size() * sizeof(TileTask), hipMemcpyDeviceToHost));
   d_trace.reset();
   if (FILE* f = fopen(trace_file, "w")) {   // ticket, list, kind, block, ti, tj, K range, the three clocks
      for (int t = 0; t < ts.n_tasks; ++t) {
         int x = 0;
         while (x < 7 && t >= ts.args.xoff[x + 1]) ++x;
         fprintf(f, "%d %d %d %d %d %d %d %lld %lld %lld\n", t, x, ht[t].blk >> 24, ht[t].blk & 0xffffff, ht[t].ti, ht[t].tj, ht[t].pad, h[3 * (size_t)t], h[3 * (size_t)t + 1],
                 h[3 * (size_t)t + 2]);
      }
      fclose(f);
   }
   return PIPS_OK;
}

// the leaf tails as one dependency-driven launch (tailkernel.hip.h): flags from their template, tickets cleared, k_tail_ldl
static int tail_single_launch(const TailCtx& c) {
   const TailSingle& ts = *c.single;
   const char* trace_file = knob_text<K_TAIL_TRACE>();
   DevBuf<long long> d_trace;
   const size_t n_trace = (size_t)3 * ts.n_tasks + 32 * (size_t)(c.plan->ntc_max + 1);
   {
      PhaseTimer::Scope phase(c.timer, c.stream, 2);
      HIP_TRY(hipMemcpyAsync(ts.d_flags, ts.d_flags_init, (size_t)ts.n_flags * sizeof(int), hipMemcpyDeviceToDevice, c.stream));
      HIP_TRY(hipMemsetAsync(ts.d_ctl, 0, 9 * sizeof(int), c.stream));   // (the tickets; the error word stays until it is read)
      TailLdlArgs ta = ts.args; ta.n_tasks = ts.n_tasks;
      if (trace_file) {
         PIPS_TRY(d_trace.alloc(n_trace));
         HIP_TRY(hipMemsetAsync(d_trace, 0, n_trace * sizeof(long long), c.stream));
         ta.trace = d_trace;
      }
      // two workgroups per compute unit; a single block has fewer tasks ready than that and its diagonal tiles - the chain - run 3 x faster on a
      // compute unit of their own: one workgroup per unit there (a leaf handle's factorisation 6.9 -> 6.6 ms, level 1.5 1.03 -> 0.98 s per unit;
      // 8 blocks: 17.7 -> 17.9 ms, so only there)
      hipLaunchKernelGGL(k_tail_ldl, dim3(ts.n_blocks <= 2 ? 256 : 512), dim3(512), 0, c.stream, ta);
   }
   return trace_file ? dump_tail_trace(c, d_trace, n_trace, trace_file) : PIPS_OK;
}

// The launch-per-step factorisation of the tails, tile column by tile column: update, diagonal tiles, trsm; in the right-looking modes the
// trailing update of every finished panel.  trsm_tri: k_tile_gemm<5> for the trsm (tail_factor)
static int tail_columns(const TailCtx& c, bool trsm_tri) {
   const TailPlan& p = *c.plan;
   // Lookahead bookkeeping (right-looking modes with a side stream): while the side stream applies a finished panel to
   // the tile columns >= side_from, the main stream may only write columns left of that.
   bool side_busy = false; int side_from = 0;
   auto main_writes = [&](int col) -> int {
      if (side_busy && col >= side_from) {
         HIP_TRY(hipStreamWaitEvent(c.stream, c.ev_rest, 0));
         side_busy = false;
      }
      return PIPS_OK;
   };
   for (int j = 0; j < p.ntc_max; ++j) {
      PIPS_TRY(main_writes(j));
      const bool ahead = c.side && p.upd_diag[j].cnt > 0;   // left-looking batch: diagonal tiles first, factorised on the side stream
      if (ahead) {
         // side stream: update the diagonal tiles of column j (deep K, one workgroup per block) and factorise them, while
         // the main stream updates the rest of the column
         HIP_TRY(hipEventRecord(c.ev_panel, c.stream));
         HIP_TRY(hipStreamWaitEvent(c.side, c.ev_panel, 0));
         launch_tile_gemm<4>(c, p.d_tasks, p.upd_diag[j], c.side);
         launch_tile_diag(c, p.d_tasks, p.diag[j], c.side);
         HIP_TRY(hipEventRecord(c.ev_rest, c.side));
      } else if (p.upd_diag[j].cnt > 0) {
         launch_tile_gemm<4>(c, p.d_tasks, p.upd_diag[j], c.stream);
      }
      if (p.upd[j].cnt > 0) { PhaseTimer::Scope phase(c.timer, c.stream, 2); launch_tile_update(c, p.upd[j], c.stream); }
      if (ahead) {
         HIP_TRY(hipStreamWaitEvent(c.stream, c.ev_rest, 0));   // trsm needs Winv_j and d_j
      } else {
         PhaseTimer::Scope phase(c.timer, c.stream, 3);
         launch_tile_diag(c, p.d_tasks, p.diag[j], c.stream);
      }
      if (p.trsm[j].cnt > 0) {
         PhaseTimer::Scope phase(c.timer, c.stream, 4);
         if (trsm_tri) launch_tile_gemm<5>(c, p.d_tasks, p.trsm[j], c.stream);
         else launch_tile_gemm<1>(c, p.d_tasks, p.trsm[j], c.stream);
      }
      // Bunch-Kaufman root that will be looked at (DenseLdl::check_pivots): multipliers beyond what a whole-column search allows?
      if (p.trsm[j].cnt > 0 && c.bunch_kaufman && c.is_root && c.d_pert_cnt)
         hipLaunchKernelGGL(k_bk_growth, dim3(TILE), dim3(256), 0, c.stream, c.d_blks, c.d_arena, j, 1e8, c.d_pert_cnt, c.d_pert_list);
      // right-looking modes: trailing update with the panel that ends at column j.  With a side stream the bulk of it
      // (tile columns >= j+2) runs there, so that the main stream can finish column j+1 and go on with its diagonal tile
      // and trsm meanwhile (lookahead of one column).
      if (p.trail_next[j].cnt > 0 || p.trail[j].cnt > 0) {
         PIPS_TRY(main_writes(j + 1));
         const bool split = c.side && p.trail[j].cnt > 0;
         if (split) {
            HIP_TRY(hipEventRecord(c.ev_panel, c.stream));   // panel final: its trsm is queued before this point
            HIP_TRY(hipStreamWaitEvent(c.side, c.ev_panel, 0));
            launch_tile_update(c, p.trail[j], c.side);       // queued behind the bulk of the previous panel
            HIP_TRY(hipEventRecord(c.ev_rest, c.side));
            side_busy = true;
            side_from = j + 2;
         }
         PhaseTimer::Scope phase(c.timer, c.stream, 2);
         if (p.trail_next[j].cnt > 0) launch_tile_update(c, p.trail_next[j], c.stream);
         if (!split && p.trail[j].cnt > 0) launch_tile_update(c, p.trail[j], c.stream);
      }
   }
   return main_writes(1 << 30);   // join the side stream
}

// The leaf tails group by group (PanelPlan; left-looking batches in the static pivot order with the triangular trsm): per group of P tile
// columns the main stream has two launches, the deep update of the tile rows below the group's diagonal block and one k_tile_panel that
// finishes those rows across the group; the block itself - its deep update, then per column short update, diagonal tile, trsm, the
// column launches' kernels on short lists - is a chain on the side stream beside the deep launch, from the panel launch of the group
// before (ev_panel) to this group's (ev_rest).  The panel launch is booked with the updates (phase 2), the trsm inside it included; a
// chain on the side stream is not booked (it ends under the deep launch: DESIGN.md 4.2).
static int tail_panels(const TailCtx& c) {
   const TailPlan& p = *c.plan;
   const PanelPlan& g = *c.panels;
   const int n_tasks = (int)g.h_tasks.size();
   for (int i = 0; i < g.n_groups; ++i) {
      // a group without a deep launch (the first) has nothing to hide its chain behind: it runs on the main stream, booked as the column
      // launches book their steps
      const bool beside = g.deep[i].cnt > 0;
      const hipStream_t st = beside ? c.side : c.stream;
      PhaseTimer* const tm = beside ? nullptr : c.timer;
      if (beside) {
         HIP_TRY(hipEventRecord(c.ev_panel, c.stream));
         HIP_TRY(hipStreamWaitEvent(c.side, c.ev_panel, 0));
      }
      if (g.pre[i].cnt > 0) { PhaseTimer::Scope phase(tm, st, 2); launch_tile_gemm<4>(c, g.d_tasks, g.pre[i], st); }
      if (g.block_deep[i].cnt > 0) { PhaseTimer::Scope phase(tm, st, 2); launch_tile_gemm<4>(c, g.d_tasks, g.block_deep[i], st); }
      for (int j = i * g.P; j < std::min((i + 1) * g.P, p.ntc_max); ++j) {
         if (g.upd_in[j].cnt > 0) { PhaseTimer::Scope phase(tm, st, 2); launch_tile_gemm<4>(c, g.d_tasks, g.upd_in[j], st); }
         { PhaseTimer::Scope phase(tm, st, 3); launch_tile_diag(c, p.d_tasks, p.diag[j], st); }
         if (g.trsm_in[j].cnt > 0) { PhaseTimer::Scope phase(tm, st, 4); launch_tile_gemm<5>(c, g.d_tasks, g.trsm_in[j], st); }
      }
      if (beside) {
         HIP_TRY(hipEventRecord(c.ev_rest, c.side));
         { PhaseTimer::Scope phase(c.timer, c.stream, 2); launch_tile_update(c, g.deep[i], c.stream, g.d_tasks); }
         HIP_TRY(hipStreamWaitEvent(c.stream, c.ev_rest, 0));
      }
      if (g.strips[i].cnt > 0) {
         PhaseTimer::Scope phase(c.timer, c.stream, 2);
         hipLaunchKernelGGL(k_tile_panel, dim3(tile_grid(g.strips[i].cnt)), dim3(512), 0, c.stream, g.d_strips + g.strips[i].off, g.strips[i].cnt, g.d_tasks, n_tasks,
                            c.d_blks, c.d_arena, c.d_dtail, c.d_winv, c.d_uarena);
      }
   }
   return PIPS_OK;
}

// The tails' Schur contribution SC -= L_b D L_b^T over the border rows of every block (k_tile_gemm<2>), one of four ways: deterministic
// rounds into the group buffers, row-panel groups with an event each, one balanced launch, one plain launch
static int tail_schur(const TailCtx& c, double* SC, int ldSC) {
   const TailPlan& p = *c.plan;
   const bool rounds = c.det_rounds != nullptr, panels = !rounds && c.sc_groups && !c.d_sctab;
   if (!SC || (!rounds && !panels && p.schur.cnt == 0)) return PIPS_OK;   // (no launch: no timer record either)
   PhaseTimer::Scope phase(c.timer, c.stream, 5);
   if (rounds) {
      for (const TaskList& l : *c.det_rounds)   // the group buffers were zeroed (and took the head's contributions) in Engine::factor
         if (l.cnt > 0) launch_tile_gemm<2>(c, c.d_det_tasks, l, c.stream, SC, ldSC);
      if (!c.det_reduce_later) reduce_det_groups(c, SC, ldSC);
   } else if (panels) {
      for (size_t g = 0; g < c.sc_groups->size(); ++g) {
         const TaskList& l = (*c.sc_groups)[g];
         if (l.cnt > 0) launch_tile_gemm<2>(c, c.d_sc_tasks, l, c.stream, SC, ldSC);
         HIP_TRY(hipEventRecord((*c.ev_sc)[g], c.stream));   // (an empty group too: its panel is final)
      }
   } else if (tile_gemm_bal_ready(c) && !c.d_sctab)
      launch_tile_gemm_bal<2>(c, p.d_tasks, p.schur, c.stream, SC, ldSC);
   else
      launch_tile_gemm<2>(c, p.d_tasks, p.schur, c.stream, SC, ldSC);
   return PIPS_OK;
}

// Numeric factorisation of the dense tails (leaf batch: all blocks at once; dense root: one block) and, with SC, their Schur contribution
static int tail_factor(const TailCtx& c, double* SC, int ldSC) {
   // trsm of the leaf tails in the static pivot order: Winv is lower triangular, k_tile_gemm<5> skips the products with its zeros
   // (PIPS_HIP_TRSM_DENSE=1: the dense product, for A/B runs and the test that compares the two bit for bit)
   const bool trsm_tri = !c.bunch_kaufman && !c.is_root && knob_int<K_TRSM_DENSE>() == 0;
   // ... and group by group, unless PIPS_HIP_TAIL_PANEL=0 (or the dense trsm) asks for the column launches
   if (!c.single && c.panels && c.side && trsm_tri && knob_int<K_TAIL_PANEL>() != 0) PIPS_TRY(tail_panels(c));
   else if (!c.single) PIPS_TRY(tail_columns(c, trsm_tri));
   else if (c.single->n_tasks > 0) PIPS_TRY(tail_single_launch(c));
   PIPS_TRY(tail_schur(c, SC, ldSC));
   HIP_TRY(hipGetLastError());
   return PIPS_OK;
}

static int tail_fwd(const TailCtx& c, double* xw, int nrhs = 1, long long xw_stride = 0) {
   const TailPlan& p = *c.plan;
   if (c.sweep && c.sweep->enabled && nrhs <= SWEEP_NRHS_MAX) {
      hipLaunchKernelGGL(k_tail_rows_fwd, dim3(c.sweep->n_tasks, nrhs), dim3(256), 0, c.stream, c.sweep->args(xw_stride, c.stream), c.d_blks, c.d_arena, c.d_dtail,
                         c.d_winv, xw);
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   for (int j = 0; j < p.ntc_max; ++j)
      if (p.fwd[j].cnt > 0)
         hipLaunchKernelGGL(k_tail_fwd, dim3(p.fwd[j].cnt, nrhs), dim3(256), 0, c.stream, p.d_tasks + p.fwd[j].off, c.d_blks,
                            c.d_arena, c.d_dtail, c.d_winv, xw, j, xw_stride);
   HIP_TRY(hipGetLastError());
   return PIPS_OK;
}

static int tail_bwd(const TailCtx& c, double* xw, int nrhs = 1, long long xw_stride = 0, int border = 0) {
   const TailPlan& p = *c.plan;
   if (p.ntc_max == 0) return PIPS_OK;   // no block has a dense tail
   if (border && !(c.sweep && c.sweep->enabled)) PIPS_FAIL(PIPS_ERR_STATE, "border-backward sweep needs the single-launch tail sweeps");
   if (c.sweep && c.sweep->enabled && nrhs <= SWEEP_NRHS_MAX) {
      hipLaunchKernelGGL(k_tail_rows_bwd, dim3(c.sweep->n_tasks, nrhs), dim3(256), 0, c.stream, c.sweep->args(xw_stride, c.stream), c.d_blks, c.d_arena, c.d_dtail,
                         c.d_winv, xw, border);
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   for (int i = p.ntc_max - 1; i >= 0; --i)
      if (p.bwd[i].cnt > 0)
         hipLaunchKernelGGL(k_tail_bwd, dim3(p.bwd[i].cnt, nrhs), dim3(256), 0, c.stream, p.d_tasks + p.bwd[i].off, c.d_blks,
                            c.d_arena, c.d_dtail, c.d_winv, xw, i, xw_stride);
   HIP_TRY(hipGetLastError());
   return PIPS_OK;
}

// The tail sweeps of np interleaved panels of MQ right-hand sides (kernels.hip.h "multi-vector solves"; panel p at xm + p * panel_stride), the
// one launch site of k_mtail_rows_fwd / _bwd<NC> and k_mtail_fwd / _bwd for both owners (Engine::solve_once_multi, DenseLdl::solve_multi_dev).
// mtail_slices chooses once per pass: 0 = the launch per tile column, else the slices per panel of the single launch per direction.
// Few tile rows per step (a single leaf, a small root): a workgroup takes a quarter or a half of a panel's right-hand sides, so that the chain
// of a pass - one workgroup's tile products per step - is shorter; many: whole panels, L read once per 32 right-hand sides.  Every workgroup
// of the launch must be resident for the slices to advance side by side (two per compute unit: the whole tile sits in registers), so the
// finest slicing that keeps the launch within 512 workgroups is taken.  forced: PIPS_HIP_MULTI = 2 / 4 (Engine::multi_knob().slices; tests);
// pin: a fixed slicing - the blocked Schur solves of deterministic mode, whose bits must not follow sweep->n_tasks, i.e. the blocks per rank
static int mtail_slices(const TailCtx& c, int np, int forced, int pin = 0) {
   if (!(c.sweep && c.sweep->enabled && np * 4 <= SWEEP_NRHS_MAX && c.plan->ntc_max > 0)) return 0;   // (tickets and flag rows are per blockIdx.y)
   const long long wg = (long long)c.sweep->n_tasks * np;
   return pin ? pin : forced ? forced : wg * 4 <= 512 ? 4 : wg * 2 <= 512 ? 2 : 1;
}
static void mtail_sweep(const TailCtx& c, double* xm, long long panel_stride, int np, int sl, int backward) {
   const TailPlan& p = *c.plan;
   if (sl > 0) {
      const SweepArgs sa = c.sweep->args(0, c.stream);
      const dim3 grid(c.sweep->n_tasks, np * sl), wg(256);
      if (sl == 4 && !backward) hipLaunchKernelGGL(k_mtail_rows_fwd<2>, grid, wg, 0, c.stream, sa, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, xm, panel_stride);
      else if (sl == 4) hipLaunchKernelGGL(k_mtail_rows_bwd<2>, grid, wg, 0, c.stream, sa, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, xm, panel_stride);
      else if (sl == 2 && !backward) hipLaunchKernelGGL(k_mtail_rows_fwd<4>, grid, wg, 0, c.stream, sa, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, xm, panel_stride);
      else if (sl == 2) hipLaunchKernelGGL(k_mtail_rows_bwd<4>, grid, wg, 0, c.stream, sa, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, xm, panel_stride);
      else if (!backward) hipLaunchKernelGGL(k_mtail_rows_fwd<8>, grid, wg, 0, c.stream, sa, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, xm, panel_stride);
      else hipLaunchKernelGGL(k_mtail_rows_bwd<8>, grid, wg, 0, c.stream, sa, c.d_blks, c.d_arena, c.d_dtail, c.d_winv, xm, panel_stride);
   } else if (!backward) {
      for (int j = 0; j < p.ntc_max; ++j)
         if (p.fwd[j].cnt > 0)
            hipLaunchKernelGGL(k_mtail_fwd, dim3(p.fwd[j].cnt, np), dim3(256), 0, c.stream, p.d_tasks + p.fwd[j].off, c.d_blks, c.d_arena, c.d_dtail,
                               c.d_winv, xm, j, panel_stride);
   } else {
      for (int i = p.ntc_max - 1; i >= 0; --i)
         if (p.bwd[i].cnt > 0)
            hipLaunchKernelGGL(k_mtail_bwd, dim3(p.bwd[i].cnt, np), dim3(256), 0, c.stream, p.d_tasks + p.bwd[i].off, c.d_blks, c.d_arena, c.d_dtail,
                               c.d_winv, xm, i, panel_stride);
   }
}


// ---------------------------------------------------------------------------------------------------------------
// batched leaf engine (BlockInput, LevelRange, MfLaunch and the host pass of the analysis: layout.h)
// ---------------------------------------------------------------------------------------------------------------
// What an analysis owns on the device and what belongs to it on the host: Engine::release() resets exactly this (a move-assignment
// from a fresh one), so a buffer declared here is freed and reset without a second mention anywhere.  The settings that survive a
// re-analysis, the inputs and the streams are members of Engine itself.
struct EngineAnalysis {
   DevBuf<double> d_norms;      // 3 * nblk: ||r||, ||rhs||, ||x|| per block
   PinnedBuf<double> h_norms;
   DevBuf<int> d_frowptr, d_fcol, d_fsrc;   // full row structure of K for the refinement residual
   DevBuf<long long> d_flong;               // its rows longer than FULL_LONG_ROW
   DevBuf<int> d_sctab;                     // sparse Schur complement (set_sc_tables): position tables, BlkDesc::sctab_off
   long long sc_len = 0;                    // ... and the length of its value array (one group buffer of deterministic mode); 0: dense, S x S
   DevBuf<int> d_schur_cols, d_schur_slot;
   // Schur mode 2 into the sparse Schur complement (set_sc_tables; Engine::schur_by_packed_solves): the blocks' border column sets, per
   // border row its local index (-1: empty) and the start of its row of the block's position table, and on the host what the lists of
   // deterministic mode are built from
   SchurPack pack;
   int packed_rhs = 0;                  // max_b nb_b where the packed path is active, else 0
   DevBuf<int> d_pk_la;
   DevBuf<long long> d_pk_tabrow;
   PackRows h_pk_rows;
   std::vector<int> h_pk_tab;
   // fronts on the rows of K only (BlockSym::mf_konly): records and lists of k_border_rows / k_border_tail
   DevBuf<int> d_kb_rec;
   DevBuf<long long> d_kb_off;          // per supernode (sorted id): offset of its record, -1 none
   DevBuf<int> d_kb_list;               // fronts with border rows, level after level
   DevBuf<int> d_kb_tail;
   DevBuf<double> d_mfU;                // update matrices of the fronts
   DevBuf<double> d_mfLV;               // d and l of the simple leaves below fronts, front by front
   DevBuf<int> d_roots, d_root_off;     // fronts without a head parent, per block (k_root_assemble)
   // first touch of the tails (BatchLayout::tail_first_touch): per tail column the entries of K and of the border and the pieces of the
   // root fronts (k_tail_first_touch); the simple leaves whose products follow (k_leaf_products)
   DevBuf<long long> d_ft_colbase;
   DevBuf<int> d_ft_init_off, d_ft_piece_off, d_ft_leaves;
   DevBuf<FtInit> d_ft_init;
   DevBuf<FtPiece> d_ft_piece;
   DevBuf<BbBatch> d_bb_batches;        // border split (k_border_schur): batches of supernodes with border rows, block after block
   DevBuf<BbMeta> d_bb_meta;
   DevBuf<int> d_bb_off, d_bb_pos;      // batches of block b: [d_bb_off[b], d_bb_off[b + 1]); compressed border ids of the staged rows
   DevBuf<double> d_bb_out;             // deterministic mode: the blocks' border x border triangles before they join their groups
   DevBuf<int> d_bb_round_blk;          // deterministic mode: the blocks of round k of k_border_schur
   DevBuf<int> d_round_blk;             // deterministic mode: the blocks of round k of k_root_assemble (DetGroupPlan::round_off)
   DevBuf<int> d_mfint;                 // front records (common.h)
   DevBuf<long long> d_mfdbg;           // PIPS_HIP_MF_CLOCKS: phase stamps of every front (8 per supernode), dumped after the factorisation
   DevBuf<int> d_spine, d_spine_off;
   TailPlan plan;
   PanelPlan panels;                    // ... regrouped by groups of tile columns (tail_panels; not for the single-launch tails)
   SweepRt sweep;
   TailSingle tsingle;                  // the tails as one dependency-driven launch (tailkernel.hip.h)
   DevBuf<double> d_uarena;             // U = L D copies of the tails (see k_tile_gemm)
   DevBuf<double> d_arena, d_kval, d_bval, d_winv, d_dtail, d_xw, d_rhs, d_res, d_stage, d_pref;
   DevBuf<long long> d_kdst, d_bdst, d_kdiag, d_kptr, d_psign_off, d_perm_off, d_rowbase, d_bt_xoff;
   DevBuf<SnDesc> d_sns;
   DevBuf<BlkDesc> d_blks;
   // Forward substitution of the simple leaves as a gather (k_leaf_fwd_gather): the leaves' L entries by TARGET row - row list,
   // row pointers, source (the leaf's position in the work vector), values (written in this order by k_head_factor_simple through
   // d_lf_pos, which is indexed like d_rowidx).  No atomics, fixed order of the sums.
   DevBuf<int> d_lf_rows, d_lf_ptr, d_lf_src, d_lf_pos;
   DevBuf<double> d_lf_val;
   DevBuf<LeafDesc> d_leafdesc;         // compact records of the level-0 simple leaves, in the order of d_sns (k_leaf_bwd)
   DevBuf<int> d_lb_list;               // the simple leaves that own border rows (k_leaf_border)
   DevBuf<int> d_rowidx, d_upd, d_sncol, d_bmap, d_perm, d_inertia, d_nprimal;
   DevBuf<int> d_br_rowptr, d_br_sc, d_br_src;   // the border by leaf row (k_border_mult_rows)
   DevBuf<int> d_krowptr, d_kcolidx, d_bt_rowptr, d_bt_colidx, d_bt_rowsc;
   DevBuf<signed char> d_psign;
   // ---- deterministic mode (see Engine): slots, gather lists, group buffers.  What the lists hold is planned on the host (detplan.h)
   struct GatherList {
      long long n_targets = 0, n_slots = 0;
      DevBuf<long long> d_tgt, d_off, d_slots;
      int upload(const HostGather& h) {
         *this = GatherList();
         n_targets = (long long)h.tgt.size(); n_slots = (long long)h.slots.size();
         if (h.tgt.empty()) return PIPS_OK;
         int rc;
         if ((rc = d_tgt.upload(h.tgt)) || (rc = d_off.upload(h.off)) || (rc = d_slots.upload(h.slots))) return rc;
         return PIPS_OK;
      }
   };
   DetGroupPlan det;                    // groups, rounds and the sweep of the augmented factor: what the launches read of the plan
   ScKept sc_kept;                      // the Schur targets of the head as recorded (build_deterministic), for DetGroupPlan::sc_grp
   DevBuf<double> d_slot_val, d_vslot_val;
   DevBuf<double> d_mvslot;             // several right-hand sides: the forward substitution's slots for one panel of MQ (solve_multi)
   std::vector<GatherList> g_levels, gv_levels;   // targets inside the head, per level (factorisation / forward substitution)
   GatherList g_tail, g_sc, gv_tail;
   GatherList g_sc_grp;                 // Schur targets of the head inside the group buffers
   GatherList g_btm_grp;                // border rows per (group, Schur column): Br^T z summed group-wise, then in the fixed tree
   GatherList g_pk_grp;                 // packed blocked solves: contributions per (group, position of the value array) (k_border_tmult_chunk_packed_det)
   DevBuf<double> d_gvec, d_tvec;
   DevBuf<TileTask> d_det_tasks;
   DevBuf<double> d_gbuf;
   DevBuf<int> d_blk_group;
   GatherList g_btm, g_bm;              // border products: rows per Schur column, entries per leaf row
   // forward sweep of the augmented factor: the border slots of the work vector are gathered, target by target, from the border rows
   // of the head supernodes (k_border_gather_det: no atomics, fixed order) and then group-wise into d_gvec like Br^T z
   DevBuf<BgEntry> d_bg_ent;
   DevBuf<long long> d_bg_ptr, d_bg_slot;
   DevBuf<int> d_bg_idx;
   DevBuf<double> d_bg_val;
   GatherList g_bslot_grp;
   DevBuf<double> d_bt_tmp;
   DevBuf<int> d_gemm_ctr;              // counter slots of the persistent update kernel
   // ---- Schur SYRK in row-panel groups, so that a multi-rank root can reduce panel p while the leaves still compute p + 1 ..
   ScPanelPlan scp;                     // the groups and the panels' first rows (its tasks are dropped once uploaded)
   std::vector<hipEvent_t> ev_sc;       // one per group (destroyed by Engine::release / set_sc_panels)
   DevBuf<TileTask> d_sc_tasks;
   // ---- multi-RHS solve (Engine::ensure_multi_buffers)
   DevBuf<double> d_mx_xw, d_mx_rhs, d_mx_res;
   int mx_cap = 0;
   DevBuf<double> d_mmeasure;           // solve_multi: the refinement measure per right-hand side (device / pinned) ...
   PinnedBuf<double> h_mmeasure;
   DevBuf<int> d_midx;                  // ... and the columns that take the correction solve
   // ---- inertia counters in pinned host memory (Engine::fetch_inertia)
   PinnedBuf<int> h_inertia_pin;
   hipEvent_t ev_inertia = nullptr;     // (destroyed by Engine::release)
   bool inertia_in_flight = false, inertia_on_host = false;
};

// The host side of the analysis - offsets, sorted supernodes, launch lists, the decisions - is the BatchLayout (layout.h) the engine is
// built on; its big index arrays are dropped once they are uploaded.
struct Engine : EngineAnalysis, BatchLayout {
   int device = 0;
   hipStream_t stream = nullptr;
   int nblk = 0, S = 0;
   bool analyzed = false, factored = false;
   long long analysis_gen = 0;   // bumped by every analyze(): device buffers of the previous analysis are gone (captured graphs are stale)
   int refine_steps = 1;       // maximum number of iterative-refinement steps per solve
   double refine_tol = 0.0;    // > 0: adaptive refinement, stop as soon as the error measure of every block is <= tol
   int refine_mode = 0;        // 0: ||r_b||inf / ||rhs_b||inf ; 1: normwise backward error ||r_b||inf / (max|K_b| ||x_b||inf + ||rhs_b||inf)
   double last_refine_measure = 0.0;
   int last_refine_steps = 0;
   double thr_rel = 1e-13, repl_rel = 1e-8;
   AnalyzeOptions opt;
   std::vector<BlockInput> in;
   std::vector<BlockSym> sym;
   int schur_mode = 0;        // requested: 0 auto, 1 augmented partial factorisation, 2 blocked solves (reference K4-K6)
   int sn_width = 0;           // > 0: supernode width cap of this engine instead of the tuned default (the sparse root: a single block, every level is latency)
   PhaseTimer timer;
   std::vector<int> h_inertia;
   std::vector<double> h_amax;   // max|K_b| of the current factorisation (backward-error refinement criterion)

   ~Engine() {
      release();
      if (side) (void)hipStreamDestroy(side);
      if (ev_diag_in) (void)hipEventDestroy(ev_diag_in);
      if (ev_diag_out) (void)hipEventDestroy(ev_diag_out);
   }
   // everything the analysis owns goes, on the device and on the host; the settings, the inputs and the streams stay
   void release() {
      for (auto ev : ev_sc) (void)hipEventDestroy(ev);
      if (ev_inertia) (void)hipEventDestroy(ev_inertia);
      static_cast<EngineAnalysis&>(*this) = EngineAnalysis();
      static_cast<BatchLayout&>(*this) = BatchLayout();
      analyzed = factored = head_slots = false;
   }

   hipStream_t side = nullptr;                       // diagonal tiles of the tail are factorised here, beside the column update
   hipEvent_t ev_diag_in = nullptr, ev_diag_out = nullptr;
   // ---- deterministic mode (pips_hip_batch_set_deterministic): no FP64 atomics on the path.  Every scattered contribution of
   // the head owns a slot; at analyze time the kernels run once in recording mode, the host groups the slots by target (per
   // elimination-tree level, then the tail, then the Schur complement) and the factorisation gathers them in that fixed order.
   bool deterministic = false;
   // The slot / gather scheme of the head belongs to deterministic mode (without it, round 2 measured the head phase of config 2 at 5.0 ms
   // against 5.5 ms with FP64 atomics - not worth 16 bytes of device memory per contribution and the longer analysis; the switch that
   // selected it alone is gone).  Beyond HEAD_SLOTS_MAX contributions deterministic mode refuses.
   bool head_slots = false;
   static constexpr long long HEAD_SLOTS_MAX = 400LL * 1000 * 1000;
   int last_multi_path = 0;      // how the last solve(nrhs) went: 0 one sweep per right-hand side, 1 interleaved panels, 2 interleaved panels with the slot / gather forward substitution
   bool defer_group_reduce = false;   // set by pips_hip_kkt_factorize around its factor() call: it adds the groups of ALL ranks in one tree itself;
                                      // a direct pips_hip_batch_factor on the same batch reduces its own groups as on one rank
   // length of one group buffer: S x S (dense Schur complement) or the value array of the sparse one (set_sc_tables)
   long long det_gstride() const { return sc_len > 0 ? sc_len : (long long)S * S; }
   // The groups of the deterministic Schur accumulation for this rank of n_ranks (build_det_group_plan), uploaded.  (The group buffers
   // themselves are allocated by the first factorisation that has a Schur complement to fill: a system with the sparse root never needs
   // the n_groups x S x S doubles of the dense layout this is first called with.)
   int set_det_groups(int rank, int n_ranks) {
      if (!analyzed || !deterministic) return PIPS_OK;
      PackedTables packed;
      if (packed_rhs > 0) { packed.rows = &h_pk_rows; packed.tab = &h_pk_tab; }
      det = build_det_group_plan(*this, sym, S, rank, n_ranks, det_gstride(), sc_kept, packed);
      aug_sweeps_ok = det.aug_sweeps_ok;
      d_gbuf.reset(); d_gvec.reset(); d_tvec.reset();
      d_bg_ent.reset(); d_bg_ptr.reset(); d_bg_idx.reset(); d_bg_val.reset(); d_bg_slot.reset();
      if (mf) {
         PIPS_TRY(d_round_blk.upload(det.round_blk));
         PIPS_TRY(d_bb_round_blk.upload(det.bb_round_blk));
      }
      PIPS_TRY(d_det_tasks.upload(det.tasks));
      PIPS_TRY(d_blk_group.upload(det.grp));
      PIPS_TRY(g_sc_grp.upload(det.sc_grp));
      PIPS_TRY(g_btm_grp.upload(det.btm_grp));
      if (S > 0) {
         PIPS_TRY(d_gvec.alloc((size_t)8 * S));
         PIPS_TRY(d_tvec.alloc((size_t)S));
      }
      if (det.aug.ready) {   // forward_augmented_det
         PIPS_TRY(d_bg_ent.upload(det.aug.ent));
         PIPS_TRY(d_bg_ptr.upload(det.aug.ptr));
         PIPS_TRY(d_bg_idx.upload(det.aug.idx));
         PIPS_TRY(d_bg_slot.upload(det.aug.slot));
      }
      PIPS_TRY(g_bslot_grp.upload(det.aug.bslot_grp));
      if (det.aug.ready) PIPS_TRY(d_bg_val.alloc((size_t)std::max<long long>(det.aug.n_ent, 1)));
      PIPS_TRY(g_pk_grp.upload(det.pk_grp));
      det.drop_uploaded();
      return PIPS_OK;
   }
   int gemm_ctr_cursor = 0;
   // the Schur SYRK in row-panel groups (sc_panel_plan), one event per group
   int set_sc_panels(int n_panels) {
      if (!analyzed) PIPS_FAIL(PIPS_ERR_STATE, "set_sc_panels: analyze first");
      for (auto ev : ev_sc) (void)hipEventDestroy(ev);
      ev_sc.clear();
      d_sc_tasks.reset();
      scp = sc_panel_plan(*this, sym, S, n_panels);
      if (scp.groups.empty()) return PIPS_OK;
      for (size_t q = 0; q < scp.groups.size(); ++q) {
         hipEvent_t ev;
         HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
         ev_sc.push_back(ev);
      }
      PIPS_TRY(d_sc_tasks.upload(scp.tasks));
      std::vector<TileTask>().swap(scp.tasks);
      return PIPS_OK;
   }
   TailCtx ctx() {
      TailCtx c;
      c.d_blks = d_blks; c.plan = &plan; c.d_arena = d_arena; c.d_uarena = d_uarena; c.d_dtail = d_dtail; c.d_winv = d_winv;
      c.d_psign = d_psign; c.d_psign_off = d_psign_off; c.d_inertia = d_inertia; c.d_pref = d_pref;
      c.stream = stream; c.side = side; c.ev_panel = ev_diag_in; c.ev_rest = ev_diag_out; c.d_bmap = d_bmap; c.d_sctab = d_sctab;
      if (!scp.groups.empty()) { c.sc_groups = &scp.groups; c.d_sc_tasks = d_sc_tasks; c.ev_sc = &ev_sc; }
      c.d_ctr_pool = d_gemm_ctr; c.ctr_cursor = &gemm_ctr_cursor;
      if (deterministic && d_gbuf) {
         c.det_rounds = &det.rounds; c.d_det_tasks = d_det_tasks; c.d_gbuf = d_gbuf; c.gstride = det_gstride(); c.sc_len = sc_len; c.d_blk_group = d_blk_group;
         c.n_groups = det.n_groups; c.first_slot = det.first_slot;
         c.det_defer_reduce = det.global && defer_group_reduce;   // (only the kkt paths finish the reduction themselves)
      }
      c.sweep = &sweep;
      if (tail_single) {
         tsingle.args.blks = d_blks; tsingle.args.arena = d_arena; tsingle.args.uarena = d_uarena; tsingle.args.winv = d_winv; tsingle.args.dtail = d_dtail;
         tsingle.args.pref = d_pref; tsingle.args.psign = d_psign; tsingle.args.psign_off = d_psign_off; tsingle.args.inertia = d_inertia;
         c.single = &tsingle;
      } else if (panels.n_groups > 0)
         c.panels = &panels;
      return c;
   }

   // check inputs; read knobs; symbolic analysis with its two retries; host layout; upload; task plans; streams; deterministic mode.
   // What the previous analysis held goes first, whatever comes of this one (sym is overwritten: the old buffers would not match it);
   // the free memory that decides tail_single is thereby read as it always was, without the old buffers.
   int analyze(int n_threads) {
      for (int b = 0; b < nblk; ++b)
         if (in[b].n <= 0) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_analyze: block %d was never set", b);
      AnalyzeKnobs knobs;
      const EngineSettings settings{sn_width, deterministic, schur_mode};
      read_layout_knobs(&settings, opt, knobs);
      HIP_TRY(hipSetDevice(device));
      release();
      {
         size_t free_b = 0, total_b = 0;
         (void)hipMemGetInfo(&free_b, &total_b);
         knobs.free_device_bytes = (long long)free_b;
      }
      int rc = analyze_symbolic(in, S, n_threads, opt, knobs, sym);
      if (rc) return rc;
      {  // an input error is met here, before the first allocation
         BatchLayout lay;
         if ((rc = build_batch_layout(in, sym, S, knobs, lay))) return rc;
         static_cast<BatchLayout&>(*this) = std::move(lay);
      }
      if ((rc = upload_layout())) return rc;
      // the diagonal tile of a column runs ahead on the side stream, its update first; tile rows start at their envelope (variants of the
      // tail factorisation without either: docs/HISTORY_r1_r2.md)
      // tile columns per launch of the left-looking tail update (ColumnPlan::build_leaf, group).  configs[1], ms per unit / ms of update, two boxes:
      // 1 column 125.0 - 126.8 / 73.8 - 74.7; 2: 123.6 - 124.0 / 72.4; 3: 122.0 / 70.8; 4: 120.0 - 121.7 / 70.3 - 71.0; 6: 120.5 / 70.3; 8: 120.8 / 70.9
      const int pair2 = 4;   // (1: a column per launch; the switch that chose it went with round 6)
      if ((rc = plan.build_leaf(h_blks, tile_first, pair2))) return rc;
      if ((rc = sweep.build(h_blks, &tile_first))) return rc;
      if (tail_single) {
         if ((rc = tsingle.build(plan, h_blks, stream))) return rc;
         tsingle.args.poll_limit = knobs.tail_poll_limit;
         tsingle.args.diag_blocked = knobs.tail_diag_blocked;
      } else if ((rc = panels.build(plan, pair2)))
         return rc;
      drop_uploaded();
      if (!side) {
         // highest priority: the few workgroups of the diagonal chain must not queue behind the thousands of the column update
         int prio_lo = 0, prio_hi = 0;
         HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
         HIP_TRY(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, prio_hi));
         HIP_TRY(hipEventCreateWithFlags(&ev_diag_in, hipEventDisableTiming));
         HIP_TRY(hipEventCreateWithFlags(&ev_diag_out, hipEventDisableTiming));
      }
      h_inertia.assign(3 * nblk, 0);
      analyzed = true;
      ++analysis_gen;
      if (deterministic) {
         if (slots_total + vslots_total > HEAD_SLOTS_MAX)
            PIPS_FAIL(PIPS_ERR_STATE, "deterministic mode: %lld head contributions exceed the slot budget of %lld", slots_total + vslots_total, HEAD_SLOTS_MAX);
         if ((rc = build_deterministic(n_threads))) return rc;
         head_slots = true;
         if ((rc = set_det_groups(0, 1))) return rc;
      }
      return PIPS_OK;
   }

   // Allocation and upload of an analysis: one line per buffer, from the layout's arrays.  (The order is the one the allocations always
   // had: the addresses of the arenas, and with them the timings, stay what they were.)
   int upload_layout() {
      if (mf) {
         PIPS_TRY(d_roots.upload(h_roots));
         PIPS_TRY(d_root_off.upload(h_root_off));
      }
      if (n_bb > 0) {   // border split
         PIPS_TRY(d_bb_batches.upload(h_bb_batches));
         PIPS_TRY(d_bb_meta.upload(h_bb_meta));
         PIPS_TRY(d_bb_pos.upload(h_bb_pos));
         PIPS_TRY(d_bb_off.upload(h_bb_off));
      }
      if (kb_any) {   // fronts on the rows of K only
         PIPS_TRY(d_kb_rec.upload(h_kb_rec));
         PIPS_TRY(d_kb_off.upload(h_kb_off));
         PIPS_TRY(d_kb_list.upload(h_kb_list));
         PIPS_TRY(d_kb_tail.upload(h_kb_tail));
      }
      if (mf) {
         PIPS_TRY(d_mfint.upload(h_mfint));
         PIPS_TRY(d_mfU.alloc((size_t)std::max<long long>(mfU_total, 1)));
         PIPS_TRY(d_mfLV.alloc((size_t)std::max<long long>(mfLV_total, 1)));
      }
      PIPS_TRY(d_frowptr.upload(h_frowptr));
      PIPS_TRY(d_fcol.upload(h_fcol));
      PIPS_TRY(d_fsrc.upload(h_fsrc));
      PIPS_TRY(d_flong.upload(h_flong));
      if (deterministic && bt_rows_total > 0) {   // gather lists of the border products (see k_border_rowdot)
         const BorderGathers bg = border_product_gathers(*this);
         PIPS_TRY(g_btm.upload(bg.btm));
         PIPS_TRY(g_bm.upload(bg.bm));
         PIPS_TRY(d_bt_tmp.alloc((size_t)std::max<long long>(std::max(bt_rows_total, nnzB_total), 1)));
      }
      PIPS_TRY(d_schur_cols.upload(schur_cols));
      PIPS_TRY(d_schur_slot.upload(h_schur_slot));
      PIPS_TRY(d_arena.alloc(std::max<long long>(arena_total + bb_doubles + tail_scratch, 1)));
      if (tail_single) HIP_TRY(hipMemsetAsync(d_arena, 0, (size_t)arena_total * sizeof(double), stream));   // (tiles of the panels outside the envelopes are never written: they read as zero)
      if (bb_doubles > 0) HIP_TRY(hipMemsetAsync(d_arena + arena_total, 0, (size_t)bb_doubles * sizeof(double), stream));   // (the padding rows of the border-row arena stay zero)
      PIPS_TRY(d_uarena.alloc(std::max<long long>(uarena_total, 1)));
      PIPS_TRY(d_kval.alloc(std::max<long long>(nnzK_total, 1)));
      HIP_TRY(hipMemset(d_kval, 0, std::max<long long>(nnzK_total, 1) * sizeof(double)));
      PIPS_TRY(d_winv.alloc(std::max<long long>(winv_total, 1)));
      PIPS_TRY(d_dtail.alloc(std::max<long long>(dtail_total, 1)));
      PIPS_TRY(d_xw.alloc(std::max<long long>(xw_total, 1)));
      PIPS_TRY(d_pref.alloc(std::max<long long>(xw_total, 1)));
      PIPS_TRY(d_rhs.alloc(std::max<long long>(n_total, 1)));
      PIPS_TRY(d_res.alloc(std::max<long long>(n_total, 1)));
      PIPS_TRY(d_stage.alloc(std::max<long long>(n_total, 1)));
      PIPS_TRY(d_norms.alloc((size_t)3 * nblk));
      PIPS_TRY(h_norms.alloc((size_t)3 * nblk));
      PIPS_TRY(d_inertia.alloc((size_t)3 * nblk));
      HIP_TRY(hipMemset(d_inertia, 0, (size_t)3 * nblk * sizeof(int)));
      PIPS_TRY(d_bval.upload(h_bval));
      PIPS_TRY(d_kdst.upload(h_kdst));
      PIPS_TRY(d_bdst.upload(h_bdst));
      PIPS_TRY(d_kdiag.upload(h_kdiag));
      PIPS_TRY(d_kptr.upload(kptr));
      PIPS_TRY(d_psign_off.upload(h_psign_off));
      PIPS_TRY(d_perm_off.upload(h_perm_off));
      PIPS_TRY(d_rowbase.upload(h_rowbase));
      PIPS_TRY(d_bt_xoff.upload(h_bt_xoff));
      PIPS_TRY(d_sns.upload(h_sns));
      PIPS_TRY(d_blks.upload(h_blks));
      PIPS_TRY(d_rowidx.upload(h_rowidx));
      if (n_lb > 0) PIPS_TRY(d_lb_list.upload(h_lb_list));
      if (!h_leafdesc.empty()) PIPS_TRY(d_leafdesc.upload(h_leafdesc));
      if (lf_entries > 0) {   // the simple leaves' forward substitution as a gather
         PIPS_TRY(d_lf_rows.upload(h_lf_rows));
         PIPS_TRY(d_lf_ptr.upload(h_lf_ptr));
         PIPS_TRY(d_lf_src.upload(h_lf_src));
         PIPS_TRY(d_lf_pos.upload(h_lf_pos));
         PIPS_TRY(d_lf_val.alloc((size_t)lf_entries));
      }
      PIPS_TRY(d_upd.upload(h_upd));
      PIPS_TRY(d_spine.upload(h_spine));
      PIPS_TRY(d_spine_off.upload(h_spine_off));
      PIPS_TRY(d_sncol.upload(h_sncol));
      PIPS_TRY(d_bmap.upload(h_bmap));
      PIPS_TRY(d_perm.upload(h_perm));
      PIPS_TRY(d_psign.upload(h_psign));
      PIPS_TRY(d_krowptr.upload(h_krowptr));
      PIPS_TRY(d_kcolidx.upload(h_kcolidx));
      PIPS_TRY(d_bt_rowptr.upload(h_bt_rowptr));
      PIPS_TRY(d_bt_colidx.upload(h_bt_colidx));
      PIPS_TRY(d_bt_rowsc.upload(h_bt_rowsc));
      if (!h_br_rowptr.empty()) {   // the border by leaf row (k_border_mult_rows)
         PIPS_TRY(d_br_rowptr.upload(h_br_rowptr));
         PIPS_TRY(d_br_sc.upload(h_br_sc));
         PIPS_TRY(d_br_src.upload(h_br_src));
      }
      PIPS_TRY(d_nprimal.upload(h_nprimal));
      if (tail_first_touch) {   // (behind the others: the arenas keep their addresses)
         // a column of more than 64 KB of LDS: the kernel is told once per analysis, not per factorisation
         if ((size_t)ft_ld_max * sizeof(double) > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void*)k_tail_first_touch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(ft_ld_max * sizeof(double))));
         PIPS_TRY(d_ft_colbase.upload(h_ft_colbase));
         PIPS_TRY(d_ft_init_off.upload(h_ft_init_off));
         PIPS_TRY(d_ft_init.upload(h_ft_init));
         PIPS_TRY(d_ft_piece_off.upload(h_ft_piece_off));
         PIPS_TRY(d_ft_piece.upload(h_ft_piece));
         PIPS_TRY(d_ft_leaves.upload(h_ft_leaves));
      }
      return PIPS_OK;
   }

   ScatterCtx sx_atomic() const { return ScatterCtx{0, nullptr, nullptr, nullptr, nullptr}; }
   void launch_head_level(const LevelRange& L, double* SC, int ldSC, const ScatterCtx& sx) {
      if (L.simple_cnt > 0)
         hipLaunchKernelGGL(k_head_factor_simple, dim3((L.simple_cnt + 255) / 256), dim3(256), 0, stream, d_sns, L.simple_begin,
                            L.simple_cnt, d_blks, d_rowidx, d_upd, d_psign, d_psign_off, d_bmap, d_arena, SC, ldSC, d_inertia, d_pref, d_sctab, sx,
                            mf ? 1 : 0, d_mfLV, d_lf_pos, d_lf_val, d_arena, tail_first_touch ? 1 : 0);
      if (mf) return;
      if (L.small_cnt > 0)
         hipLaunchKernelGGL((k_head_factor<64, 8, 640>), dim3(L.small_cnt), dim3(64), (size_t)std::max(L.small_lds, 1) * sizeof(double), stream, d_sns,
                            L.small_begin, d_blks, d_rowidx, d_upd, d_psign, d_psign_off, d_bmap, d_arena, SC, ldSC, d_inertia, d_pref, d_sctab, sx,
                            L.small_lds);
      if (L.large_cnt > 0)   // the L21 cache is sized to the widest panel of this launch: small panels, many workgroups per compute unit
         hipLaunchKernelGGL((k_head_factor<256, 32, 6144>), dim3(L.large_cnt), dim3(256), (size_t)std::max(L.large_lds, 1) * sizeof(double), stream, d_sns,
                            L.large_begin, d_blks, d_rowidx, d_upd, d_psign, d_psign_off, d_bmap, d_arena, SC, ldSC,
                            d_inertia, d_pref, d_sctab, sx, L.large_lds);
   }
   template <int BLOCK, int WMAX, bool UG = false>
   int launch_front(const MfLaunch& m, double* SC, int ldSC) {
      const size_t lds = (size_t)m.lds_doubles * sizeof(double);
      if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)k_front<BLOCK, WMAX, UG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL((k_front<BLOCK, WMAX, UG>), dim3(m.cnt), dim3(BLOCK), lds, stream, d_sns, m.begin, d_blks, d_rowidx, d_mfint, d_psign,
                         d_psign_off, d_bmap, d_arena, d_mfU, SC, ldSC, d_inertia, d_pref, d_sctab, d_mfdbg, d_mfLV, d_kval, d_bval, deterministic ? 1 : 0, d_arena);
      return PIPS_OK;
   }
   int launch_border_schur(double* SC, int ldSC) {
      // LDS: packed nb x nb triangle + one staged batch + its rows' positions + the batch's supernode records
      constexpr int BLK = 512;
      const long long ncp = ((long long)bb_nbmax * (bb_nbmax + 1) / 2 + 1) & ~1LL;
      // (the triangle shared by 2 / 3 / 4 workgroups by column ranges, so that several fit a compute unit, measured 14.97 / 17.7 / 18.3 ms
      // against 14.94 on the 256-block chain's head: every part stages every batch - docs/HISTORY_r4.md; one workgroup holds it whole)
      constexpr int parts = 1;
      const long long c_cap = ncp;
      BbPlanSize z; z.stage = bb_stage; z.poscap = bb_poscap; z.nbmax = bb_nbmax;
      const size_t lds = bb_lds_bytes(z);
      if (!bb_fits(z))   // (analyze() has checked the same formula and taken the split off where it does not hold: an assertion)
         PIPS_FAIL(PIPS_ERR_STATE, "k_border_schur: %zu bytes of LDS for nb = %d (batch of %d doubles, %d rows)", lds, bb_nbmax, bb_stage, bb_poscap);
      // a block's batches are walked by `split` workgroups (each with its own accumulator): enough of them to fill the chip
      const int split = std::max(1, std::min(32, (bb_two_per_cu ? 512 : 256) / std::max(nblk, 1)));
      auto go = [&](auto kern, int cnt, const int* list, double* gb, long long gs, const int* grp, int sp, int ordered, double* out = nullptr,
                    long long out_stride = 0) -> int {
         if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
         hipLaunchKernelGGL(kern, dim3(cnt, sp, parts), dim3(BLK), lds, stream, list, d_bb_off, d_bb_batches, d_bb_meta, d_bb_pos, d_blks, d_bmap, d_arena, SC, ldSC,
                            d_sctab, gb, gs, grp, bb_stage, bb_poscap, ordered, out, out_stride, (int)c_cap);
         return PIPS_OK;
      };
      const bool small = bb_stage <= 2 * 3 * BLK;
      int rc = PIPS_OK;
      if (deterministic && d_gbuf && d_bb_round_blk) {
         // every block at once (each supernode list in its fixed order) into a triangle of its own, then the blocks of a group in order: a walk
         // takes as long for 8 workgroups as for 256, so one launch per round of blocks made the share's factorisation 230 ms
         const long long tri = (long long)ncp;
         if (!d_bb_out) PIPS_TRY(d_bb_out.alloc((size_t)std::max(nblk, 1) * tri));
         rc = small ? go(k_border_schur<BLK, 3>, nblk, (const int*)nullptr, (double*)nullptr, 0LL, (const int*)nullptr, 1, 1, d_bb_out, tri)
                    : go(k_border_schur<BLK, 6>, nblk, (const int*)nullptr, (double*)nullptr, 0LL, (const int*)nullptr, 1, 1, d_bb_out, tri);
         for (size_t k = 0; k + 1 < det.bb_round_off.size() && !rc; ++k) {
            const int cnt = det.bb_round_off[k + 1] - det.bb_round_off[k];
            if (cnt > 0)
               hipLaunchKernelGGL(k_border_schur_add, dim3(cnt, 8), dim3(256), 0, stream, d_bb_round_blk + det.bb_round_off[k], d_blks, d_bmap, d_bb_out, tri, ldSC, d_sctab,
                                  d_gbuf, det_gstride(), d_blk_group);
         }
      } else
         rc = small ? go(k_border_schur<BLK, 3>, nblk, (const int*)nullptr, (double*)nullptr, 0LL, (const int*)nullptr, split, deterministic ? 1 : 0)
                    : go(k_border_schur<BLK, 6>, nblk, (const int*)nullptr, (double*)nullptr, 0LL, (const int*)nullptr, split, deterministic ? 1 : 0);
      return rc;
   }
   int dump_front_clocks() {
      std::vector<long long> h((size_t)nsn_total * 8);
      HIP_TRY(hipStreamSynchronize(stream));
      HIP_TRY(hipMemcpy(h.data(), d_mfdbg, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
      static const char* names[7] = {"panel+zero", "stage ints", "leaf values + children", "leaf columns", "pivots", "update", "write-out"};
      for (const MfLaunch& m : mf_launches) {
         double ph[8] = {0}; long long nfs = 0, ws = 0;
         for (int i = m.begin; i < m.begin + m.cnt; ++i) {
            for (int q = 0; q < 7; ++q) ph[q] += (double)(h[(size_t)i * 8 + q + 1] - h[(size_t)i * 8 + q]);
            nfs += h_sns[i].w + h_sns[i].r; ws += h_sns[i].w;
         }
         fprintf(stderr, "[mf clocks] level %2d variant %d fronts %6d lds %6d  avg nf %5.1f w %4.1f | ", m.level, m.cls, m.cnt, m.lds_doubles * 8, (double)nfs / m.cnt, (double)ws / m.cnt);
         for (int q = 0; q < 7; ++q) fprintf(stderr, "%s %.1f%s", names[q], ph[q] / m.cnt * 0.01, q == 6 ? " us\n" : ", ");
      }
      return PIPS_OK;
   }
   // the border rows of the fronts of one level that hold the rows of K only (k_border_rows): a wave per pair - one wave per front where the
   // fronts of the level have a few pairs, four or eight where some have many
   void launch_border_rows(size_t l, hipStream_t st) {
      const int cnt = kb_level_off[l + 1] - kb_level_off[l];
      if (cnt == 0) return;
      const int* lst = d_kb_list + kb_level_off[l];
      if (kb_level_pairs[l] <= 3 || (cnt >= 16384 && kb_level_pairs[l] <= 8))   // (one wave for every level of >= 4096 fronts: head 17.5 against 16.6 ms)
         hipLaunchKernelGGL((k_border_rows<64, 16>), dim3(cnt), dim3(64), kb_level_lds[l], st, lst, d_sns, d_blks, d_rowidx, d_kb_rec, d_kb_off, d_arena, d_arena, d_bval);
      else if (cnt <= 4096 && kb_level_pairs[l] > 8)
         hipLaunchKernelGGL((k_border_rows<512, 16>), dim3(cnt), dim3(512), kb_level_lds[l], st, lst, d_sns, d_blks, d_rowidx, d_kb_rec, d_kb_off, d_arena, d_arena, d_bval);
      else
         hipLaunchKernelGGL((k_border_rows<256, 16>), dim3(cnt), dim3(256), kb_level_lds[l], st, lst, d_sns, d_blks, d_rowidx, d_kb_rec, d_kb_off, d_arena, d_arena, d_bval);
   }
   int launch_fronts(int level, double* SC, int ldSC) {
      int rc = PIPS_OK;
      for (const MfLaunch& m : mf_launches) {
         if (m.level != level) continue;
         switch (m.cls) {
            case 0: rc = launch_front<64, 16>(m, SC, ldSC); break;
            case 1: rc = launch_front<128, 16>(m, SC, ldSC); break;
            case 2: rc = launch_front<256, 16>(m, SC, ldSC); break;
            case 3: rc = launch_front<64, 32>(m, SC, ldSC); break;
            case 4: rc = launch_front<128, 32>(m, SC, ldSC); break;
            case 5: rc = launch_front<256, 32>(m, SC, ldSC); break;
            case 6: rc = launch_front<256, 32, true>(m, SC, ldSC); break;
            default: rc = launch_front<512, 32, true>(m, SC, ldSC); break;
         }
         if (rc) return rc;
      }
      return PIPS_OK;
   }
   void gather(const GatherList& g, const double* vals, double* target) {
      if (g.n_targets > 0)
         hipLaunchKernelGGL(k_gather_slots, dim3(grid_for(g.n_targets, 256)), dim3(256), 0, stream, g.n_targets, g.d_tgt, g.d_off, g.d_slots, vals, target);
   }

   int build_deterministic(int n_threads) {
      if (spine_total > 0) PIPS_FAIL(PIPS_ERR_STATE, "deterministic mode: spine kernels must be off");
      const int nlev = (int)levels.size();
      g_levels = std::vector<GatherList>(nlev);
      gv_levels = std::vector<GatherList>(nlev);
      int rc = PIPS_OK;
      // ---- factorisation scatter: record where every slot goes (structure only; the numbers this pass produces are discarded)
      std::vector<long long> rec((size_t)std::max<long long>(slots_total, 1), -1);
      if (slots_total > 0) {
         DevBuf<long long> d_rec;
         PIPS_TRY(d_rec.alloc((size_t)slots_total));
         HIP_TRY(hipMemsetAsync(d_rec, 0xff, (size_t)slots_total * sizeof(long long), stream));
         double* fakeSC = d_arena;   // only offsets relative to it are formed (S > 0 blocks have border rows; none in Schur mode 2, whose heads have no border)
         const ScatterCtx sx{1, d_rec, nullptr, d_arena, fakeSC};
         for (const LevelRange& L : levels) launch_head_level(L, fakeSC, S, sx);
         HIP_TRY(hipGetLastError());
         HIP_TRY(hipStreamSynchronize(stream));
         HIP_TRY(hipMemcpy(rec.data(), d_rec, (size_t)slots_total * sizeof(long long), hipMemcpyDeviceToHost));
         d_rec.reset();
         PIPS_TRY(d_slot_val.alloc((size_t)slots_total));
      }
      {  // the slots by target: head panels level by level, tails, Schur complement (detplan.h)
         FactorSlotPlan fp;
         if ((rc = classify_factor_slots(rec, SCATTER_SC_FLAG, *this, sym, fp))) return rc;
         std::vector<long long>().swap(rec);
         for (int l = 0; l < nlev; ++l) PIPS_TRY(g_levels[l].upload(fp.levels[l]));
         PIPS_TRY(g_tail.upload(fp.tail));
         PIPS_TRY(g_sc.upload(fp.sc));
         sc_kept = std::move(fp.kept);
      }
      // ---- forward-substitution scatter: same recording, targets are entries of the permuted work vector
      if (vslots_total > 0) {
         DevBuf<long long> d_rec;
         PIPS_TRY(d_rec.alloc((size_t)vslots_total));
         HIP_TRY(hipMemsetAsync(d_rec, 0xff, (size_t)vslots_total * sizeof(long long), stream));
         const ScatterCtx sxv{1, d_rec, nullptr, d_xw, nullptr};
         for (const LevelRange& L : levels) {
            // (the simple leaves own no slots where their forward substitution is the gather by target row: fixed order by construction)
            if (L.simple_cnt > 0 && lf_rows == 0)
               hipLaunchKernelGGL(k_head_solve_simple, dim3((L.simple_cnt + 255) / 256, 1), dim3(256), 0, stream, d_sns, L.simple_begin,
                                  L.simple_cnt, d_blks, d_rowidx, d_arena, d_xw, 0LL, 0, sxv);
            const int begin = L.small_cnt > 0 ? L.small_begin : L.large_begin;
            const int cnt = L.small_cnt + L.large_cnt;
            if (cnt > 0) hipLaunchKernelGGL(k_head_fwd, dim3(cnt, 1), dim3(64), 0, stream, d_sns, begin, d_blks, d_rowidx, d_arena, d_xw, 0LL, sxv);
         }
         HIP_TRY(hipGetLastError());
         HIP_TRY(hipStreamSynchronize(stream));
         std::vector<long long> vrec((size_t)vslots_total);
         HIP_TRY(hipMemcpy(vrec.data(), d_rec, (size_t)vslots_total * sizeof(long long), hipMemcpyDeviceToHost));
         d_rec.reset();
         PIPS_TRY(d_vslot_val.alloc((size_t)vslots_total));
         SolveSlotPlan vp;
         classify_solve_slots(vrec, *this, sym, vp);
         for (int l = 0; l < nlev; ++l) PIPS_TRY(gv_levels[l].upload(vp.levels[l]));
         PIPS_TRY(gv_tail.upload(vp.tail));
      }
      (void)n_threads;
      return PIPS_OK;
   }

   // Sparse Schur complement: tab holds, block after block, the nb x nb table "position of entry (la, lb), la >= lb, of this
   // block's contribution inside the value array of SC's lower-triangular CSR"; factor(values, 0) then accumulates there.
   // la / lb count the block's non-empty border columns (border_pack(): BlockSym::bmap is empty where the border stayed out of the
   // symbolic analysis).  Schur mode 2: the blocked solves run packed by these local columns (schur_by_packed_solves); their per-row
   // tables are built here, once.
   const SchurPack& border_pack() {
      if (pack.off.empty()) build_schur_pack(in, S, pack);
      return pack;
   }
   int set_sc_tables(const std::vector<int>& tab, const std::vector<long long>& off, long long sc_nnz) {
      if (!analyzed) PIPS_FAIL(PIPS_ERR_STATE, "set_sc_tables: analyze first");
      HIP_TRY(hipSetDevice(device));
      int rc = d_sctab.upload(tab);
      if (rc) return rc;
      for (int b = 0; b < nblk; ++b) h_blks[b].sctab_off = off[b];
      HIP_TRY(hipMemcpy(d_blks, h_blks.data(), (size_t)nblk * sizeof(BlkDesc), hipMemcpyHostToDevice));
      sc_len = sc_nnz;
      packed_rhs = 0;
      if (schur_mode_eff == 2) {
         const SchurPack& pk = border_pack();
         if (pk.nb_max >= (1 << 24)) PIPS_FAIL(PIPS_ERR_STATE, "set_sc_tables: %d border columns in one block exceed the packed solves' 2^24", pk.nb_max);
         if ((rc = schur_pack_rows(in, S, off, (long long)tab.size(), h_pk_rows))) return rc;
         if ((long long)h_pk_rows.la.size() != bt_rows_total)
            PIPS_FAIL(PIPS_ERR_STATE, "set_sc_tables: %zu border rows, the analysis holds %lld", h_pk_rows.la.size(), bt_rows_total);
         PIPS_TRY(d_pk_la.upload(h_pk_rows.la));
         PIPS_TRY(d_pk_tabrow.upload(h_pk_rows.tabrow));
         if (deterministic) h_pk_tab = tab;   // (build_det_group_plan builds the lists of k_border_tmult_chunk_packed_det from them)
         else h_pk_rows = PackRows();
         packed_rhs = pk.nb_max;
      }
      if (head_slots) {   // the Schur targets of the head moved into the CSR value array: record again
         g_levels.clear(); gv_levels.clear();
         g_tail = GatherList(); g_sc = GatherList(); gv_tail = GatherList();
         d_slot_val.reset(); d_vslot_val.reset(); d_mvslot.reset();
         if ((rc = build_deterministic(1))) return rc;
      }
      return PIPS_OK;
   }

   // ---- numeric factorisation: factor() calls the stages below in this order
   // block maxima and thresholds, the arena cleared and filled with the values of K (and of the border), the reference magnitudes of the pivots
   int factor_prologue() {
      PhaseTimer::Scope phase(&timer, stream, 0);
      hipLaunchKernelGGL(k_block_absmax_init, dim3((nblk + 255) / 256), dim3(256), 0, stream, d_blks, nblk);
      hipLaunchKernelGGL(k_block_absmax, dim3(std::max(1, std::min(64, (int)(nnzK_total / nblk / 4096))), nblk), dim3(256), 0, stream, d_kval,
                         d_kptr, d_blks);
      hipLaunchKernelGGL(k_block_absmax_finish, dim3((nblk + 255) / 256), dim3(256), 0, stream, d_blks, nblk, thr_rel, repl_rel);
      // multifrontal head: no panel of the head is read before it is written (simple leaves: every entry of the panel is an entry of K or
      // of the border and comes with k_scatter; fronts: assembled in LDS, written out whole) - only the tails are cleared
      // (first touch of the tails: k_tail_first_touch writes every tail column once, assembled, after the head - no clear, no padding diagonal here)
      if (!tail_first_touch) hipLaunchKernelGGL(k_arena_clear, dim3(256, nblk), dim3(256), 0, stream, d_blks, d_arena, mf ? 1 : 0);
      HIP_TRY(hipMemsetAsync(d_inertia, 0, (size_t)3 * nblk * sizeof(int), stream));
      if (!d_gemm_ctr) PIPS_TRY(d_gemm_ctr.alloc((size_t)GEMM_CTR_SLOTS * 8));
      HIP_TRY(hipMemsetAsync(d_gemm_ctr, 0, (size_t)GEMM_CTR_SLOTS * 8 * sizeof(int), stream));
      gemm_ctr_cursor = 0;
      if (nnzK_total > 0)
         hipLaunchKernelGGL(k_scatter, dim3(grid_for(nnzK_total, 256)), dim3(256), 0, stream, d_kdst, d_kval, d_arena, nnzK_total);
      if (nnzB_total > 0 && schur_mode_eff == 1)
         hipLaunchKernelGGL(k_scatter, dim3(grid_for(nnzB_total, 256)), dim3(256), 0, stream, d_bdst, d_bval, d_arena, nnzB_total);
      if (!tail_first_touch) hipLaunchKernelGGL(k_tail_pad_diag, dim3(nblk), dim3(128), 0, stream, d_blks, d_arena, nblk);
      hipLaunchKernelGGL(k_pref_rows, dim3(32, nblk), dim3(256), 0, stream, d_blks, d_kval, d_kdiag, d_res, d_nprimal, d_krowptr, d_kcolidx);   // (d_res: scratch of the solves)
      hipLaunchKernelGGL(k_pref_init, dim3(32, nblk), dim3(256), 0, stream, d_blks, d_perm, d_perm_off, (const double*)d_res, d_pref);
      return PIPS_OK;
   }
   // the last update matrices of the fronts: into the tail and the Schur complement, front by front
   void launch_root_assemble(double* SC, int ldSC) {
      // about 2048 workgroups in the launch (what is resident at once): half of a block's chunks on the tail's columns, half on the border's
      const int asm_half = std::max(1, std::min(32, 1024 / std::max(nblk, 1)));
      if (tail_first_touch) {   // the tails were assembled column by column (launch_tail_first_touch): only the border x border part is left
         if (SC && n_roots > 0)
            hipLaunchKernelGGL(k_root_assemble, dim3(nblk, asm_half), dim3(256), 0, stream, (const int*)nullptr, d_root_off, d_roots, d_sns, d_blks, d_rowidx, d_bmap,
                               d_arena, d_mfU, SC, ldSC, d_sctab, (double*)nullptr, 0LL, (const int*)nullptr, 0, asm_half);
         return;
      }
      if (deterministic && d_gbuf && SC && d_round_blk) {
         for (size_t k = 0; k + 1 < det.round_off.size(); ++k) {
            const int cnt = det.round_off[k + 1] - det.round_off[k];
            if (cnt > 0)
               hipLaunchKernelGGL(k_root_assemble, dim3(cnt, 2 * asm_half), dim3(256), 0, stream, d_round_blk + det.round_off[k], d_root_off, d_roots, d_sns, d_blks, d_rowidx,
                                  d_bmap, d_arena, d_mfU, SC, ldSC, d_sctab, d_gbuf, det_gstride(), d_blk_group, asm_half, asm_half);
         }
      } else
         hipLaunchKernelGGL(k_root_assemble, dim3(nblk, 2 * asm_half), dim3(256), 0, stream, (const int*)nullptr, d_root_off, d_roots, d_sns, d_blks, d_rowidx, d_bmap,
                            d_arena, d_mfU, SC, ldSC, d_sctab, (double*)nullptr, 0LL, (const int*)nullptr, asm_half, asm_half);
   }
   // first touch of the tails: every tail column written once - the entries of K and of the border, the padding diagonal, the root fronts'
   // update matrices - and then the products of the simple leaves that have no front above them
   int launch_tail_first_touch(double* SC, int ldSC) {
      const size_t lds = (size_t)ft_ld_max * sizeof(double);
      hipLaunchKernelGGL(k_tail_first_touch, dim3(ft_cols_max, nblk), dim3(64), lds, stream, d_blks, d_ft_colbase, d_ft_init_off, d_ft_init, d_ft_piece_off,
                         d_ft_piece, d_rowidx, d_kval, d_bval, d_mfU, d_arena);
      if (n_ft_leaves > 0)
         hipLaunchKernelGGL(k_leaf_products, dim3((n_ft_leaves + 255) / 256), dim3(256), 0, stream, d_ft_leaves, n_ft_leaves, d_sns, d_blks, d_rowidx, d_bmap,
                            d_arena, SC, ldSC, d_sctab);
      return PIPS_OK;
   }
   // the head by levels, then what follows from its finished panels; one phase-1 record per level and per stage that runs
   int factor_head(double* SC, int ldSC) {
      const ScatterCtx sx = head_slots ? ScatterCtx{2, nullptr, d_slot_val, d_arena, SC} : sx_atomic();
      for (size_t li = 0; li < levels.size(); ++li) {
         PhaseTimer::Scope phase(&timer, stream, 1);
         if (head_slots) gather(g_levels[li], d_slot_val, d_arena);   // contributions of the lower levels, in fixed order
         launch_head_level(levels[li], SC, ldSC, sx);
         if (mf) PIPS_TRY(launch_fronts((int)li, SC, ldSC));
      }
      if (head_slots) {
         PhaseTimer::Scope phase(&timer, stream, 1);
         gather(g_tail, d_slot_val, d_arena);
         if (SC && deterministic && d_gbuf) {
            HIP_TRY(hipMemsetAsync(d_gbuf, 0, (size_t)det.n_groups * det_gstride() * sizeof(double), stream));
            gather(g_sc_grp, d_slot_val, d_gbuf);
         } else if (SC) gather(g_sc, d_slot_val, SC);
      }
      if (tail_first_touch) { PhaseTimer::Scope phase(&timer, stream, 1); PIPS_TRY(launch_tail_first_touch(SC, ldSC)); }
      if (mf && n_roots > 0) { PhaseTimer::Scope phase(&timer, stream, 1); launch_root_assemble(SC, ldSC); }
      if (mf && d_kb_list) {   // fronts on the rows of K only: their border rows now, level by level, from the finished panels; then the head's part
                               // of the dense tail's border rows.  (Forming level l on a second stream beside the fronts above it, which need
                               // nothing of it, was measured: no gain, 17.4 against 16.7 ms of head on the configs[3] share.)
         PhaseTimer::Scope phase(&timer, stream, 1);
         for (size_t l = 0; l + 1 < kb_level_off.size(); ++l) launch_border_rows(l, stream);
         if (n_kb_tail > 0) hipLaunchKernelGGL(k_border_tail<16>, dim3(n_kb_tail), dim3(64), 0, stream, d_kb_tail, d_sns, d_blks, d_rowidx, d_arena);
      }
      // border split: the border x border part of every block's Schur contribution, from the finished panels
      if (mf && n_bb > 0 && SC) { PhaseTimer::Scope phase(&timer, stream, 1); PIPS_TRY(launch_border_schur(SC, ldSC)); }
      if (spine_total > 0) {
         PhaseTimer::Scope phase(&timer, stream, 1);
         hipLaunchKernelGGL((k_head_factor_spine<256, 32, 6144>), dim3(nblk), dim3(256), 0, stream, d_spine, d_spine_off, d_sns, d_blks,
                            d_rowidx, d_upd, d_psign, d_psign_off, d_bmap, d_arena, SC, ldSC, d_inertia, d_pref, d_sctab);
      }
      if (mf && knob_set<K_MF_CLOCKS>()) {
         if (!d_mfdbg) PIPS_TRY(d_mfdbg.alloc((size_t)std::max(nsn_total, 1) * 8));
         else PIPS_TRY(dump_front_clocks());
      }
      hipLaunchKernelGGL(k_pref_tail, dim3(8, nblk), dim3(256), 0, stream, d_blks, d_arena, d_pref, 0);
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   // the tails, and with Schur mode 2 the leaves' Schur contribution by blocked solves
   int factor_tail(double* SC, int ldSC) {
      TailCtx c = ctx();
      c.timer = &timer;                           // (the tail's phase records belong to the factorisation: the solves leave it out)
      c.det_reduce_later = schur_mode_eff == 2;   // (deterministic mode 2: the group buffers are filled by schur_by_solves, below)
      PIPS_TRY(tail_factor(c, SC, ldSC));
      factored = true;
      perturbed_cache = -1;
      if (SC && schur_mode_eff == 2 && !schur_cols.empty()) {
         const int rec_schur = timer.begin_i(stream, 5);   // (stays open across the records of the solves inside: solve_once times its sweeps)
         const int rc = schur_by_solves(SC, ldSC);
         timer.end_i(rec_schur, stream);
         if (rc) return rc;
      }
      if (SC && c.det_rounds && c.det_reduce_later) reduce_det_groups(c, SC, ldSC);   // one fixed-tree add, after every chunk
      return PIPS_OK;
   }
   // The inertia counters go to pinned host memory behind the factorisation (fetch_inertia waits for the event only)
   int post_inertia() {
      h_amax.clear();
      if (!h_inertia_pin) {
         PIPS_TRY(h_inertia_pin.alloc((size_t)(3 * nblk + 1)));
         h_inertia_pin[3 * nblk] = 0;
         HIP_TRY(hipEventCreateWithFlags(&ev_inertia, hipEventDisableTiming));
      }
      HIP_TRY(hipMemcpyAsync(h_inertia_pin, d_inertia, (size_t)3 * nblk * sizeof(int), hipMemcpyDeviceToHost, stream));
      if (tail_single)   // (the error word of the single-launch tail factorisation travels with the counters)
         HIP_TRY(hipMemcpyAsync(h_inertia_pin + 3 * nblk, tsingle.d_ctl + 9, sizeof(int), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipEventRecord(ev_inertia, stream));
      inertia_in_flight = true;
      inertia_on_host = false;
      return PIPS_OK;
   }
   int factor(double* SC, int ldSC) {
      if (!analyzed) PIPS_FAIL(PIPS_ERR_STATE, "factor called before analyze");
      HIP_TRY(hipSetDevice(device));
      if (deterministic && SC && S > 0 && !d_gbuf && d_blk_group)
         PIPS_TRY(d_gbuf.alloc((size_t)det.n_groups * det_gstride()));
      timer.reset();
      const int rec_total = timer.begin_i(stream, 6);   // the whole factorisation: stays open across the records of the stages
      PIPS_TRY(factor_prologue());
      PIPS_TRY(factor_head(SC, ldSC));
      PIPS_TRY(factor_tail(SC, ldSC));
      timer.end_i(rec_total, stream);
      return post_inertia();
   }

   // SC -= sum_b Br_b^T K_b^-1 Br_b, chunk by chunk of 32 border columns: densify, solve (all blocks at once), multiply back.
   // Deterministic mode: into the group buffers instead (k_border_tmult_chunk_det; Engine::factor adds them in the fixed tree afterwards), the
   // chunk solved by the atomics-free sweeps - one interleaved panel (solve_once_multi, whole-panel slicing whatever the launch size) where its
   // forward-substitution slots fit, else column by column.  A column's solution then depends on its own right-hand side only, not on the lane
   // or chunk it lands in nor on the other blocks, so its bits do not change with the rank count
   int schur_by_solves(double* SC, int ldSC) {
      int rc = ensure_multi_buffers();
      if (rc) return rc;
      const bool det = deterministic && d_gbuf;
      const bool det_panel = det && det_panel_fits();
      if (det_panel && !d_mvslot) PIPS_TRY(d_mvslot.alloc((size_t)std::max<long long>(vslots_total, 1) * MQ));
      if (packed_rhs > 0) return schur_by_packed_solves(SC, det, det_panel);
      if (det && ldSC != S) PIPS_FAIL(PIPS_ERR_ARG, "deterministic mode, Schur mode 2: ldSC %d must equal S %d (the group buffers are S x S)", ldSC, S);
      const int bs = 32, ncols = (int)schur_cols.size();
      for (int c0 = 0; c0 < ncols; c0 += bs) {
         const int nr = std::min(bs, ncols - c0);
         HIP_TRY(hipMemsetAsync(d_mx_rhs, 0, (size_t)nr * n_total * sizeof(double), stream));
         hipLaunchKernelGGL(k_border_rows_to_dense, dim3(grid_for(bt_rows_total, 256)), dim3(256), 0, stream, d_bt_rowptr, d_bt_colidx,
                            d_bval, d_bt_rowsc, d_bt_xoff, d_schur_slot, c0, nr, d_mx_rhs, n_total, bt_rows_total);
         if ((rc = solve_chunk(d_mx_rhs, nr, det, det_panel))) return rc;
         if (det) {
            if (g_btm_grp.n_targets > 0)
               hipLaunchKernelGGL(k_border_tmult_chunk_det, dim3(grid_for(g_btm_grp.n_targets * 32, 256)), dim3(256), 0, stream, g_btm_grp.n_targets,
                                  g_btm_grp.d_tgt, g_btm_grp.d_off, g_btm_grp.d_slots, d_bt_rowptr, d_bt_colidx, d_bval, d_bt_xoff, d_schur_cols + c0, nr,
                                  d_mx_rhs, n_total, d_gbuf, det_gstride(), S, ldSC);
            continue;
         }
         hipLaunchKernelGGL(k_border_tmult_chunk, dim3(grid_for(bt_rows_total, 256, 1024), nr), dim3(256), 0, stream, d_bt_rowptr,
                            d_bt_colidx, d_bval, d_bt_rowsc, d_bt_xoff, d_schur_cols + c0, nr, d_mx_rhs, n_total, SC, ldSC,
                            bt_rows_total);
      }
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   // The same into the value array of the sparse Schur complement (set_sc_tables), the border columns packed block by block: chunks of 32
   // LOCAL columns - right-hand side q holds every block's q-th non-empty border column, so packed_rhs = max_b nb_b right-hand sides
   // instead of one per distinct Schur column (2-link borders: n0 plus two pairs' linking rows, whatever the number of blocks).  Same
   // clear, same choice of sweeps as above; the three kernels address by local column (kernels.hip.h, k_border_tmult_chunk_packed)
   int schur_by_packed_solves(double* values, bool det, bool det_panel) {
      int rc = PIPS_OK;
      const int bs = 32;
      for (int q0 = 0; q0 < packed_rhs; q0 += bs) {
         const int nr = std::min(bs, packed_rhs - q0);
         HIP_TRY(hipMemsetAsync(d_mx_rhs, 0, (size_t)nr * n_total * sizeof(double), stream));
         hipLaunchKernelGGL(k_border_rows_to_dense_packed, dim3(grid_for(bt_rows_total, 256)), dim3(256), 0, stream, d_bt_rowptr, d_bt_colidx,
                            d_bval, d_bt_xoff, d_pk_la, q0, nr, d_mx_rhs, n_total, bt_rows_total);
         if ((rc = solve_chunk(d_mx_rhs, nr, det, det_panel))) return rc;
         if (det) {
            if (g_pk_grp.n_targets > 0)
               hipLaunchKernelGGL(k_border_tmult_chunk_packed_det, dim3(grid_for(g_pk_grp.n_targets, 256)), dim3(256), 0, stream, g_pk_grp.n_targets,
                                  g_pk_grp.d_tgt, g_pk_grp.d_off, g_pk_grp.d_slots, d_bt_rowptr, d_bt_colidx, d_bval, d_bt_xoff, q0, nr, d_mx_rhs,
                                  n_total, d_gbuf);
            continue;
         }
         hipLaunchKernelGGL(k_border_tmult_chunk_packed, dim3(grid_for(bt_rows_total, 256, 1024), nr), dim3(256), 0, stream, d_bt_rowptr,
                            d_bt_colidx, d_bval, d_bt_xoff, d_pk_la, d_pk_tabrow, d_sctab, q0, nr, d_mx_rhs, n_total, values, bt_rows_total);
      }
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   // nr <= 32 right-hand sides, contiguous at X, by the sweeps that suit them (work vectors: d_mx_xw).  det: the atomics-free sweeps - one
   // interleaved panel with whole-panel slicing whatever the launch size (det_panel: d_mvslot holds its slots), else column by column.
   // Otherwise the interleaved sweep from use_multi's threshold on, below it the per-right-hand-side sweeps
   int solve_chunk(double* X, int nr, bool det, bool det_panel) {
      if (det_panel) return solve_once_multi(X, nr, n_total, d_mx_xw, 1);
      if (det) {
         int rc = PIPS_OK;
         for (int r = 0; r < nr && !rc; ++r) rc = solve_once(X + (long long)r * n_total);
         return rc;
      }
      return use_multi(nr) ? solve_once_multi(X, nr, n_total, d_mx_xw) : solve_once(X, nr, n_total, d_mx_xw);
   }
   // deterministic blocked solves: the slots of one interleaved panel (MQ doubles per forward-substitution contribution of the head) within 4 GB, as
   // solve_multi's budget.  (A rank's contributions are a part of the one-rank total: where one rank takes the panels, every rank count does)
   bool det_panel_fits() const { return head_slots && (double)std::max<long long>(vslots_total, 1) * MQ * sizeof(double) <= 4e9; }

   // workgroups per block of the vector norms: slices of about 16 K rows, the launch kept near the number resident at once
   int absmax_chunks() const { return (int)std::max<long long>(1, std::min<long long>(std::min<long long>(64, 2048 / std::max(nblk, 1) + 1), n_total / std::max(nblk, 1) / 16384 + 1)); }
   // ---- the head levels of a solve sweep: one walk per direction, on nrhs work vectors at xw + r * xws (the callers keep their own
   //      prologue, tail sweep and timer phases) ----
   // Forward substitution.  sx says where a supernode's contributions go.  Mode 0: atomics on the work vector (the chain kernels, any nrhs).
   // Mode 2, one right-hand side: without atomics - the contributions go to their slots (sx.val), every level first gathers what the lower
   // levels left for its own columns, the tail rows are gathered before the dense sweep.  border: the border slots of the augmented factor
   // are targets too (atomics, one right-hand side): the chain kernels take their own border rows, k_leaf_border those of the simple leaves.
   // (The spine kernels know neither slots nor border rows: deterministic mode refuses spines, aug_sweeps_ok needs spine_total == 0.)
   void head_forward(double* xw, int nrhs, long long xws, const ScatterCtx& sx, int border) {
      const bool slots = sx.mode == 2;
      for (size_t li = 0; li < levels.size(); ++li) {
         const LevelRange& L = levels[li];
         if (slots) gather(gv_levels[li], sx.val, xw);
         if (L.simple_cnt > 0 && lf_rows > 0)   // the leaves' columns are final as they stand: every target row collects its sum
            hipLaunchKernelGGL(k_leaf_fwd_gather, dim3((unsigned)((lf_rows + 255) / 256), nrhs), dim3(256), 0, stream, d_lf_rows, d_lf_ptr, d_lf_src,
                               d_lf_val, xw, xws, (int)lf_rows);
         else if (L.simple_cnt > 0)
            hipLaunchKernelGGL(k_head_solve_simple, dim3((L.simple_cnt + 255) / 256, nrhs), dim3(256), 0, stream, d_sns, L.simple_begin,
                               L.simple_cnt, d_blks, d_rowidx, d_arena, xw, xws, 0, sx);
         if (border && L.simple_cnt > 0 && n_lb > 0)
            hipLaunchKernelGGL(k_leaf_border, dim3((n_lb + 255) / 256), dim3(256), 0, stream, d_lb_list, n_lb, d_sns, d_blks, d_rowidx, d_arena, xw, 0);
         // small and large supernodes of one level are contiguous in d_sns
         const int begin = L.small_cnt > 0 ? L.small_begin : L.large_begin;
         const int cnt = L.small_cnt + L.large_cnt;
         if (cnt > 0 && slots)
            hipLaunchKernelGGL(k_head_fwd, dim3(cnt, 1), dim3(64), 0, stream, d_sns, begin, d_blks, d_rowidx, d_arena, xw, 0LL, sx);
         else if (cnt > 0)
            hipLaunchKernelGGL(head_wcap <= 16 ? k_head_fwd_chain<16> : k_head_fwd_chain<HEAD_WMAX>, dim3(cnt, nrhs), dim3(64), 0, stream, d_sns, begin,
                               d_blks, d_rowidx, d_arena, xw, xws, border);
      }
      if (slots) gather(gv_tail, sx.val, xw);
      if (spine_total > 0)
         hipLaunchKernelGGL(k_head_solve_spine, dim3(nblk, nrhs), dim3(64), 0, stream, d_spine, d_spine_off, d_sns, d_blks, d_rowidx,
                            d_arena, xw, xws, 0);
   }
   // Backward substitution.  border: the border slots of the work vector hold the root solution and the border rows of the factor take part.
   // dscale: D^-1 of the head columns inside the kernels (they read the diagonal's cache line anyway) - not with spines, whose kernel has no
   // such argument.  The simple leaves: from their compact records (k_leaf_bwd: it stops at the border) where the layout has them, their
   // border rows then by k_leaf_border; leaf_border_inline: instead k_head_solve_simple walks a leaf's rows, border included, in one sum.
   void head_backward(double* xw, int nrhs, long long xws, int border, int dscale, bool leaf_border_inline = false) {
      if (spine_total > 0)
         hipLaunchKernelGGL(k_head_solve_spine, dim3(nblk, nrhs), dim3(64), 0, stream, d_spine, d_spine_off, d_sns, d_blks, d_rowidx,
                            d_arena, xw, xws, 1, border);
      const int inline_border = border && leaf_border_inline ? 1 : 0;
      for (int l = (int)levels.size() - 1; l >= 0; --l) {
         const LevelRange& L = levels[l];
         const int begin = L.small_cnt > 0 ? L.small_begin : L.large_begin;
         const int cnt = L.small_cnt + L.large_cnt;
         if (cnt > 0)
            hipLaunchKernelGGL(head_wcap <= 16 ? k_head_bwd_chain<16> : k_head_bwd_chain<HEAD_WMAX>, dim3(cnt, nrhs), dim3(64), 0, stream, d_sns, begin,
                               d_blks, d_rowidx, d_arena, xw, xws, border, dscale);
         if (L.simple_cnt > 0 && d_leafdesc && !inline_border)
            hipLaunchKernelGGL(k_leaf_bwd, dim3((L.simple_cnt + 255) / 256, nrhs), dim3(256), 0, stream, d_leafdesc, L.simple_cnt, d_rowidx, d_arena,
                               xw, xws, dscale);
         else if (L.simple_cnt > 0)
            hipLaunchKernelGGL(k_head_solve_simple, dim3((L.simple_cnt + 255) / 256, nrhs), dim3(256), 0, stream, d_sns, L.simple_begin,
                               L.simple_cnt, d_blks, d_rowidx, d_arena, xw, xws, 1, sx_atomic(), inline_border, 0, dscale);
         if (border && !inline_border && L.simple_cnt > 0 && n_lb > 0)
            hipLaunchKernelGGL(k_leaf_border, dim3((n_lb + 255) / 256), dim3(256), 0, stream, d_lb_list, n_lb, d_sns, d_blks, d_rowidx, d_arena, xw, 1);
      }
   }

   // nrhs right-hand sides at x_dev + r * x_stride (flat over all blocks each); work vectors at xw + r * xw_total
   int solve_once(double* x_dev, int nrhs = 1, long long x_stride = 0, double* xw = nullptr) {
      if (deterministic && nrhs != 1) PIPS_FAIL(PIPS_ERR_STATE, "deterministic mode solves one right-hand side at a time");
      if (!xw) xw = d_xw;
      const long long xws = nrhs > 1 ? xw_total : 0;
      const dim3 pg(64, nblk, nrhs);
      { PhaseTimer::Scope phase(&timer, stream, 7); hipLaunchKernelGGL(k_permute_in, pg, dim3(256), 0, stream, d_blks, d_perm, d_perm_off, x_dev, x_stride, xw, xws); }
      {
         PhaseTimer::Scope phase(&timer, stream, 8);
         head_forward(xw, nrhs, xws, deterministic && head_slots ? ScatterCtx{2, nullptr, d_vslot_val, xw, nullptr} : sx_atomic(), 0);
      }
      // D^-1 of the head columns: fused into the backward kernels of the common path (chain kernels + thread-per-leaf kernel: they
      // read the diagonal's cache line anyway; the separate pass reads 88 bytes of descriptor per supernode - 12.9 M of them on the
      // configs[3] share); with spines (their kernel does not scale) the pass stays
      const bool fused_d = spine_total == 0;
      {
         PhaseTimer::Scope phase(&timer, stream, 9);
         const TailCtx c = ctx();
         PIPS_TRY(tail_fwd(c, xw, nrhs, xws));
         if (nsn_total > 0 && !fused_d)
            hipLaunchKernelGGL(k_head_dscale, dim3(grid_for(nsn_total, 256), nrhs), dim3(256), 0, stream, d_sns, nsn_total, d_blks,
                               d_arena, xw, xws, 0);
         PIPS_TRY(tail_bwd(c, xw, nrhs, xws));
      }
      { PhaseTimer::Scope phase(&timer, stream, 10); head_backward(xw, nrhs, xws, 0, fused_d ? 1 : 0); }
      { PhaseTimer::Scope phase(&timer, stream, 7); hipLaunchKernelGGL(k_permute_out, pg, dim3(256), 0, stream, d_blks, d_perm, d_perm_off, x_dev, x_stride, xw, xws); }
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }

   // The interleaved multi-vector sweep reads every entry of L once per panel of 32 right-hand sides instead of once per right-hand side
   // and multiplies on the matrix pipe; the per-right-hand-side sweeps (grid.y = right-hand side) re-read L each time.  Round 2 measured
   // one config-2 block, 256 rhs: 11 ms separate / 43 ms interleaved - with a scalar multiply-add loop in the tile kernels; with the
   // matrix-pipe tiles and all panels in every launch the interleaved sweep wins from a few right-hand sides on.
   // PIPS_HIP_MULTI, read at every call (tests change it between the solves of one process).  Not set: the rule above, and solve_once_multi
   // slices its tail sweeps by the launch size.  0: never interleaved.  Any other value: from two right-hand sides on; 2 also takes whole
   // panels whatever the size, 4 half panels
   struct MultiKnob { int from; int slices; };   // fewest right-hand sides of an interleaved sweep (0 = never); forced slicing (0 = none)
   static MultiKnob multi_knob() {
      const bool given = knob_set<K_MULTI>();
      const int v = (int)knob_int<K_MULTI>();
      return MultiKnob{!given ? 8 : v != 0 ? 2 : 0, v == 2 ? 1 : v == 4 ? 2 : 0};
   }
   bool use_multi(int nr) const {
      const int from = multi_knob().from;
      return from > 0 && nr >= from;
   }

   // nr right-hand sides at X + q * x_stride in one interleaved sweep (kernels.hip.h "multi-vector solves"): panels of MQ, every launch
   // takes all of them (grid.y / grid.z); xm holds ceil(nr / MQ) * MQ * xw_total doubles
   int solve_once_multi(double* X, int nr, long long x_stride, double* xm, int pin_slices = 0) {
      const int np = (nr + MQ - 1) / MQ;
      const long long ps = (long long)MQ * xw_total;
      const dim3 pg(64, nblk, np);
      hipLaunchKernelGGL(k_mpermute, pg, dim3(256), 0, stream, d_blks, d_perm, d_perm_off, X, x_stride, nr, xm, 0, ps);
      auto head = [&](const LevelRange& L, int backward) {
         const int cnt = L.simple_cnt + L.small_cnt + L.large_cnt;   // contiguous: sorted by (level, class)
         if (cnt == 0) return;
         const int begin = L.simple_cnt > 0 ? L.simple_begin : (L.small_cnt > 0 ? L.small_begin : L.large_begin);
         hipLaunchKernelGGL(k_mhead, dim3((cnt + 3) / 4, np), dim3(256), 0, stream, d_sns, begin, cnt, d_blks, d_rowidx, d_arena, xm, backward, ps);
      };
      if (deterministic) {
         // forward substitution without atomics, like solve_once's: every contribution of a supernode goes to its slot (MQ right-hand sides
         // wide: d_mvslot, one panel at a time), every level first takes what the lower levels left for its columns, in the recorded order;
         // the simple leaves by target row where that list exists.  One panel per call (the caller cuts the right-hand sides into panels).
         // (k_mgather_slots / k_mleaf_fwd_gather take one target per 32 threads and no grid stride: their grids are not capped - with the
         //  4096-workgroup cap of grid_for the targets beyond 32 768 were dropped, which a batch of configs[1] blocks reaches)
         if (np != 1 || !d_mvslot) PIPS_FAIL(PIPS_ERR_STATE, "deterministic mode: several right-hand sides go panel by panel");
         auto mgather = [&](const GatherList& g) {
            if (g.n_targets > 0)
               hipLaunchKernelGGL(k_mgather_slots, dim3(grid_for(g.n_targets * 32, 256, INT32_MAX)), dim3(256), 0, stream, g.n_targets, g.d_tgt, g.d_off, g.d_slots, d_mvslot, xm);
         };
         for (size_t li = 0; li < levels.size(); ++li) {
            const LevelRange& L = levels[li];
            mgather(gv_levels[li]);
            if (L.simple_cnt > 0 && lf_rows > 0)
               hipLaunchKernelGGL(k_mleaf_fwd_gather, dim3(grid_for(lf_rows * 32, 256, INT32_MAX)), dim3(256), 0, stream, d_lf_rows, d_lf_ptr, d_lf_src, d_lf_val, xm, (int)lf_rows);
            else if (L.simple_cnt > 0)
               hipLaunchKernelGGL(k_mhead, dim3((L.simple_cnt + 3) / 4, 1), dim3(256), 0, stream, d_sns, L.simple_begin, L.simple_cnt, d_blks, d_rowidx, d_arena, xm, 0, ps,
                                  d_mvslot);
            const int begin = L.small_cnt > 0 ? L.small_begin : L.large_begin;
            const int cnt = L.small_cnt + L.large_cnt;
            if (cnt > 0)
               hipLaunchKernelGGL(k_mhead, dim3((cnt + 3) / 4, 1), dim3(256), 0, stream, d_sns, begin, cnt, d_blks, d_rowidx, d_arena, xm, 0, ps, d_mvslot);
         }
         mgather(gv_tail);
      } else {
      for (const LevelRange& L : levels) head(L, 0);
      for (const LevelRange& L : levels_top) head(L, 0);
      }
      // the tail sweeps: slicing and launches are mtail_slices / mtail_sweep's (shared with the dense root)
      const TailCtx c = ctx();
      const int sl = mtail_slices(c, np, multi_knob().slices, pin_slices);
      mtail_sweep(c, xm, ps, np, sl, 0);
      if (nsn_total > 0)
         hipLaunchKernelGGL(k_mhead_dscale, dim3(grid_for((long long)nsn_total * MQ, 256), np), dim3(256), 0, stream, d_sns, nsn_total, d_blks,
                            d_arena, xm, ps);
      mtail_sweep(c, xm, ps, np, sl, 1);
      for (int l = (int)levels_top.size() - 1; l >= 0; --l) head(levels_top[l], 1);
      for (int l = (int)levels.size() - 1; l >= 0; --l) head(levels[l], 1);
      hipLaunchKernelGGL(k_mpermute, pg, dim3(256), 0, stream, d_blks, d_perm, d_perm_off, X, x_stride, nr, xm, 1, ps);
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }

   // multi-RHS solve (DoubleLinearSolver::solve(int nrhss, double* rhss, int*), PardisoSolver.C:276-352): all right-hand
   // sides share every launch (grid.y/z = rhs index); refine_steps unconditional refinement steps.  X_dev: nrhs vectors of
   // length n_total at distance x_stride.
   static constexpr int MULTI_CHUNK_MAX = 256;   // right-hand sides per pass (eight panels)
   int ensure_multi_buffers(int want = 32) {
      want = std::min(MULTI_CHUNK_MAX, (std::max(want, 32) + MQ - 1) / MQ * MQ);
      if (mx_cap < want) {
         HIP_TRY(hipSetDevice(device));
         HIP_TRY(hipStreamSynchronize(stream));
         d_mx_xw.reset(); d_mx_rhs.reset(); d_mx_res.reset();   // (all three go before the larger ones come)
         PIPS_TRY(d_mx_xw.alloc((size_t)want * std::max<long long>(xw_total, 1)));
         PIPS_TRY(d_mx_rhs.alloc((size_t)want * std::max<long long>(n_total, 1)));
         PIPS_TRY(d_mx_res.alloc((size_t)want * std::max<long long>(n_total, 1)));
         mx_cap = want;
      }
      if (!d_mmeasure) {   // per right-hand side: the measure of the adaptive refinement (device / pinned host, behind it the list of columns to correct)
         PIPS_TRY(d_mmeasure.alloc(MULTI_CHUNK_MAX));
         PIPS_TRY(d_midx.alloc(MULTI_CHUNK_MAX));
         PIPS_TRY(h_mmeasure.alloc(MULTI_CHUNK_MAX + MULTI_CHUNK_MAX / 2));   // (a double and an int per right-hand side)
      }
      return PIPS_OK;
   }
   int solve_multi(double* X_dev, int nrhs, long long x_stride) {
      if (!factored) PIPS_FAIL(PIPS_ERR_STATE, "solve called before factor");
      HIP_TRY(hipSetDevice(device));
      // deterministic mode: the interleaved sweeps panel by panel with the slot / gather forward substitution (solve_once_multi) where the
      // slots of a panel fit 4 GB (MQ doubles per contribution of the head: a leaf handle, a small batch), else one right-hand side at a time
      const bool det_multi = deterministic && head_slots && use_multi(nrhs) && vslots_total > 0 && (double)vslots_total * MQ * sizeof(double) <= 4e9;
      last_multi_path = det_multi ? 2 : (deterministic || !use_multi(nrhs)) ? 0 : 1;
      if (deterministic && !det_multi) {   // one right-hand side at a time through the atomics-free sweeps
         int steps = 0;   // (as below: the steps of the last right-hand side that took any)
         for (int r = 0; r < nrhs; ++r) {
            if (int rc = solve(X_dev + (long long)r * x_stride)) return rc;
            if (last_refine_steps > 0) steps = last_refine_steps;
         }
         last_refine_steps = steps;
         return PIPS_OK;
      }
      if (det_multi && !d_mvslot) PIPS_TRY(d_mvslot.alloc((size_t)vslots_total * MQ));
      last_refine_steps = 0;   // (over the chunks: the steps of the last one that took any - not their sum)
      const bool multi = use_multi(nrhs);
      const int chunk_max = det_multi ? MQ : multi ? MULTI_CHUNK_MAX : 32;   // (the per-right-hand-side sweeps keep their 32 work vectors)
      int rc0 = ensure_multi_buffers(std::min(nrhs, chunk_max));
      if (rc0) return rc0;
      for (int r0 = 0; r0 < nrhs; r0 += chunk_max) {
         const int nr = std::min(chunk_max, nrhs - r0);
         double* X = X_dev + (long long)r0 * x_stride;
         if (refine_steps > 0)
            HIP_TRY(hipMemcpy2DAsync(d_mx_rhs, (size_t)n_total * sizeof(double), X, (size_t)x_stride * sizeof(double),
                                     (size_t)n_total * sizeof(double), nr, hipMemcpyDeviceToDevice, stream));
         int rc = multi ? solve_once_multi(X, nr, x_stride, d_mx_xw) : solve_once(X, nr, x_stride, d_mx_xw);
         if (rc) return rc;
         int chunk_steps = 0;
         for (int it = 0; it < refine_steps; ++it) {
            HIP_TRY(hipMemcpyAsync(d_mx_res, d_mx_rhs, (size_t)nr * n_total * sizeof(double), hipMemcpyDeviceToDevice, stream));
            // r = rhs - K x for every right-hand side: x at stride x_stride, r contiguous -> a contiguous view of x where the caller's is not
            // (d_mx_xw is free between solves; it is at least nr * n_total long because xw_total >= n_total)
            const double* Xc = X;
            if (x_stride != n_total) {
               HIP_TRY(hipMemcpy2DAsync(d_mx_xw, (size_t)n_total * sizeof(double), X, (size_t)x_stride * sizeof(double),
                                        (size_t)n_total * sizeof(double), nr, hipMemcpyDeviceToDevice, stream));
               Xc = d_mx_xw;
            }
            if ((rc = launch_residual(Xc, n_total, nullptr, d_mx_res, nr))) return rc;
            int n_fix = nr;   // right-hand sides that take the correction solve: all of them, or (adaptive) those whose measure says so
            if (refine_tol > 0.0 && d_mmeasure) {
               // adaptive like the single right-hand side (solve()), per right-hand side like PARDISO: every column's worst block is measured,
               // one small copy back to the host, and the correction solve takes only the columns that were not accurate enough - their
               // residuals moved side by side to the front (ascending: a column never lands on one that is still to move)
               HIP_TRY(hipMemsetAsync(d_mmeasure, 0, (size_t)nr * sizeof(double), stream));
               hipLaunchKernelGGL(k_mrefine_measure, dim3(nblk, nr), dim3(256), 0, stream, d_blks, d_mx_res, n_total, d_mx_rhs, n_total, Xc, n_total,
                                  refine_mode == 1 ? 1.0 / (repl_rel > 0 ? repl_rel : 1.0) : 0.0, d_mmeasure);
               HIP_TRY(hipMemcpyAsync(h_mmeasure, d_mmeasure, (size_t)nr * sizeof(double), hipMemcpyDeviceToHost, stream));
               HIP_TRY(hipStreamSynchronize(stream));
               int* fix = (int*)(h_mmeasure + MULTI_CHUNK_MAX);
               n_fix = 0;
               double worst = 0.0;
               for (int q = 0; q < nr; ++q) {
                  if (!(h_mmeasure[q] <= worst)) worst = h_mmeasure[q];
                  if (!(h_mmeasure[q] <= refine_tol)) fix[n_fix++] = q;
               }
               last_refine_measure = worst;
               if (n_fix == 0) break;
               if (n_fix < nr) {
                  for (int i = 0; i < n_fix; ++i)
                     if (fix[i] != i)
                        HIP_TRY(hipMemcpyAsync(d_mx_res + (size_t)i * n_total, d_mx_res + (size_t)fix[i] * n_total, (size_t)n_total * sizeof(double), hipMemcpyDeviceToDevice, stream));
                  HIP_TRY(hipMemcpyAsync(d_midx, fix, (size_t)n_fix * sizeof(int), hipMemcpyHostToDevice, stream));
               }
            }
            // (not solve_chunk: the choice follows the whole batch (multi), not n_fix, and a deterministic panel keeps the slicing of the first solve)
            rc = (multi && (n_fix > 1 || det_multi)) ? solve_once_multi(d_mx_res, n_fix, n_total, d_mx_xw) : solve_once(d_mx_res, n_fix, n_total, d_mx_xw);
            if (rc) return rc;
            if (n_fix < nr) hipLaunchKernelGGL(k_maxpy_idx, dim3(grid_for(n_total, 256, 1024), n_fix), dim3(256), 0, stream, X, x_stride, d_mx_res, n_total, 1.0, n_total, d_midx);
            else hipLaunchKernelGGL(k_maxpy, dim3(grid_for(n_total, 256, 1024), nr), dim3(256), 0, stream, X, x_stride, d_mx_res, n_total, 1.0, n_total);
            ++chunk_steps;
         }
         if (chunk_steps > 0) last_refine_steps = chunk_steps;
      }
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }

   // res = rhs - K x for nr vectors at distance stride (x and res alike) against the CSR values on the device.  rhs == nullptr: res holds the
   // right-hand sides on entry.  Else (one vector) the copy of rhs is folded into the product - unless there are long rows, whose kernel
   // subtracts from what res holds
   int launch_residual(const double* x, long long stride, const double* rhs, double* res, int nr) {
      if (rhs && n_flong > 0) {
         HIP_TRY(hipMemcpyAsync(res, rhs, (size_t)n_total * sizeof(double), hipMemcpyDeviceToDevice, stream));
         rhs = nullptr;
      }
      hipLaunchKernelGGL(k_full_spmv_sub, dim3(grid_for(n_total * 8, 256, 65536), nr), dim3(256), 0, stream, d_frowptr, d_fcol, d_fsrc, d_kval,
                         x, res, n_total, d_rowbase, stride, rhs);
      if (n_flong > 0)
         hipLaunchKernelGGL(k_full_spmv_sub_long, dim3(n_flong, nr), dim3(256), 0, stream, d_flong, d_frowptr, d_fcol, d_fsrc, d_kval, x, res, d_rowbase, stride);
      return PIPS_OK;
   }
   // The measure of the adaptive refinement from the per-block norms on the device (d_norms: ||r_b||inf, ||rhs_b||inf, ||x_b||inf): the worst
   // block of ||r_b|| over the denominator of refine_mode - max|K_b| ||x_b|| + ||rhs_b|| (normwise backward error) or ||rhs_b||.  Ends the
   // caller's timer phase behind the copy of the norms; one host wait
   int worst_from_norms(double* worst_out) {
      HIP_TRY(hipMemcpyAsync(h_norms, d_norms, (size_t)3 * nblk * sizeof(double), hipMemcpyDeviceToHost, stream));
      timer.end(stream);
      std::vector<BlkDesc> tmp;
      const bool need_amax = refine_mode == 1 && h_amax.empty();   // (the blocks' largest entries: once per factorisation, with the same wait)
      if (need_amax) {
         tmp.resize(nblk);
         HIP_TRY(hipMemcpyAsync(tmp.data(), d_blks, (size_t)nblk * sizeof(BlkDesc), hipMemcpyDeviceToHost, stream));
      }
      HIP_TRY(hipStreamSynchronize(stream));
      if (need_amax) {
         h_amax.resize(nblk);
         for (int b = 0; b < nblk; ++b) h_amax[b] = tmp[b].repl_abs / (repl_rel > 0 ? repl_rel : 1.0);   // = max|K_b| (k_block_absmax)
      }
      double worst = 0.0;
      for (int b = 0; b < nblk; ++b) {
         const double den = refine_mode == 1 ? h_amax[b] * h_norms[2 * nblk + b] + h_norms[nblk + b] : h_norms[nblk + b];
         // (a non-finite norm - Inf, or Inf / Inf = NaN - must win the comparison: never "converged" on a poisoned iterate)
         if (den > 0.0) { const double q = h_norms[b] / den; if (!(q <= worst)) worst = q; }
      }
      *worst_out = worst;
      last_refine_measure = worst;
      return PIPS_OK;
   }

   // x := K^-1 x with up to refine_steps steps of iterative refinement against the CSR values on the device.
   // refine_tol > 0 makes it adaptive like PARDISO's iparm[7] (PardisoProjectSolver.C:72): after every solve the residual
   // is formed and the loop stops once max_b ||r_b||inf / ||rhs_b||inf <= refine_tol (one small D2H copy + stream sync).
   int solve(double* x_dev) {
      if (!factored) PIPS_FAIL(PIPS_ERR_STATE, "solve called before factor");
      HIP_TRY(hipSetDevice(device));
      last_refine_steps = 0;
      if (refine_steps <= 0) return solve_once(x_dev);
      const size_t bytes = (size_t)n_total * sizeof(double);
      HIP_TRY(hipMemcpyAsync(d_rhs, x_dev, bytes, hipMemcpyDeviceToDevice, stream));
      if (refine_tol > 0.0) {
         HIP_TRY(hipMemsetAsync(d_norms + nblk, 0, (size_t)nblk * sizeof(double), stream));
         hipLaunchKernelGGL(k_vec_block_absmax, dim3(absmax_chunks(), nblk), dim3(256), 0, stream, d_rhs, d_blks, d_norms + nblk);
      }
      int rc = solve_once(x_dev);
      if (rc) return rc;
      for (int it = 0; it < refine_steps; ++it) {
         timer.begin(stream, 11);
         if ((rc = launch_residual(x_dev, 0, d_rhs, d_res, 1))) return rc;
         if (refine_tol > 0.0) {
            HIP_TRY(hipMemsetAsync(d_norms, 0, (size_t)nblk * sizeof(double), stream));
            hipLaunchKernelGGL(k_vec_block_absmax, dim3(absmax_chunks(), nblk), dim3(256), 0, stream, d_res, d_blks, d_norms);
            if (refine_mode == 1) {
               HIP_TRY(hipMemsetAsync(d_norms + 2 * nblk, 0, (size_t)nblk * sizeof(double), stream));
               hipLaunchKernelGGL(k_vec_block_absmax, dim3(absmax_chunks(), nblk), dim3(256), 0, stream, x_dev, d_blks, d_norms + 2 * nblk);
            }
            double worst;
            if ((rc = worst_from_norms(&worst))) return rc;
            if (worst <= refine_tol) break;
         } else
            timer.end(stream);
         rc = solve_once(d_res);
         if (rc) return rc;
         hipLaunchKernelGGL(k_axpy, dim3(grid_for(n_total, 256)), dim3(256), 0, stream, x_dev, d_res, 1.0, n_total);
         ++last_refine_steps;
      }
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }

   // The measure of the adaptive refinement for a solution somebody else produced: worst block of ||rhs - K x||inf over the denominator of
   // refine_mode (normwise backward error, or ||rhs||inf) - one product with the CSR values, the norms, one small copy to the host.
   int residual_measure(const double* rhs_dev, const double* x_dev, double* worst_out) {
      if (refine_steps <= 0 || !d_res || !d_norms) PIPS_FAIL(PIPS_ERR_STATE, "residual_measure: refinement buffers missing");
      timer.begin(stream, 11);
      HIP_TRY(hipMemsetAsync(d_norms, 0, (size_t)3 * nblk * sizeof(double), stream));
      hipLaunchKernelGGL(k_vec_block_absmax, dim3(absmax_chunks(), nblk), dim3(256), 0, stream, rhs_dev, d_blks, d_norms + nblk);
      if (int rc = launch_residual(x_dev, 0, rhs_dev, d_res, 1)) return rc;
      hipLaunchKernelGGL(k_vec_block_absmax, dim3(absmax_chunks(), nblk), dim3(256), 0, stream, d_res, d_blks, d_norms);
      if (refine_mode == 1) hipLaunchKernelGGL(k_vec_block_absmax, dim3(absmax_chunks(), nblk), dim3(256), 0, stream, x_dev, d_blks, d_norms + 2 * nblk);
      return worst_from_norms(worst_out);
   }

   // the measure of a solveCompressed by sweeps in one launch (k_measure_leaf_rows): x = the result, b = the leaf right-hand side as the
   // caller gave it, x0 = the root solution.  Same quantity and same host formula as residual_measure on (b - Br x0, x); available where
   // every row of K is short and the border is held by leaf row
   bool can_measure_fused() const { return refine_steps > 0 && d_norms && n_flong == 0 && (bt_rows_total == 0 || d_br_rowptr); }   // (deterministic mode too: a row is summed by eight lanes in a fixed tree, the maxima do not depend on an order)
   int residual_measure_fused(const double* b_dev, const double* x0_dev, const double* x_dev, double* worst_out) {
      timer.begin(stream, 11);
      HIP_TRY(hipMemsetAsync(d_norms, 0, (size_t)3 * nblk * sizeof(double), stream));
      hipLaunchKernelGGL(k_measure_leaf_rows, dim3(std::max(absmax_chunks(), (int)std::min<long long>(256, n_total / std::max(nblk, 1) / 2048 + 1)), nblk), dim3(256), 0, stream,
                         d_blks, d_frowptr, d_fcol, d_fsrc, d_kval, x_dev, b_dev, bt_rows_total > 0 ? d_br_rowptr : (const int*)nullptr, d_br_sc, d_br_src, d_bval, x0_dev,
                         d_norms, nblk);
      return worst_from_norms(worst_out);
   }

   // The inertia counters travel to pinned host memory at the end of every factorisation (factor()); a query only waits for that
   // copy - not for whatever was queued behind the factorisation (the leaf solves of an Lsolve, say).
   int fetch_inertia() {
      if (inertia_in_flight && h_inertia_pin) {   // one wait per factorisation: a query per block (256 of them per IPM iteration) reads the host copy
         HIP_TRY(hipEventSynchronize(ev_inertia));
         std::copy(h_inertia_pin.get(), h_inertia_pin + h_inertia.size(), h_inertia.begin());
         inertia_in_flight = false;
         inertia_on_host = true;
         if (tail_single && h_inertia_pin[3 * nblk]) {
            h_inertia_pin[3 * nblk] = 0;
            int fi[6] = {0, 0, 0, 0, 0, 0};   // the first wait that gave up: kind, tile, K range, block + 1
            (void)hipMemcpy(fi, tsingle.d_ctl + 10, sizeof(fi), hipMemcpyDeviceToHost);
            HIP_TRY(hipMemsetAsync(tsingle.d_ctl + 9, 0, 7 * sizeof(int), stream));
            PIPS_FAIL(PIPS_ERR_HIP, "the single-launch factorisation of the dense tails (PIPS_HIP_TAIL_SINGLE) gave up waiting for a tile after %lld polls - first: task "
                                    "kind %d on tile (%d, %d) of block %d; its factors are unusable.  Another process holding the device for seconds can cause that",
                      tsingle.args.poll_limit, fi[1], fi[2], fi[3], fi[5] - 1);
         }
         return PIPS_OK;
      }
      if (inertia_on_host) return PIPS_OK;
      HIP_TRY(hipMemcpyAsync(h_inertia.data(), d_inertia, h_inertia.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      return PIPS_OK;
   }

   // ---- border-backward sweep ----------------------------------------------------------------------
   // u_i = K_i^-1 Br_i x0 for every block from the augmented factor alone:  Br_i = L D L21^T, so  u = L^-T (L21^T x0)  - the
   // backward sweep of the augmented factor [L 0; L21 I] with a zero right-hand side and the border unknowns fixed to -x0.  No
   // border product, no forward sweep, no diagonal scaling.  Pays where the border rows of the factor are no larger than what a
   // forward sweep reads (decided at analyze time, border_backward_ok); needs Schur mode 1 and the single-launch tail sweeps.
   // There is no refinement in it: the caller uses it only while the factorisation has no perturbed pivot (perturbed_leaf_pivots).
   long long aug_passes = 0;     // passes (forward + backward) of those sweeps so far
   int perturbed_cache = -1;   // perturbed pivots of the current factorisation over all blocks; -1 = not fetched yet
   int perturbed_leaf_pivots(int* out) {
      if (perturbed_cache < 0) {
         int rc = fetch_inertia();
         if (rc) return rc;
         int z = 0;
         for (int b = 0; b < nblk; ++b) z += h_inertia[3 * b + 2];
         perturbed_cache = z;
      }
      *out = perturbed_cache;
      return PIPS_OK;
   }
   // Forward sweep of the augmented factor [L 0; L_b I] on [b; 0]: the work vector keeps y = L^-1 P b (tail rows D^-1-scaled, as the tail
   // sweep leaves them) for backward_augmented, and red += -L_b y = -Br^T K^-1 b, block by block (what Lsolve adds to b0,
   // sLinsysRootAug.C:323-344, without the backward sweep, the residual check and the sparse border product of a full solve).
   int forward_augmented(const double* b_dev, double* red) {
      if (!factored) PIPS_FAIL(PIPS_ERR_STATE, "solve called before factor");
      HIP_TRY(hipSetDevice(device));
      {
         PhaseTimer::Scope phase(&timer, stream, 7);
         hipLaunchKernelGGL(k_border_fill, dim3(8, nblk), dim3(256), 0, stream, d_blks, d_bmap, (const double*)nullptr, d_xw, 0.0);
         hipLaunchKernelGGL(k_permute_in, dim3(64, nblk, 1), dim3(256), 0, stream, d_blks, d_perm, d_perm_off, b_dev, 0LL, d_xw, 0LL);
      }
      { PhaseTimer::Scope phase(&timer, stream, 8); head_forward(d_xw, 1, 0, sx_atomic(), 1); }
      {
         PhaseTimer::Scope phase(&timer, stream, 9);   // (one record of this phase per pass: the backward half books its tail sweep with the head's)
         PIPS_TRY(tail_fwd(ctx(), d_xw));
         if (nb_pad_max > 0)
            hipLaunchKernelGGL(k_tail_border_fwd, dim3(nb_pad_max / TILE, nblk), dim3(256), 0, stream, d_blks, d_arena, d_dtail, d_xw);
         hipLaunchKernelGGL(k_border_collect, dim3(8, nblk), dim3(256), 0, stream, d_blks, d_bmap, d_xw, red);
      }
      ++aug_passes;
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   // The same sweep in deterministic mode: the head by the slot / gather scheme of solve_once (no atomics), the border slots of every block by
   // k_border_gather_det from the finished head part (target by target, fixed order), the dense tail's border rows by k_tail_border_fwd (one
   // writer per row).  The border slots stay in the work vector: the caller gathers them group-wise (g_bslot_grp) like Br^T z.
   int forward_augmented_det(const double* b_dev) {
      if (!factored) PIPS_FAIL(PIPS_ERR_STATE, "solve called before factor");
      if (!det.aug.ready || !head_slots) PIPS_FAIL(PIPS_ERR_STATE, "forward_augmented_det: not prepared");
      HIP_TRY(hipSetDevice(device));
      {
         PhaseTimer::Scope phase(&timer, stream, 7);
         hipLaunchKernelGGL(k_border_fill, dim3(8, nblk), dim3(256), 0, stream, d_blks, d_bmap, (const double*)nullptr, d_xw, 0.0);
         hipLaunchKernelGGL(k_permute_in, dim3(64, nblk, 1), dim3(256), 0, stream, d_blks, d_perm, d_perm_off, b_dev, 0LL, d_xw, 0LL);
      }
      {
         PhaseTimer::Scope phase(&timer, stream, 8);
         head_forward(d_xw, 1, 0, ScatterCtx{2, nullptr, d_vslot_val, d_xw, nullptr}, 0);   // (the border slots: by the two kernels below, from the finished head part)
         hipLaunchKernelGGL(k_border_rowdot_det, dim3(grid_for(det.aug.n_ent, 256, 1 << 20)), dim3(256), 0, stream, det.aug.n_ent, d_bg_ent, d_arena, d_xw, d_bg_val);
         hipLaunchKernelGGL(k_border_gather_det, dim3((unsigned)((det.aug.n_targets + 3) / 4)), dim3(256), 0, stream, det.aug.n_targets, d_bg_ptr, d_bg_idx, d_bg_slot, d_bg_val, d_xw);
      }
      {
         PhaseTimer::Scope phase(&timer, stream, 9);
         PIPS_TRY(tail_fwd(ctx(), d_xw));
         if (nb_pad_max > 0)
            hipLaunchKernelGGL(k_tail_border_fwd, dim3(nb_pad_max / TILE, nblk), dim3(256), 0, stream, d_blks, d_arena, d_dtail, d_xw);
      }
      ++aug_passes;
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   // ... and the backward sweep from where forward_augmented stopped: border slots = x0, x = L^-T (D^-1 y - L_b^T x0) = K^-1 (b - Br x0)
   // in original order at out_dev (Ltsolve, sLinsysRootAug.C:346-365 / LniTransMult, with nothing left to combine)
   int backward_augmented(const double* x0_dev, double* out_dev) {
      if (!factored) PIPS_FAIL(PIPS_ERR_STATE, "solve called before factor");
      HIP_TRY(hipSetDevice(device));
      {
         PhaseTimer::Scope phase(&timer, stream, 10);
         hipLaunchKernelGGL(k_border_fill, dim3(8, nblk), dim3(256), 0, stream, d_blks, d_bmap, x0_dev, d_xw, 1.0);
         PIPS_TRY(tail_bwd(ctx(), d_xw, 1, 0, 1));
         head_backward(d_xw, 1, 0, 1, 1);
      }
      { PhaseTimer::Scope phase(&timer, stream, 7); hipLaunchKernelGGL(k_permute_out, dim3(64, nblk, 1), dim3(256), 0, stream, d_blks, d_perm, d_perm_off, out_dev, 0LL, d_xw, 0LL); }
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   int solve_border_backward(const double* x0_dev, double* out_dev) {
      if (!factored) PIPS_FAIL(PIPS_ERR_STATE, "solve called before factor");
      HIP_TRY(hipSetDevice(device));
      HIP_TRY(hipMemsetAsync(d_xw, 0, (size_t)xw_total * sizeof(double), stream));
      hipLaunchKernelGGL(k_border_fill, dim3(8, nblk), dim3(256), 0, stream, d_blks, d_bmap, x0_dev, d_xw);
      TailCtx c = ctx();
      int rc = tail_bwd(c, d_xw, 1, 0, 1);
      if (rc) return rc;
      // no D^-1 (the right-hand side is zero); the leaves take their border rows in the sum of their other rows
      head_backward(d_xw, 1, 0, 1, 0, true);
      hipLaunchKernelGGL(k_permute_out, dim3(64, nblk, 1), dim3(256), 0, stream, d_blks, d_perm, d_perm_off, out_dev, 0LL, d_xw, 0LL);
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
};

// resolves -1 to the current device and checks the range (the entry points that create something on a device)
static int resolve_device(int device, int* out) {
   int cnt = 0;
   if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0)
      PIPS_FAIL(PIPS_ERR_NO_DEVICE, "no HIP device visible: the MI355X backend has no CPU fallback");
   if (device < 0) { HIP_TRY(hipGetDevice(&device)); }
   if (device >= cnt) PIPS_FAIL(PIPS_ERR_ARG, "device %d out of range (%d visible)", device, cnt);
   *out = device;
   return PIPS_OK;
}

#include "denseroot.hip.h"

// add_regularization_local_kkt (DistributedLeafLinearSystem.C:108-143): K diag += primal on the leading n_primal rows,
// -= dual on the rest
__global__ void k_add_regularization(const BlkDesc* __restrict__ blks, const int* __restrict__ n_primal,
                                     const long long* __restrict__ kdiag, double* __restrict__ kval, double primal, double dual) {
   const BlkDesc bd = blks[blockIdx.y];
   const int np = n_primal[blockIdx.y];
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < bd.n; i += gridDim.x * blockDim.x)
      kval[kdiag[bd.x_off + i]] += (np < 0 || i < np) ? primal : -dual;
}

#include "borderpanel.hip.h"

// the one launch site of the two border-panel products outside deterministic mode (KktSystem::solve_panel, pips_hip_batch_border_*_panel_dev)
static void launch_border_tmult_panel(Engine* e, const double* Z, long long ldz, int nr, double* T, long long ldt, double alpha) {
   if (e->bt_rows_total > 0)
      hipLaunchKernelGGL(k_border_tmult_panel<false>, dim3(grid_for(e->bt_rows_total * BT_LANES, 256, 65536)), dim3(256), 0, e->stream, e->d_bt_rowptr, e->d_bt_colidx,
                         e->d_bval, e->d_bt_rowsc, e->d_bt_xoff, Z, ldz, nr, T, ldt, e->bt_rows_total, alpha);
}
// W = alpha Br X0: every row of W is written.  layout_border_csr builds the border by leaf row whenever the border has entries (fewer than
// 2^31: the int row pointers of the concatenated Bt CSR hold no more), so the lists are never missing where there is something to multiply -
// building them on first use, which the single path's k_border_mult stands in for, has no case; a batch that had none would be told so
static int launch_border_mult_panel(Engine* e, const double* X0, long long ldx, int nr, double* W, long long ldw, double alpha) {
   if (e->bt_rows_total > 0 && e->d_br_rowptr)
      hipLaunchKernelGGL(k_border_mult_panel, dim3(grid_for(e->n_total, 256, 1 << 20)), dim3(256), 0, e->stream, e->d_br_rowptr, e->d_br_sc, e->d_br_src, e->d_bval,
                         X0, ldx, nr, W, ldw, e->n_total, alpha);
   else if (e->bt_rows_total == 0 || e->nnzB_total == 0)
      HIP_TRY(hipMemset2DAsync(W, (size_t)ldw * sizeof(double), 0, (size_t)e->n_total * sizeof(double), (size_t)nr, e->stream));
   else
      PIPS_FAIL(PIPS_ERR_STATE, "the border by leaf row was not built (2^31 or more border entries): no panel product of Br");
   return PIPS_OK;
}
#include "kkt.hip.h"

}  // namespace pips

// =================================================================================================================
// C ABI
// =================================================================================================================
using namespace pips;

extern "C" {

const char* pips_hip_last_error(void) { return pips::last_error(); }
long long pips_hip_host_wait_count(void) { return pips::g_host_waits.load(std::memory_order_relaxed); }
long long pips_hip_device_allocs_live(void) { return pips::g_mem_allocs_live.load(std::memory_order_relaxed); }
long long pips_hip_device_bytes_live(void) { return pips::g_mem_bytes_live.load(std::memory_order_relaxed); }
int pips_hip_host_wait_sites(char* buf, int cap) {
   int used = 0;
   if (buf && cap > 0) buf[0] = 0;
   for (const pips::WaitSite& w : pips::g_wait_sites) {
      const char* f = w.file.load();
      if (!f || w.n.load() == 0) continue;
      const char* base = strrchr(f, '/');
      const int k = snprintf(buf ? buf + used : nullptr, buf && cap > used ? cap - used : 0, "%s:%d %lld\n", base ? base + 1 : f, w.line.load(), w.n.load());
      if (k < 0 || !buf || used + k >= cap) break;
      used += k;
   }
   return used;
}

int pips_hip_device_count(void) {
   int n = 0;
   if (hipGetDeviceCount(&n) != hipSuccess) return 0;
   return n;
}

// ---- batch -------------------------------------------------------------------------------------------------------
int pips_hip_batch_create(void** handle, int n_blocks, int S, int device, void* stream) {
   if (!handle || n_blocks <= 0 || S < 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_batch_create: bad arguments");
   auto e = std::make_unique<Engine>();
   e->nblk = n_blocks;
   e->S = S;
   e->device = device;   // resolved at analyze time so that set_block / symbolic work without a GPU
   e->stream = (hipStream_t)stream;
   e->in.assign(n_blocks, BlockInput());
   e->deterministic = env_deterministic();   // default of pips_hip_batch_set_deterministic
   *handle = e.release();
   return PIPS_OK;
}

int pips_hip_batch_set_block(void* handle, int b, int n, int n_primal, const int* K_rowptr, const int* K_colidx,
                             const int* Bt_rowptr, const int* Bt_colidx, const double* Bt_val) {
   Engine* e = (Engine*)handle;
   if (!e || b < 0 || b >= e->nblk || n <= 0 || !K_rowptr || !K_colidx) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_batch_set_block: bad arguments");
   BlockInput& in = e->in[b];
   in.n = n;
   in.n_primal = n_primal;
   in.krow.assign(K_rowptr, K_rowptr + n + 1);
   in.kcol.assign(K_colidx, K_colidx + K_rowptr[n]);
   in.btrow.clear(); in.btcol.clear(); in.btval.clear();
   if (Bt_rowptr && e->S > 0) {
      in.btrow.assign(Bt_rowptr, Bt_rowptr + e->S + 1);
      const int nnz = Bt_rowptr[e->S];
      in.btcol.assign(Bt_colidx, Bt_colidx + nnz);
      if (Bt_val) in.btval.assign(Bt_val, Bt_val + nnz); else in.btval.assign(nnz, 0.0);
   }
   e->analyzed = false;
   return PIPS_OK;
}

int pips_hip_batch_set_options(void* handle, int force_n_head, int refine_steps, double thr_rel, double repl_rel) {
   Engine* e = (Engine*)handle;
   if (!e) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   e->opt.force_n_head = force_n_head;
   if (refine_steps >= 0) e->refine_steps = refine_steps;
   if (thr_rel >= 0) e->thr_rel = thr_rel;
   if (repl_rel > 0) e->repl_rel = repl_rel;
   return PIPS_OK;
}

int pips_hip_batch_set_schur_mode(void* handle, int mode) {
   Engine* e = (Engine*)handle;
   if (!e || mode < 0 || mode > 2) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_batch_set_schur_mode: mode must be 0 (auto), 1 or 2");
   if (e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_set_schur_mode: call before analyze");
   e->schur_mode = mode;
   return PIPS_OK;
}

int pips_hip_batch_set_deterministic(void* handle, int on) {
   Engine* e = (Engine*)handle;
   if (!e) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   if (e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_set_deterministic: call before pips_hip_batch_analyze");
   e->deterministic = on != 0;
   return PIPS_OK;
}

int pips_hip_batch_get_schur_mode(void* handle, int* mode) {
   Engine* e = (Engine*)handle;
   if (!e || !mode || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_get_schur_mode: analyze first");
   *mode = e->schur_mode_eff;
   return PIPS_OK;
}

int pips_hip_batch_add_regularization(void* handle, double primal, double dual) {
   Engine* e = (Engine*)handle;
   if (!e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_add_regularization: analyze first");
   HIP_TRY(hipSetDevice(e->device));
   hipLaunchKernelGGL(k_add_regularization, dim3(32, e->nblk), dim3(256), 0, e->stream, e->d_blks, e->d_nprimal, e->d_kdiag, e->d_kval,
                      primal, dual);
   HIP_TRY(hipGetLastError());
   return PIPS_OK;
}

int pips_hip_batch_set_refinement(void* handle, int max_steps, double tol) {
   Engine* e = (Engine*)handle;
   if (!e || max_steps < 0 || tol < 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_batch_set_refinement: bad arguments");
   e->refine_steps = max_steps;
   e->refine_tol = tol;
   e->refine_mode = 0;
   return PIPS_OK;
}

int pips_hip_batch_set_refinement_backward_error(void* handle, int max_steps, double tol) {
   Engine* e = (Engine*)handle;
   if (!e || max_steps < 0 || tol < 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_batch_set_refinement_backward_error: bad arguments");
   e->refine_steps = max_steps;
   e->refine_tol = tol;
   e->refine_mode = 1;
   return PIPS_OK;
}

double pips_hip_batch_last_refinement_measure(void* handle) {
   Engine* e = (Engine*)handle;
   return e ? e->last_refine_measure : -1.0;
}

int pips_hip_batch_last_refinement_steps(void* handle) {
   Engine* e = (Engine*)handle;
   return e ? e->last_refine_steps : -1;
}

int pips_hip_batch_analyze(void* handle, int n_threads) {
   Engine* e = (Engine*)handle;
   if (!e) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   int dev;
   int rc = resolve_device(e->device, &dev);
   if (rc) return rc;
   e->device = dev;
   return e->analyze(n_threads);
}

int pips_hip_batch_set_values(void* handle, int b, const double* K_val_host) {
   Engine* e = (Engine*)handle;
   if (!e || !e->analyzed || b < 0 || b >= e->nblk) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_set_values: analyze first");
   HIP_TRY(hipSetDevice(e->device));
   HIP_TRY(hipMemcpyAsync(e->d_kval + e->kptr[b], K_val_host, (size_t)(e->kptr[b + 1] - e->kptr[b]) * sizeof(double),
                          hipMemcpyHostToDevice, e->stream));
   HIP_TRY(hipStreamSynchronize(e->stream));
   return PIPS_OK;
}

int pips_hip_batch_set_diagonals_dev(void* handle, const double* diag_dev) {
   Engine* e = (Engine*)handle;
   if (!e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_set_diagonals: analyze first");
   HIP_TRY(hipSetDevice(e->device));
   hipLaunchKernelGGL(k_put_diag, dim3(grid_for(e->n_total, 256)), dim3(256), 0, e->stream, e->d_kdiag, diag_dev, e->d_kval,
                      e->n_total);
   HIP_TRY(hipGetLastError());
   return PIPS_OK;
}

int pips_hip_batch_set_diagonals(void* handle, const double* diag_host) {
   Engine* e = (Engine*)handle;
   if (!e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_set_diagonals: analyze first");
   HIP_TRY(hipSetDevice(e->device));
   HIP_TRY(hipMemcpyAsync(e->d_stage, diag_host, (size_t)e->n_total * sizeof(double), hipMemcpyHostToDevice, e->stream));
   int rc = pips_hip_batch_set_diagonals_dev(handle, e->d_stage);
   if (rc) return rc;
   HIP_TRY(hipStreamSynchronize(e->stream));
   return PIPS_OK;
}

int pips_hip_batch_factor(void* handle, double* SC_dev, int ldSC) {
   Engine* e = (Engine*)handle;
   if (!e) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   if (SC_dev && ldSC < e->S) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_batch_factor: ldSC %d < S %d", ldSC, e->S);
   return e->factor(SC_dev, ldSC);
}

int pips_hip_batch_solve_dev(void* handle, double* x_dev) {
   Engine* e = (Engine*)handle;
   if (!e) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   return e->solve(x_dev);
}

int pips_hip_batch_solve(void* handle, double* x_host) {
   Engine* e = (Engine*)handle;
   if (!e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_solve: analyze first");
   HIP_TRY(hipSetDevice(e->device));
   const size_t bytes = (size_t)e->n_total * sizeof(double);
   HIP_TRY(hipMemcpyAsync(e->d_stage, x_host, bytes, hipMemcpyHostToDevice, e->stream));
   int rc = e->solve(e->d_stage);
   if (rc) return rc;
   HIP_TRY(hipMemcpyAsync(x_host, e->d_stage, bytes, hipMemcpyDeviceToHost, e->stream));
   HIP_TRY(hipStreamSynchronize(e->stream));
   return e->sweep.take_error("pips_hip_batch_solve");
}

int pips_hip_batch_border_tmult_dev(void* handle, const double* z_dev, double* b0_dev, double alpha) {
   Engine* e = (Engine*)handle;
   if (!e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "border_tmult: analyze first");
   HIP_TRY(hipSetDevice(e->device));
   if (e->bt_rows_total > 0 && e->deterministic) {
      hipLaunchKernelGGL(k_border_rowdot, dim3(grid_for(e->bt_rows_total, 256)), dim3(256), 0, e->stream, e->d_bt_rowptr, e->d_bt_colidx, e->d_bval,
                         e->d_bt_xoff, z_dev, e->d_bt_tmp, e->bt_rows_total, alpha);
      e->gather(e->g_btm, e->d_bt_tmp, b0_dev);
   } else if (e->bt_rows_total > 0)
      hipLaunchKernelGGL(k_border_tmult, dim3(grid_for(e->bt_rows_total * BT_LANES, 256, 65536)), dim3(256), 0, e->stream, e->d_bt_rowptr,
                         e->d_bt_colidx, e->d_bval, e->d_bt_rowsc, e->d_bt_xoff, z_dev, b0_dev, e->bt_rows_total, alpha);
   HIP_TRY(hipGetLastError());
   return PIPS_OK;
}

int pips_hip_batch_border_mult_dev(void* handle, const double* x0_dev, double* t_dev, double alpha) {
   Engine* e = (Engine*)handle;
   if (!e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "border_mult: analyze first");
   HIP_TRY(hipSetDevice(e->device));
   if (e->bt_rows_total > 0 && e->deterministic) {
      hipLaunchKernelGGL(k_border_entry_products, dim3(grid_for(e->bt_rows_total, 256)), dim3(256), 0, e->stream, e->d_bt_rowptr, e->d_bval,
                         e->d_bt_rowsc, x0_dev, e->d_bt_tmp, e->bt_rows_total, alpha);
      e->gather(e->g_bm, e->d_bt_tmp, t_dev);
   } else if (e->bt_rows_total > 0 && e->d_br_rowptr)
      hipLaunchKernelGGL(k_border_mult_rows, dim3(grid_for(e->n_total, 256, 1 << 20)), dim3(256), 0, e->stream, e->d_br_rowptr, e->d_br_sc, e->d_br_src,
                         e->d_bval, x0_dev, t_dev, e->n_total, alpha);
   else if (e->bt_rows_total > 0)
      hipLaunchKernelGGL(k_border_mult, dim3(grid_for(e->bt_rows_total * BT_LANES, 256, 65536)), dim3(256), 0, e->stream, e->d_bt_rowptr,
                         e->d_bt_colidx, e->d_bval, e->d_bt_rowsc, e->d_bt_xoff, x0_dev, t_dev, e->bt_rows_total, alpha);
   HIP_TRY(hipGetLastError());
   return PIPS_OK;
}

// the two border products on nrhs vectors (borderpanel.hip.h): the launches KktSystem::solve_panel makes outside deterministic mode
int pips_hip_batch_border_tmult_panel_dev(void* handle, int nrhs, const double* Z_dev, long long ldz, double* T_dev, long long ldt, double alpha) {
   Engine* e = (Engine*)handle;
   if (!e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "border_tmult_panel: analyze first");
   if (nrhs < 0 || !Z_dev || !T_dev || ldz < e->n_total || ldt < nrhs) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_batch_border_tmult_panel_dev: bad arguments");
   if (e->deterministic) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_border_tmult_panel_dev: deterministic mode sums the panel through pips_hip_kkt_solve_compressed_multi");
   if (nrhs == 0 || e->bt_rows_total == 0) return PIPS_OK;
   HIP_TRY(hipSetDevice(e->device));
   launch_border_tmult_panel(e, Z_dev, ldz, nrhs, T_dev, ldt, alpha);
   HIP_TRY(hipGetLastError());
   return PIPS_OK;
}

int pips_hip_batch_border_mult_panel_dev(void* handle, int nrhs, const double* X0_dev, long long ldx, double* W_dev, long long ldw, double alpha) {
   Engine* e = (Engine*)handle;
   if (!e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "border_mult_panel: analyze first");
   if (nrhs < 0 || !X0_dev || !W_dev || ldx < e->S || ldw < e->n_total) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_batch_border_mult_panel_dev: bad arguments");
   if (nrhs == 0) return PIPS_OK;
   HIP_TRY(hipSetDevice(e->device));
   if (int rc = launch_border_mult_panel(e, X0_dev, ldx, nrhs, W_dev, ldw, alpha)) return rc;
   HIP_TRY(hipGetLastError());
   return PIPS_OK;
}

int pips_hip_batch_inertia(void* handle, int b, int* pos, int* neg, int* zero) {
   Engine* e = (Engine*)handle;
   if (!e || !e->factored || b < 0 || b >= e->nblk) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_inertia: factor first");
   int rc = e->fetch_inertia();
   if (rc) return rc;
   if (pos) *pos = e->h_inertia[3 * b];
   if (neg) *neg = e->h_inertia[3 * b + 1];
   if (zero) *zero = e->h_inertia[3 * b + 2];
   return PIPS_OK;
}

int pips_hip_batch_tail_to_host(void* handle, int b, int which, double* out, int64_t n_out, int* dims) {
   Engine* e = (Engine*)handle;
   if (!e || !e->factored || b < 0 || b >= e->nblk || which < 0 || which > 2) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_tail_to_host: factor first");
   const BlkDesc& bd = e->h_blks[b];
   if (dims) { dims[0] = bd.m; dims[1] = bd.m_pad; dims[2] = bd.nb; dims[3] = bd.ldT; }
   if (!out) return PIPS_OK;
   const double* src = which == 0 ? e->d_arena + bd.T : which == 1 ? e->d_uarena + bd.U : e->d_dtail + bd.dt_off;
   const int64_t n = which == 0 ? (int64_t)bd.ldT * bd.m_pad : which == 1 ? (int64_t)bd.m_pad * bd.m_pad : bd.m_pad;
   if (n_out < n) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_batch_tail_to_host: %lld doubles needed, %lld given", (long long)n, (long long)n_out);
   HIP_TRY(hipSetDevice(e->device));
   HIP_TRY(hipStreamSynchronize(e->stream));
   if (n > 0) HIP_TRY(hipMemcpy(out, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
   return PIPS_OK;
}

int pips_hip_batch_info(void* handle, int64_t* what, int n_what) {
   Engine* e = (Engine*)handle;
   if (!e || e->sym.empty()) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_batch_info: analyze first");
   sym_info(e->sym, what, n_what);
   if (n_what > 13) what[13] = e->border_backward_ok ? 1 : 0;
   if (n_what > 14) what[14] = e->mf ? 1 : 0;
   if (n_what > 15) { what[15] = 0; for (const BlockSym& s : e->sym) what[15] = std::max<int64_t>(what[15], s.mf_max_front); }
   if (n_what > 16) what[16] = e->mfU_total * 8;
   if (n_what > 17) { what[17] = 0; for (const MfLaunch& m : e->mf_launches) if (m.cls >= 6) what[17] += m.cnt; }
   if (n_what > 19) {   // the sparse head alone: stored entries of L and row indices (algorithmic bytes of its factorisation)
      what[18] = what[19] = 0;
      for (const BlockSym& s : e->sym) {
         what[18] += s.nnzL - (int64_t)s.m * (s.m + 1) / 2;
         what[19] += (int64_t)s.rowidx.size();
      }
   }
   if (n_what > 21) {   // entries of L in border rows (head panels / border-row arena + the tails' border rows): read by the sweeps of the
                        // augmented factor, not by a solve with K_i; and whether those sweeps may serve solveCompressed
      what[20] = 0;
      int64_t tail_border = 0;
      for (const BlockSym& s : e->sym) {
         for (const HeadSupernode& hs : s.sn) what[20] += (int64_t)hs.w * (hs.r - hs.rb);   // (counted in nnzL: stored with the head)
         tail_border += (int64_t)s.nb * s.m;                                                   // (not counted in nnzL)
      }
      what[21] = e->aug_sweeps_ok ? 1 : 0;
      if (n_what > 22) what[22] = e->aug_passes;
      if (n_what > 23) what[23] = tail_border;
   }
   if (n_what > 24) { what[24] = 0; for (const BlockSym& s : e->sym) what[24] += s.mf_split ? 1 : 0; }   // blocks with the border split
   if (n_what > 25) { what[25] = 0; for (const BlockSym& s : e->sym) what[25] += (e->mf && s.mf_konly) ? 1 : 0; }   // ... whose fronts hold the rows of K only
   if (n_what > 26) what[26] = e->packed_rhs;   // right-hand sides of the packed blocked solves (Schur mode 2 with the sparse root), else 0
   if (n_what > 27) what[27] = e->tail_first_touch ? 1 : 0;   // the tails are written once, assembled (k_tail_first_touch), not cleared and added to
   return PIPS_OK;
}

int pips_hip_batch_sync(void* handle) {
   Engine* e = (Engine*)handle;
   if (!e) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   HIP_TRY(hipSetDevice(e->device));
   HIP_TRY(hipStreamSynchronize(e->stream));
   return e->sweep.take_error("pips_hip_batch_sync");
}

int pips_hip_batch_set_timing(void* handle, int on) {
   Engine* e = (Engine*)handle;
   if (!e) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   e->timer.on = on != 0;
   return PIPS_OK;
}

int pips_hip_batch_get_timing(void* handle, double* ms, int64_t* cnt, int n) {
   Engine* e = (Engine*)handle;
   if (!e) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   HIP_TRY(hipSetDevice(e->device));
   HIP_TRY(hipStreamSynchronize(e->stream));
   e->timer.collect();
   for (int i = 0; i < n && i < PhaseTimer::NPHASE; ++i) {
      if (ms) ms[i] = e->timer.ms[i];
      if (cnt) cnt[i] = e->timer.cnt[i];
   }
   return PIPS_OK;
}

void pips_hip_batch_destroy(void* handle) { delete (Engine*)handle; }

#include "ldlhandle.hip.h"

// ---- plain device buffers ------------------------------------------------------------------------------------------
// (what the caller holds is owned here under its address, so that it is counted like every other allocation)
static std::mutex g_user_mu;
static std::map<void*, DevBuf<char>>& g_user_bufs = *new std::map<void*, DevBuf<char>>;   // (never destroyed, like the Schur scratch)
int pips_hip_malloc(void** dev_ptr, size_t bytes) {
   if (!dev_ptr) PIPS_FAIL(PIPS_ERR_ARG, "null pointer");
   DevBuf<char> b;
   PIPS_TRY(b.alloc(bytes ? bytes : 8));
   *dev_ptr = b.get();
   std::lock_guard<std::mutex> lock(g_user_mu);
   g_user_bufs[*dev_ptr] = std::move(b);
   return PIPS_OK;
}
int pips_hip_free(void* dev_ptr) {
   std::lock_guard<std::mutex> lock(g_user_mu);
   if (dev_ptr && !g_user_bufs.erase(dev_ptr)) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_free: not a pointer of pips_hip_malloc");
   return PIPS_OK;
}
int pips_hip_memcpy_h2d(void* dst, const void* src, size_t bytes) {
   HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
   return PIPS_OK;
}
int pips_hip_memcpy_d2h(void* dst, const void* src, size_t bytes) {
   HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
   return PIPS_OK;
}
int pips_hip_memset(void* dst, int value, size_t bytes) {
   HIP_TRY(hipMemset(dst, value, bytes));
   return PIPS_OK;
}

// ---- fused KKT system (kkt.hip.h) ---------------------------------------------------------------------------------
int pips_hip_kkt_create(void** handle, void* batch, int n0, int my0, int myl, int mzl, const int* A0_rowptr,
                        const int* A0_colidx, const double* A0_val, const int* F0_rowptr, const int* F0_colidx,
                        const double* F0_val, const int* G0_rowptr, const int* G0_colidx, const double* G0_val, void* comm,
                        int rank, int n_ranks) {
   Engine* e = (Engine*)batch;
   if (!handle || !e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_create: the leaf batch must be analyzed first");
   HIP_TRY(hipSetDevice(e->device));
   const RootRows rows[3] = {{A0_rowptr, A0_colidx, A0_val, my0, n0}, {F0_rowptr, F0_colidx, F0_val, myl, n0 + my0}, {G0_rowptr, G0_colidx, G0_val, mzl, n0 + my0 + myl}};
   return KktSystem::create(handle, e, "pips_hip_kkt_create", false, n0, my0, myl, mzl, rows, 0, nullptr, nullptr, comm, rank, n_ranks);
}

// Sparse root (KktSystem::init_sparse_root).  blk_cols_ptr / blk_cols (optional): the border column sets of ALL blocks of the problem
// (needed with n_ranks > 1, where a rank only knows its own blocks but every rank must reduce the same value array); NULL: the blocks
// of this batch.
int pips_hip_kkt_create_sparse(void** handle, void* batch, int n0, int my0, int myl, int mzl, const int* A0_rowptr,
                               const int* A0_colidx, const double* A0_val, const int* F0_rowptr, const int* F0_colidx,
                               const double* F0_val, const int* G0_rowptr, const int* G0_colidx, const double* G0_val,
                               int n_blocks_global, const int* blk_cols_ptr, const int* blk_cols, void* comm, int rank,
                               int n_ranks) {
   Engine* e = (Engine*)batch;
   if (!handle || !e || !e->analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_create_sparse: the batch must be analyzed");
   HIP_TRY(hipSetDevice(e->device));
   const RootRows rows[3] = {{A0_rowptr, A0_colidx, A0_val, my0, n0}, {F0_rowptr, F0_colidx, F0_val, myl, n0 + my0}, {G0_rowptr, G0_colidx, G0_val, mzl, n0 + my0 + myl}};
   return KktSystem::create(handle, e, "pips_hip_kkt_create_sparse", true, n0, my0, myl, mzl, rows, n_blocks_global, blk_cols_ptr, blk_cols, comm, rank, n_ranks);
}

int pips_hip_kkt_factorize(void* handle, const double* leaf_diag_dev, const double* xdiag0_dev, const double* zdiag_link_dev) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   HIP_TRY(hipSetDevice(k->leaves->device));
   return k->factorize(leaf_diag_dev, xdiag0_dev, zdiag_link_dev);
}

int pips_hip_kkt_set_root_regularization(void* handle, double primal, double dual) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || primal < 0.0 || dual < 0.0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_set_root_regularization: bad arguments");
   k->root_reg_primal = primal;
   k->root_reg_dual = dual;
   return PIPS_OK;
}

int pips_hip_kkt_solve_compressed(void* handle, double* b0_dev, double* b_leaf_dev) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || !b0_dev || !b_leaf_dev) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_solve_compressed: bad arguments");
   HIP_TRY(hipSetDevice(k->leaves->device));
   return k->solve_compressed(b0_dev, b_leaf_dev);
}

int pips_hip_kkt_solve_compressed_multi(void* handle, int nrhs, double* B0_dev, long long ld0, double* Bleaf_dev, long long ldl) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_solve_compressed_multi: null handle");
   if (nrhs < 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_solve_compressed_multi: nrhs = %d is negative", nrhs);
   if (k->factor_gen == 0) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_solve_compressed_multi: pips_hip_kkt_factorize first");
   if (nrhs == 0) return PIPS_OK;   // (no column is touched: the pointers of an empty set may be anything)
   if (!B0_dev || !Bleaf_dev) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_solve_compressed_multi: %s is NULL", !B0_dev ? "B0_dev" : "Bleaf_dev");
   if (ld0 < k->S + k->mz0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_solve_compressed_multi: ld0 = %lld is below S + mz0 = %d", ld0, k->S + k->mz0);
   if (ldl < k->leaves->n_total) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_solve_compressed_multi: ldl = %lld is below n_total = %lld", ldl, (long long)k->leaves->n_total);
   HIP_TRY(hipSetDevice(k->leaves->device));
   return k->solve_compressed_multi(nrhs, B0_dev, ld0, Bleaf_dev, ldl);
}

int pips_hip_kkt_solve_multi_info(void* handle, int64_t* what, int n_what) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || !what || n_what < 1) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_solve_multi_info: bad arguments");
   for (int i = 0; i < n_what; ++i) what[i] = i < 6 ? k->multi_info[i] : 0;
   return PIPS_OK;
}

int pips_hip_kkt_set_root_stream(void* handle, int own_stream) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   int rc = k->root_wait();
   if (rc) return rc;
   k->root_own_stream = own_stream != 0;
   return PIPS_OK;
}

int pips_hip_kkt_set_solve_graph(void* handle, int on) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   k->solve_graph = on != 0;
   if (!on && k->graph_exec) { (void)hipGraphExecDestroy(k->graph_exec); k->graph_exec = nullptr; }
   return PIPS_OK;
}

int pips_hip_kkt_solve_graph_stats(void* handle, int64_t* captures, int64_t* replays) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   if (captures) *captures = k->graph_captures;
   if (replays) *replays = k->graph_replays;
   return PIPS_OK;
}

int pips_hip_kkt_set_solve_check(void* handle, int every) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || every < 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_set_solve_check: bad arguments");
   k->solve_check_every = every;
   k->sweeps_since_check = 0;
   return PIPS_OK;
}

int pips_hip_kkt_solve_check_counts(void* handle, long long* checked, long long* failed) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   if (checked) *checked = k->checked_solves;
   if (failed) *failed = k->failed_checks;
   return PIPS_OK;
}

int pips_hip_kkt_last_solve_path(void* handle, int* path) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || !path) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_last_solve_path: bad arguments");
   *path = k->last_solve_path;
   return PIPS_OK;
}

int pips_hip_kkt_last_ltsolve_from_factor(void* handle, int* flag) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || !flag) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_last_ltsolve_from_factor: bad arguments");
   *flag = k->last_ltsolve_from_factor ? 1 : 0;
   return PIPS_OK;
}

int pips_hip_kkt_get_timing(void* handle, double* ms, int64_t* cnt, int n) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   HIP_TRY(hipSetDevice(k->leaves->device));
   HIP_TRY(hipStreamSynchronize(k->leaves->stream));
   if (k->root_stream) HIP_TRY(hipStreamSynchronize(k->root_stream));
   k->timer.collect();
   for (int i = 0; i < n && i < PhaseTimer::NPHASE; ++i) {
      if (ms) ms[i] = k->timer.ms[i];
      if (cnt) cnt[i] = k->timer.cnt[i];
   }
   return PIPS_OK;
}

int pips_hip_kkt_set_root_inequalities(void* handle, int mz0, const int* C0_rowptr, const int* C0_colidx, const double* C0_val) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || mz0 < 0 || (mz0 > 0 && (!C0_rowptr || !C0_colidx || !C0_val))) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_set_root_inequalities: bad arguments");
   HIP_TRY(hipSetDevice(k->leaves->device));
   return k->set_root_inequalities(mz0, C0_rowptr, C0_colidx, C0_val);
}

int pips_hip_kkt_set_root_hessian(void* handle, const int* Q0_rowptr, const int* Q0_colidx, const double* Q0_val) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || (Q0_rowptr && k->n0 > 0 && Q0_rowptr[k->n0] > Q0_rowptr[0] && (!Q0_colidx || !Q0_val)))
      PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_set_root_hessian: bad arguments");
   HIP_TRY(hipSetDevice(k->leaves->device));
   return k->set_root_hessian(Q0_rowptr, Q0_colidx, Q0_val);
}

int pips_hip_kkt_set_root_pivoting(void* handle, int mode) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || mode < 0 || mode > 1) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_set_root_pivoting: mode 0 (static order) or 1 (Bunch-Kaufman inside the diagonal tiles)");
   if (k->sparse) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_set_root_pivoting: the sparse root is factorised by the leaf engine (static pivot order)");
   k->root->pivoting = mode;
   k->root_pivoting_set = true;
   return PIPS_OK;
}

int pips_hip_kkt_set_zdiag0_dev(void* handle, const double* zdiag0_dev) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   k->d_zdiag0 = zdiag0_dev;
   return PIPS_OK;
}

int pips_hip_kkt_get_schur(void* handle, double** SC_dev, int* ld) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   if (k->sparse) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_get_schur: sparse-root system, use pips_hip_kkt_get_schur_sparse");
   if (SC_dev) *SC_dev = k->d_SC;
   if (ld) *ld = k->S;
   return PIPS_OK;
}

int pips_hip_kkt_root_inertia(void* handle, int* pos, int* neg, int* zero) {
   KktSystem* k = (KktSystem*)handle;
   if (!k) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   int rcw = k->root_wait();
   if (rcw) return rcw;
   if (k->sparse) return pips_hip_batch_inertia(k->root_sp.get(), 0, pos, neg, zero);
   return pips_hip_dense_ldl_inertia(k->root.get(), pos, neg, zero);
}

int pips_hip_kkt_get_schur_sparse(void* handle, int* nnz, int* rowptr, int* colidx, double* val_host) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || !k->sparse) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_get_schur_sparse: not a sparse-root system");
   const int n = k->sc_rowptr[k->S];
   if (nnz) *nnz = n;
   if (rowptr) std::copy(k->sc_rowptr.begin(), k->sc_rowptr.end(), rowptr);
   if (colidx) std::copy(k->sc_colidx.begin(), k->sc_colidx.end(), colidx);
   if (val_host) {
      HIP_TRY(hipSetDevice(k->leaves->device));
      HIP_TRY(hipStreamSynchronize(k->leaves->stream));
      HIP_TRY(hipMemcpy(val_host, k->root_sp->d_kval, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
   }
   return PIPS_OK;
}

// sparse root: what[0] = elimination order taken (0 minimum degree, 1 dense-tile band, 2 dissection around x0 / y0), then the entries
// of pips_hip_batch_info for the root's one-block engine (what[1 + i] = info[i])
int pips_hip_kkt_sparse_root_info(void* handle, int64_t* what, int n_what) {
   KktSystem* k = (KktSystem*)handle;
   if (!k || !what || n_what < 1) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_sparse_root_info: bad arguments");
   if (!k->sparse || !k->root_sp) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_sparse_root_info: not a sparse-root system");
   what[0] = k->root_order_mode;
   return n_what > 1 ? pips_hip_batch_info(k->root_sp.get(), what + 1, n_what - 1) : PIPS_OK;
}

void pips_hip_kkt_destroy(void* handle) { delete (KktSystem*)handle; }

}  // extern "C"
