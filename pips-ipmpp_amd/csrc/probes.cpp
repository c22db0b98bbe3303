// The CPU-only probes of the C ABI (include/pips_hip.h): the symbolic analysis, the host layout and the host plans as Engine::analyze
// forms them, handed out as integers.  Plain C++, no device call: the tests without a GPU go through these.
#include <algorithm>
#include <thread>
#include <vector>

#include "common.h"
#include "layout.h"
#include "detplan.h"
#include "tileplan.h"
#include "multiplan.h"
#include "knobs.h"
#include "pips_hip.h"

#define PIPS_TRY(expr)                    \
   do {                                   \
      if (int _rc = (expr)) return _rc;   \
   } while (0)

using namespace pips;

extern "C" {

// ---- symbolic probe (CPU only) -------------------------------------------------------------------------------------
int pips_symbolic_probe(int n, int n_primal, const int* krow, const int* jcol, int S, const int* Bt_rowptr,
                        const int* Bt_colidx, int force_n_head, int64_t* what, int n_what, int* perm, int* colcount) {
   if (n <= 0 || !krow || !jcol) PIPS_FAIL(PIPS_ERR_ARG, "pips_symbolic_probe: bad arguments");
   AnalyzeOptions opt;
   AnalyzeKnobs knobs;
   read_layout_knobs(nullptr, opt, knobs);
   opt.force_n_head = force_n_head;
   CsrPattern K{n, n, krow, jcol};
   CsrPattern B{0, n, nullptr, nullptr};
   if (Bt_rowptr && S > 0) B = CsrPattern{S, n, Bt_rowptr, Bt_colidx};
   std::vector<BlockSym> sym(1);
   int rc = analyze_block(K, B, n_primal, opt, sym[0]);
   if (rc) return rc;
   if (what) sym_info(sym, what, n_what);
   if (what && n_what > 16) {   // multifrontal head: usable, border split taken, doubles of update matrices, doubles of border rows kept beside the panels
      const BlockSym& bs = sym[0];
      what[13] = bs.mf_ok ? 1 : 0;
      what[14] = bs.mf_split ? (bs.mf_konly ? 2 : 1) : 0;
      what[15] = bs.mf_U_total;
      what[16] = 0;
      for (const HeadSupernode& hs : bs.sn) if (hs.ld < hs.w + hs.r) what[16] += (int64_t)hs.w * (hs.r - hs.rb);
   }
   if (const char* dump = knob_text<K_DUMP_SN>()) {   // development aid
      if (FILE* f = fopen(dump, "w")) {
         const BlockSym& bs = sym[0];
         for (size_t si = 0; si < bs.sn.size(); ++si) {
            const HeadSupernode& s = bs.sn[si];
            const int* rows = bs.rowidx.data() + s.rows;
            int nh = 0, nt = 0;
            for (int a = 0; a < s.r; ++a) { if (rows[a] < bs.n_head) ++nh; else if (rows[a] < bs.n) ++nt; }
            // c0 w r level rows-in-head rows-in-tail border-rows update-segments parent-supernode (index, -1: none in the head)
            fprintf(f, "%d %d %d %d %d %d %d %d %d\n", s.c0, s.w, s.r, s.level, nh, nt, s.r - nh - nt, s.n_useg,
                    si < bs.sn_parent.size() ? bs.sn_parent[si] : -1);
         }
         fclose(f);
         fprintf(stderr, "[pips_hip] multifrontal: ok %d, largest front %d, update matrices %lld doubles, records %zu ints\n", (int)bs.mf_ok, bs.mf_max_front,
                 (long long)bs.mf_U_total, bs.mf_int.size());
         if (bs.mf_konly) {   // gather-form records: pairs per front and their sizes, level by level
            std::vector<long long> lp, lf, lmax, lwork;
            long long pairs = 0, fronts = 0, work = 0, rowsum = 0;
            for (size_t si = 0; si < bs.sn.size(); ++si) {
               if (bs.kb_off[si] < 0) continue;
               const HeadSupernode& s = bs.sn[si];
               const int* R = bs.kb_rec.data() + bs.kb_off[si];
               if ((int)lp.size() <= s.level) { lp.resize(s.level + 1, 0); lf.resize(s.level + 1, 0); lmax.resize(s.level + 1, 0); lwork.resize(s.level + 1, 0); }
               long long wk = 0;
               for (int q = 0; q < R[0]; ++q) {
                  const HeadSupernode& c = bs.sn[R[2 + 2 * q]];
                  const int ns = (R[3 + 2 * q] >> 16) - (R[3 + 2 * q] & 0xffff);
                  wk += (long long)(c.r - c.rb) * ns * c.w;
                  rowsum += c.r - c.rb;
               }
               lp[s.level] += R[0]; ++lf[s.level]; lmax[s.level] = std::max<long long>(lmax[s.level], R[0]); lwork[s.level] += wk;
               pairs += R[0]; ++fronts; work += wk;
            }
            fprintf(stderr, "[pips_hip] gather-form border rows: %lld fronts, %lld pairs (%.1f border rows each), %lld multiply-adds, %zu tail runs\n", fronts, pairs,
                    pairs ? (double)rowsum / pairs : 0.0, work, bs.kb_tail.size() / 2);
            for (size_t l = 0; l < lp.size(); ++l)
               fprintf(stderr, "   level %2zu: %6lld fronts %7lld pairs, most %4lld, %9lld multiply-adds\n", l, lf[l], lp[l], lmax[l], lwork[l]);
         }
      }
   }
   if (perm) std::copy(sym[0].perm.begin(), sym[0].perm.end(), perm);
   if (colcount) std::copy(sym[0].colcount.begin(), sym[0].colcount.end(), colcount);
   return PIPS_OK;
}

// the order the sparse root takes for a chain-like Schur complement (hub_dissected_order: hubs last, the rest dissected) and the
// symbolic analysis under it; PIPS_ERR_STATE when the graph without the hubs has no separators
int pips_symbolic_probe_hubs(int n, int n_primal, const int* krow, const int* jcol, int n_hubs, const int* hubs, int min_size, int64_t* what,
                             int n_what, int* perm, int* colcount) {
   if (n <= 0 || !krow || !jcol || n_hubs < 0 || (n_hubs > 0 && !hubs)) PIPS_FAIL(PIPS_ERR_ARG, "pips_symbolic_probe_hubs: bad arguments");
   std::vector<int> ap(n + 1, 0), ai;
   for (int r = 0; r < n; ++r)
      for (int p = krow[r]; p < krow[r + 1]; ++p) {
         if (jcol[p] < 0 || jcol[p] > r) PIPS_FAIL(PIPS_ERR_ARG, "pips_symbolic_probe_hubs: K must be lower-triangular CSR");
         if (jcol[p] != r) { ++ap[r + 1]; ++ap[jcol[p] + 1]; }
      }
   for (int i = 0; i < n; ++i) ap[i + 1] += ap[i];
   ai.resize(ap[n]);
   {
      std::vector<int> fill(ap.begin(), ap.end() - 1);
      for (int r = 0; r < n; ++r)
         for (int p = krow[r]; p < krow[r + 1]; ++p)
            if (jcol[p] != r) { ai[fill[r]++] = jcol[p]; ai[fill[jcol[p]]++] = r; }
   }
   std::vector<int> hv(hubs, hubs + n_hubs), pv, cc;
   if (!hub_dissected_order(n, ap, ai, hv, min_size, pv, cc)) PIPS_FAIL(PIPS_ERR_STATE, "pips_symbolic_probe_hubs: no separators");
   AnalyzeOptions opt;
   AnalyzeKnobs knobs;
   read_layout_knobs(nullptr, opt, knobs);
   opt.mf_konly = false;   // (the sparse root's order: plain fronts)
   opt.user_perm = pv.data();
   opt.user_colcount = cc.data();
   {  // (the cut pips_hip_kkt_create_sparse takes)
      int cut = 0;
      while (cut < n - n_hubs && cc[cut] <= ROOT_ND_MAX_COLCOUNT) ++cut;
      opt.force_n_head = cut;
   }
   CsrPattern K{n, n, krow, jcol};
   CsrPattern B{0, n, nullptr, nullptr};
   std::vector<BlockSym> sym(1);
   int rc = analyze_block(K, B, n_primal, opt, sym[0]);
   if (rc) return rc;
   if (what) sym_info(sym, what, n_what);
   if (perm) std::copy(sym[0].perm.begin(), sym[0].perm.end(), perm);
   if (colcount) std::copy(sym[0].colcount.begin(), sym[0].colcount.end(), colcount);
   return PIPS_OK;
}

// ---- layout probe (CPU only): symbolic analysis and host layout of a batch as Engine::analyze forms them, and the layout's invariants
static int probe_inputs(const char* who, int nblk, const int* n, const int* n_primal, const int* const* krow, const int* const* kcol, int S,
                        const int* const* bt_rowptr, const int* const* bt_colidx, std::vector<BlockInput>& in) {
   if (nblk <= 0 || !n || !krow || !kcol || S < 0) PIPS_FAIL(PIPS_ERR_ARG, "%s: bad arguments", who);
   in.assign(nblk, BlockInput());
   for (int b = 0; b < nblk; ++b) {
      if (n[b] <= 0 || !krow[b] || !kcol[b]) PIPS_FAIL(PIPS_ERR_ARG, "%s: block %d is empty", who, b);
      in[b].n = n[b];
      in[b].n_primal = n_primal ? n_primal[b] : -1;
      in[b].krow.assign(krow[b], krow[b] + n[b] + 1);
      in[b].kcol.assign(kcol[b], kcol[b] + krow[b][n[b]]);
      if (S > 0 && bt_rowptr && bt_colidx && bt_rowptr[b] && bt_colidx[b]) {
         in[b].btrow.assign(bt_rowptr[b], bt_rowptr[b] + S + 1);
         in[b].btcol.assign(bt_colidx[b], bt_colidx[b] + bt_rowptr[b][S]);
         in[b].btval.assign(in[b].btcol.size(), 0.0);
      }
   }
   return PIPS_OK;
}

int pips_layout_probe(int nblk, const int* n, const int* n_primal, const int* const* krow, const int* const* kcol, int S,
                      const int* const* bt_rowptr, const int* const* bt_colidx, int deterministic, long long free_device_bytes,
                      int64_t* what, int n_what) {
   std::vector<BlockInput> in;
   PIPS_TRY(probe_inputs("pips_layout_probe", nblk, n, n_primal, krow, kcol, S, bt_rowptr, bt_colidx, in));
   AnalyzeOptions opt;
   AnalyzeKnobs knobs;
   read_layout_knobs(nullptr, opt, knobs);
   if (deterministic) { knobs.deterministic = true; opt.mf_konly = false; }
   knobs.free_device_bytes = free_device_bytes;
   std::vector<BlockSym> sym;
   BatchLayout lay;
   const int n_threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
   int rc = analyze_symbolic(in, S, n_threads, opt, knobs, sym);
   if (!rc) rc = build_batch_layout(in, sym, S, knobs, lay);
   if (!rc) rc = check_batch_layout(in, sym, S, knobs, lay);
   if (rc) return rc;
   int64_t v[21] = {lay.arena_total, lay.xw_total, lay.uarena_total, lay.nsn_total, (int64_t)lay.levels.size(), (int64_t)lay.levels_top.size(),
                    (int64_t)lay.mf_launches.size(), 0, lay.n_bb, lay.bb_stage, lay.tail_single, lay.border_backward_ok, lay.aug_sweeps_ok,
                    lay.slots_total, lay.vslots_total, lay.n_total, lay.mf, lay.schur_mode_eff, lay.bb_doubles, lay.mfU_total, lay.spine_total};
   for (const MfLaunch& m : lay.mf_launches) if (m.cls >= 6) v[7] += m.cnt;
   for (int i = 0; what && i < n_what && i < 21; ++i) what[i] = v[i];
   return PIPS_OK;
}

// ---- tail plan probe (CPU only): the task plans of a leaf batch's launch-per-step tail factorisation as Engine::analyze forms them - the
// column plan (ColumnPlan) and its regrouping by groups of tile columns (GroupPlan) - as rows of integers (include/pips_hip.h)
int pips_tail_plan_probe(int nblk, const int* n, const int* n_primal, const int* const* krow, const int* const* kcol, int S,
                         const int* const* bt_rowptr, const int* const* bt_colidx, int force_n_head, int* col_tasks, long long col_cap,
                         int* grp_tasks, long long grp_cap, int64_t* counts) {
   std::vector<BlockInput> in;
   PIPS_TRY(probe_inputs("pips_tail_plan_probe", nblk, n, n_primal, krow, kcol, S, bt_rowptr, bt_colidx, in));
   if (!counts || col_cap < 0 || grp_cap < 0 || (col_cap > 0 && !col_tasks) || (grp_cap > 0 && !grp_tasks))
      PIPS_FAIL(PIPS_ERR_ARG, "pips_tail_plan_probe: bad arguments");
   AnalyzeOptions opt;
   AnalyzeKnobs knobs;
   read_layout_knobs(nullptr, opt, knobs);
   opt.force_n_head = force_n_head;
   knobs.free_device_bytes = 0;
   std::vector<BlockSym> sym;
   BatchLayout lay;
   const int n_threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
   PIPS_TRY(analyze_symbolic(in, S, n_threads, opt, knobs, sym));
   PIPS_TRY(build_batch_layout(in, sym, S, knobs, lay));
   ColumnPlan plan;
   plan.build_leaf(lay.h_blks, lay.tile_first, 4);
   GroupPlan pp;
   pp.build(plan, 4);
   long long nc = 0, ng = 0, launches_col = 0, launches_grp = 0;
   auto col = [&](const TaskList& l, int kind) {
      launches_col += l.cnt > 0;
      for (long long q = l.off; q < l.off + l.cnt; ++q, ++nc) {
         const TileTask& t = plan.h_tasks[q];
         if (nc < col_cap) { int* r = col_tasks + 6 * nc; r[0] = kind; r[1] = t.blk; r[2] = t.ti; r[3] = t.tj; r[4] = t.pad & 0xffff; r[5] = t.pad >> 16; }
      }
   };
   auto grp = [&](long long off, int cnt, int list, int group, int index) {
      for (int q = 0; q < cnt; ++q, ++ng) {
         const TileTask& t = pp.h_tasks[off + q];
         if (ng < grp_cap) {
            int* r = grp_tasks + 9 * ng;
            r[0] = list; r[1] = group; r[2] = index; r[3] = q; r[4] = t.blk; r[5] = t.ti; r[6] = t.tj; r[7] = t.pad & 0xffff; r[8] = t.pad >> 16;
         }
      }
   };
   auto grp_list = [&](const TaskList& l, int list, int group, int index) { launches_grp += l.cnt > 0; grp(l.off, l.cnt, list, group, index); };
   for (int j = 0; j < plan.ntc_max; ++j) {
      col(plan.upd_diag[j], 0);
      col(plan.upd[j], 0);
      launches_col += plan.diag[j].cnt > 0;
      col(plan.trsm[j], 1);
   }
   for (int i = 0; i < pp.n_groups; ++i) {
      grp_list(pp.deep[i], 0, i, 0);
      grp_list(pp.pre[i], 1, i, 0);
      grp_list(pp.block_deep[i], 2, i, 0);
      for (int j = i * pp.P; j < std::min((i + 1) * pp.P, plan.ntc_max); ++j) {
         grp_list(pp.upd_in[j], 3, i, j);
         launches_grp += plan.diag[j].cnt > 0;
         grp_list(pp.trsm_in[j], 4, i, j);
      }
      launches_grp += pp.strips[i].cnt > 0;
      for (int q = 0; q < pp.strips[i].cnt; ++q) {
         const TileStrip& st = pp.h_strips[pp.strips[i].off + q];
         grp(st.off, st.cnt, 5, i, q);
      }
   }
   counts[0] = nc; counts[1] = ng; counts[2] = plan.ntc_max; counts[3] = pp.n_groups; counts[4] = launches_col; counts[5] = launches_grp;
   return PIPS_OK;
}

// ---- first-touch plan probe (CPU only): the layout of a batch twice - with the first touch of the tails refused (PIPS_HIP_TAIL_FIRST_TOUCH=0
// does the same) and as the analysis decides it - as sections of integers (include/pips_hip.h)
int pips_first_touch_probe(int nblk, const int* n, const int* n_primal, const int* const* krow, const int* const* kcol, int S,
                           const int* const* bt_rowptr, const int* const* bt_colidx, int force_n_head, int deterministic, long long lds_bytes,
                           long long free_device_bytes, long long* out, long long cap, int64_t* counts) {
   std::vector<BlockInput> in;
   PIPS_TRY(probe_inputs("pips_first_touch_probe", nblk, n, n_primal, krow, kcol, S, bt_rowptr, bt_colidx, in));
   if (!counts || cap < 0 || (cap > 0 && !out)) PIPS_FAIL(PIPS_ERR_ARG, "pips_first_touch_probe: bad arguments");
   AnalyzeOptions opt;
   AnalyzeKnobs knobs;
   read_layout_knobs(nullptr, opt, knobs);
   if (deterministic) { knobs.deterministic = true; opt.mf_konly = false; }   // (as pips_layout_probe)
   opt.force_n_head = force_n_head;
   knobs.free_device_bytes = free_device_bytes;
   if (lds_bytes > 0) knobs.ft_lds_bytes = lds_bytes;
   std::vector<BlockSym> sym;
   BatchLayout old, lay;
   const int n_threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
   PIPS_TRY(analyze_symbolic(in, S, n_threads, opt, knobs, sym));
   PIPS_TRY(build_batch_layout(in, sym, S, knobs, lay));
   PIPS_TRY(check_batch_layout(in, sym, S, knobs, lay));
   knobs.tail_first_touch = 0;
   PIPS_TRY(build_batch_layout(in, sym, S, knobs, old));
   long long at = 0;
   int section = 0;
   auto put = [&](long long v) { if (at < cap) out[at] = v; ++at; };
   long long from = 0;
   auto end = [&]() { counts[8 + section++] = at - from; from = at; };
   for (int b = 0; b < nblk; ++b) {
      const BlkDesc& d = lay.h_blks[b];
      put(d.n); put(d.n_head); put(d.m); put(d.m_pad); put(d.nb); put(d.ldT); put(d.mf_split); put(d.T_in); put(lay.kptr[b]);
      put((long long)in[b].btcol.size()); put(lay.mf ? lay.h_root_off[b + 1] - lay.h_root_off[b] : 0); put(d.ntc);
   }
   end();
   for (long long v : lay.h_ft_colbase) put(v);
   end();
   for (int v : lay.h_ft_init_off) put(v);
   end();
   for (const FtInit& e : lay.h_ft_init) { put(e.row); put(e.src); }
   end();
   for (int v : lay.h_ft_piece_off) put(v);
   end();
   for (const FtPiece& e : lay.h_ft_piece) { put(e.front); put(e.u); put(e.rows); put(e.cnt); }
   end();
   for (int v : lay.h_ft_leaves) put(v);
   end();
   for (long long v : old.h_kdst) put(v);
   end();
   for (long long v : lay.h_kdst) put(v);
   end();
   for (long long v : old.h_bdst) put(v);
   end();
   for (long long v : lay.h_bdst) put(v);
   end();
   for (int b = 0; b < nblk && lay.mf; ++b)   // the root fronts k_root_assemble walks, in its order
      for (int q = lay.h_root_off[b]; q < lay.h_root_off[b + 1]; ++q) {
         const SnDesc& sn = lay.h_sns[lay.h_roots[q]];
         put(b); put(lay.h_roots[q]); put(sn.r); put(sn.rb); put(sn.U); put(sn.rows);
      }
   end();
   for (int v : lay.h_rowidx) put(v);
   end();
   if (!lay.levels.empty()) {   // the simple leaves
      const LevelRange& L0 = lay.levels[0];
      for (int i = L0.simple_begin; i < L0.simple_begin + L0.simple_cnt; ++i) {
         const SnDesc& sn = lay.h_sns[i];
         put(i); put(sn.blk); put(sn.r); put(sn.n_useg); put(sn.rows);
      }
   }
   end();
   const int64_t head[8] = {lay.tail_first_touch, lay.mf, lay.tail_single, lay.schur_mode_eff, lay.mfU_total, lay.nnzK_total, lay.nnzB_total, at};
   std::copy(head, head + 8, counts);
   return PIPS_OK;
}

// ---- plan probe of deterministic mode (CPU only): the layout of a deterministic analysis, then the planners of detplan.h that need no
// recording, as Engine::upload_layout / set_det_groups / set_sc_panels call them - sections of integers (include/pips_hip.h)
int pips_det_plan_probe(int nblk, const int* n, const int* n_primal, const int* const* krow, const int* const* kcol, int S,
                        const int* const* bt_rowptr, const int* const* bt_colidx, int rank, int n_ranks, int n_panels, long long* out,
                        long long cap, int64_t* counts) {
   std::vector<BlockInput> in;
   PIPS_TRY(probe_inputs("pips_det_plan_probe", nblk, n, n_primal, krow, kcol, S, bt_rowptr, bt_colidx, in));
   if (!counts || cap < 0 || (cap > 0 && !out) || n_ranks < 1 || rank < 0 || rank >= n_ranks) PIPS_FAIL(PIPS_ERR_ARG, "pips_det_plan_probe: bad arguments");
   AnalyzeOptions opt;
   AnalyzeKnobs knobs;
   read_layout_knobs(nullptr, opt, knobs);
   knobs.deterministic = true; opt.mf_konly = false;   // (as pips_layout_probe with deterministic set)
   knobs.free_device_bytes = 0;
   std::vector<BlockSym> sym;
   BatchLayout lay;
   const int n_threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
   PIPS_TRY(analyze_symbolic(in, S, n_threads, opt, knobs, sym));
   PIPS_TRY(build_batch_layout(in, sym, S, knobs, lay));
   const BorderGathers bg = lay.bt_rows_total > 0 ? border_product_gathers(lay) : BorderGathers();
   const DetGroupPlan p = build_det_group_plan(lay, sym, S, rank, n_ranks, (long long)S * S, ScKept(), PackedTables());
   const ScPanelPlan sp = sc_panel_plan(lay, sym, S, n_panels);
   long long at = 0;
   int section = 0;
   auto put = [&](long long v) { if (at < cap) out[at] = v; ++at; };
   auto end = [&](long long& from) { counts[16 + section++] = at - from; from = at; };
   auto gather = [&](const HostGather& g) {
      put((long long)g.tgt.size());
      for (long long v : g.tgt) put(v);
      for (long long v : g.off) put(v);
      for (long long v : g.slots) put(v);
   };
   long long from = 0, aug_rows = 0;
   for (const SnDesc& sn : lay.h_sns) aug_rows += sn.r - sn.rb;
   for (int b = 0; b < nblk; ++b) put(p.grp[b]);
   end(from);
   for (int b = 0; b < nblk; ++b) {
      const BlkDesc& d = lay.h_blks[b];
      put(d.ntc); put(d.nb); put(d.nb_pad); put(lay.mf ? lay.h_root_off[b + 1] - lay.h_root_off[b] : 0);
      put(lay.n_bb > 0 ? lay.h_bb_off[b + 1] - lay.h_bb_off[b] : 0); put((long long)sym[b].bmap.size());
   }
   end(from);
   for (size_t k = 0; k < p.rounds.size(); ++k)
      for (long long q = p.rounds[k].off; q < p.rounds[k].off + p.rounds[k].cnt; ++q) { put((long long)k); put(p.tasks[q].blk); put(p.tasks[q].ti); put(p.tasks[q].tj); }
   end(from);
   for (size_t k = 0; k + 1 < p.round_off.size(); ++k)
      for (int q = p.round_off[k]; q < p.round_off[k + 1]; ++q) { put((long long)k); put(p.round_blk[q]); }
   end(from);
   for (size_t k = 0; k + 1 < p.bb_round_off.size(); ++k)
      for (int q = p.bb_round_off[k]; q < p.bb_round_off[k + 1]; ++q) { put((long long)k); put(p.bb_round_blk[q]); }
   end(from);
   gather(p.btm_grp); end(from);
   gather(bg.btm); end(from);
   gather(bg.bm); end(from);
   gather(p.aug.bslot_grp); end(from);
   for (const BgEntry& e : p.aug.ent) { put(e.off); put(e.y); put(e.stride); put(e.w); }
   end(from);
   for (long long v : p.aug.ptr) put(v);
   end(from);
   for (int v : p.aug.idx) put(v);
   end(from);
   for (long long v : p.aug.slot) put(v);
   end(from);
   for (int v : sp.row_begin) put(v);
   end(from);
   for (size_t g = 0; g < sp.groups.size(); ++g)
      for (long long q = sp.groups[g].off; q < sp.groups[g].off + sp.groups[g].cnt; ++q) { put((long long)g); put(sp.tasks[q].blk); put(sp.tasks[q].ti); put(sp.tasks[q].tj); }
   end(from);
   for (int b = 0; b < nblk; ++b)
      for (int v : sym[b].bmap) put(v);
   end(from);
   const int64_t head[16] = {p.n_groups, p.first_slot, p.slots, p.global, p.aug.ready, p.aug_sweeps_ok, lay.aug_sweeps_ok, lay.mf, lay.n_bb, lay.n_roots,
                             lay.schur_mode_eff, (int64_t)sp.groups.size(), p.aug.n_targets, p.aug.n_ent, aug_rows, at};
   std::copy(head, head + 16, counts);
   return PIPS_OK;
}
// ---- the chunks of pips_hip_kkt_solve_compressed_multi (multiplan.h), as the call cuts them -------------------------------------------
int pips_kkt_multi_plan_probe(int nrhs, int from, int chunk_max, long long n_total, long long budget_bytes, int* out, int cap, int* n_chunks) {
   if (nrhs < 0 || from < 0 || chunk_max < 1 || n_total < 0 || budget_bytes < 0 || !n_chunks || cap < 0 || (cap > 0 && !out))
      PIPS_FAIL(PIPS_ERR_ARG, "pips_kkt_multi_plan_probe: bad arguments");
   const std::vector<KktMultiChunk> plan = kkt_multi_plan(nrhs, from, chunk_max, n_total, budget_bytes);
   *n_chunks = (int)plan.size();
   if ((size_t)cap >= plan.size())
      for (size_t i = 0; i < plan.size(); ++i) { out[3 * i] = plan[i].first; out[3 * i + 1] = plan[i].count; out[3 * i + 2] = plan[i].path; }
   return PIPS_OK;
}

}  // extern "C"
