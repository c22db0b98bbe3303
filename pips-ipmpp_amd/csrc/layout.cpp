// Host pass of a batch analysis (layout.h): the steps of the former Engine::analyze() up to its uploads, in their order.
// The arithmetic is the engine's: same loops, same order of pushes, same tie-breaks - deterministic mode's bits depend on list order.
#include "layout.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <thread>
#include <type_traits>
#include <utility>

#include "knobs.h"

namespace pips {

// ---------------------------------------------------------------------------------------------------------------
// rules that the symbolic retries, the layout and the launches share
// ---------------------------------------------------------------------------------------------------------------
// doubles of the update matrix a front keeps: all r columns, or (border split) those of its rb rows of K
static inline long long mf_unp(const BlockSym& bs, const HeadSupernode& s) {
   const long long uc = bs.mf_split ? s.rb : s.r, r = mf_rows(bs, s);
   return uc * r - uc * (uc - 1) / 2;
}

FrontLds front_lds(const BlockSym& bs, int l) {
   const HeadSupernode& s = bs.sn[l];
   const long long w = s.w, r = mf_rows(bs, s), nf = w + r;
   FrontLds f;
   f.panel = std::max<long long>(w * nf - w * (w - 1) / 2, w * ((r + 3) / 4 * 4));   // packed panel / aligned L21 copy
   f.upd = mf_unp(bs, s);
   f.extra = 0;
   if (l < (int)bs.mf_meta.size() && bs.mf_meta[l] >= 0) {
      const int* H = bs.mf_int.data() + bs.mf_meta[l];
      f.extra = H[5] + (H[6] + H[3] + 1) / 2 + 2;
   }
   return f;
}

int mf_class(const BlockSym& bs, int l, long long lds_budget) {
   const HeadSupernode& s = bs.sn[l];
   const int w = s.w;
   const long long nf = w + mf_rows(bs, s);
   if (!front_lds(bs, l).resident(lds_budget)) return 6 + (nf <= 256 ? 0 : 1);   // update matrix stays in device memory
   // more than one wave: 256 threads - the phases around the pivots are spread over them (128 threads up to 128 rows - twice the fronts
   // per compute unit where the registers set the limit - measured 15.3 against 15.0 ms on the 256-block chain: docs/HISTORY_r4.md)
   return (nf <= 64 ? 0 : 2) + 3 * (w <= 16 ? 0 : 1);
}

bool fronts_fit(const std::vector<BlockSym>& sym, const AnalyzeOptions& opt) {
   for (const BlockSym& bs : sym) {
      if (!bs.mf_ok) return false;
      // fronts with very many leaves below them: the staged leaf data must fit beside the front
      for (int l = 0; l < (int)bs.sn.size(); ++l)
         if (bs.mf_meta[l] >= 0 && front_lds(bs, l).doubles(opt.mf_lds_doubles) > MF_LDS_MAX) return false;
   }
   return true;
}

// The supernodes whose border rows k_border_schur multiplies out - the fronts, and the simple leaves below a front (a leaf without a
// front above it scatters its whole rank-one update itself), ascending - cut into batches of up to BB_GMAX supernodes / stage doubles:
// on_sn(l, nbj, rp, sz) per supernode (border rows, padded to 4, doubles in the border-row arena), on_flush() behind every batch.
template <class OnSn, class OnFlush>
static void walk_bb_batches(const BlockSym& bs, int stage, OnSn&& on_sn, OnFlush&& on_flush) {
   int cnt = 0, nd = 0;
   for (int l = 0; l < (int)bs.sn.size(); ++l) {
      const HeadSupernode& hs = bs.sn[l];
      if (hs.rb >= hs.r || (is_simple(hs) && bs.sn_parent[l] < 0)) continue;
      const int nbj = hs.r - hs.rb, rp = (nbj + 3) & ~3, sz = hs.w * rp + ((hs.w + 1) & ~1);
      if (cnt > 0 && (cnt == BB_GMAX || nd + sz > stage)) { on_flush(); cnt = nd = 0; }
      on_sn(l, nbj, rp, sz);
      ++cnt; nd += sz;
   }
   if (cnt > 0) on_flush();
}

BbPlanSize bb_plan_size(const std::vector<BlockSym>& sym) {
   BbPlanSize z;
   for (const BlockSym& bs : sym) if (bs.mf_split) z.nbmax = std::max(z.nbmax, bs.nb);
   const long long tri = ((long long)z.nbmax * (z.nbmax + 1) / 2 + 1) & ~1LL;
   const long long room = 19200 - tri - 4 * 512 / 2 - 64;   // (positions: up to 4 * 512 ints; supernode records)
   z.stage = (int)std::max<long long>(3072, std::min<long long>(6144, room)) & ~1;
   // two workgroups on a compute unit where half the LDS leaves a staging area of 3072 doubles or more: the walk is a chain of
   // barriers and request latencies per batch, a second workgroup fills them (configs[3] shape, nb = 103: k_border_schur 3.3 -> 2.1 ms
   // with 3072 - 4096 doubles and two workgroups per block; 2048 doubles and two or three: 2.7 - 3.2 ms)
   const long long room2 = 9600 - tri - 4 * 512 / 2 - 64;
   if (room2 >= 3072) { z.stage = (int)std::min<long long>(4096, room2) & ~1; z.two_per_cu = true; }
   for (const BlockSym& bs : sym) {
      if (!bs.mf_split) continue;
      for (const HeadSupernode& hs : bs.sn)
         if (hs.rb < hs.r) {
            const int need = hs.w * ((hs.r - hs.rb + 3) / 4 * 4) + ((hs.w + 1) & ~1);
            if (need > z.stage) { z.stage = need; z.two_per_cu = false; }   // (a supernode beyond the half-LDS area: back to one workgroup's rule)
         }
   }
   if (!z.two_per_cu) z.stage = std::max<int>(z.stage, (int)std::max<long long>(3072, std::min<long long>(6144, room)) & ~1);
   for (const BlockSym& bs : sym) {
      if (!bs.mf_split) continue;
      int np = 0;
      walk_bb_batches(bs, z.stage, [&](int, int nbj, int, int) { np += nbj; }, [&]() { z.poscap = std::max(z.poscap, np); np = 0; });
   }
   return z;
}

size_t bb_lds_bytes(const BbPlanSize& z) {
   const long long ncp = ((long long)z.nbmax * (z.nbmax + 1) / 2 + 1) & ~1LL;
   return (size_t)(ncp + z.stage) * sizeof(double) + (size_t)((z.poscap + 3) & ~3) * sizeof(int) + BB_GMAX * sizeof(BbMeta);
}

bool border_split_must_go(const std::vector<BlockSym>& sym, bool mf) {
   bool any_split = false;
   for (const BlockSym& bs : sym) any_split = any_split || bs.mf_split;
   // ... or k_border_schur's triangle + staged batch + row positions exceed the LDS (nb close to the cap under wide fronts whose
   // below-rows are nearly all border rows): the same formula the launch uses, evaluated here so that such an input is analysed with
   // whole update matrices instead of failing in every factor()
   return any_split && (!mf || !bb_fits(bb_plan_size(sym)));
}

// Schur contribution by the augmented partial factorisation (border rows ride in every panel: dense work, right when
// the factor is dense anyway) or by blocked solves with the plain factor (the reference's way: 4 nnz(L) flops per border
// column, right when L is sparse and L^-1 Br would fill in).  Estimated from the bordered symbolic analysis.
bool blocked_solves_cheaper(const std::vector<BlockSym>& sym, int S, const AnalyzeOptions& opt) {
   double t_aug = 0.0, l_bytes = 0.0;
   int max_levels = 0, max_ntc = 0;
   std::vector<char> used(S, 0);
   for (const BlockSym& s : sym) {
      double pairs = 0.0, border_entries = 0.0;
      for (const HeadSupernode& sn : s.sn) {
         const double rbd = sn.r - sn.rb;
         // every scattered pair costs a w-long dot product besides its atomic (calibrated: 8e-11 s at w = 1, 1e-9 s at w = 25)
         pairs += (rbd * (sn.r - rbd) + 0.5 * rbd * rbd) * std::max(1.0, 0.5 * sn.w);
         border_entries += rbd * sn.w;
      }
      t_aug += opt.head_cost * pairs + s.flops_border / opt.mfma_rate;
      l_bytes += 8.0 * ((double)s.nnzL - border_entries);
      max_levels = std::max(max_levels, s.n_levels);
      max_ntc = std::max(max_ntc, s.m_pad / TILE);
      for (int c : s.bmap) used[c] = 1;
   }
   double ncols = 0;
   for (char u : used) ncols += u;
   const double launches = 2.0 * (max_levels + 2 * max_ntc) + 8;
   // multi-RHS sweeps over a sparse factor run at ~0.8 TB/s effective (measured, tools/banded_schur_probe.py)
   const double t_sol = ncols * 2.0 * l_bytes / 0.8e12 + std::ceil(ncols / 32.0) * launches * 12e-6;
   return t_sol < t_aug;
}

int schur_pack_block(int S, const int* bt_rowptr, int* local_of_row) {
   int nb = 0;
   for (int s = 0; s < S; ++s) local_of_row[s] = (bt_rowptr && bt_rowptr[s + 1] > bt_rowptr[s]) ? nb++ : -1;
   return nb;
}

void build_schur_pack(const std::vector<BlockInput>& in, int S, SchurPack& out) {
   const int nblk = (int)in.size();
   out = SchurPack();
   out.nb.assign(nblk, 0);
   out.off.assign(nblk + 1, 0);
   std::vector<int> local(std::max(S, 1));
   for (int b = 0; b < nblk; ++b) {
      out.nb[b] = schur_pack_block(S, in[b].btrow.empty() ? nullptr : in[b].btrow.data(), local.data());
      for (int s = 0; s < S; ++s)
         if (local[s] >= 0) out.cols.push_back(s);
      out.off[b + 1] = (long long)out.cols.size();
      out.nb_max = std::max(out.nb_max, out.nb[b]);
   }
}

int schur_pack_rows(const std::vector<BlockInput>& in, int S, const std::vector<long long>& off, long long tab_size, PackRows& out) {
   out = PackRows();
   std::vector<int> local(std::max(S, 1));
   for (int b = 0; b < (int)in.size(); ++b) {
      if (in[b].btrow.empty()) continue;   // (the rows of the global border CSR: S per block with a border, layout_border_csr)
      const int nb_b = schur_pack_block(S, in[b].btrow.data(), local.data());
      if (off[b] + (long long)nb_b * nb_b > tab_size)
         PIPS_FAIL(PIPS_ERR_ARG, "set_sc_tables: the position table of block %d is shorter than its %d x %d border columns", b, nb_b, nb_b);
      for (int s = 0; s < S; ++s) {
         out.la.push_back(local[s]);
         out.tabrow.push_back(local[s] >= 0 ? off[b] + (long long)local[s] * nb_b : 0);
      }
   }
   return PIPS_OK;
}

int analyze_blocks(const std::vector<BlockInput>& in, int S, const AnalyzeOptions& opt, int n_threads, bool with_border, std::vector<BlockSym>& sym) {
   const int nblk = (int)in.size();
   sym.assign(nblk, BlockSym());
   std::vector<int> rc(nblk, 0);
   std::vector<std::string> msgs(nblk);
   n_threads = std::max(1, std::min(n_threads, nblk));
   auto work = [&](int t) {
      for (int b = t; b < nblk; b += n_threads) {
         CsrPattern K{in[b].n, in[b].n, in[b].krow.data(), in[b].kcol.data()};
         CsrPattern B{0, in[b].n, nullptr, nullptr};
         if (with_border && !in[b].btrow.empty()) B = CsrPattern{S, in[b].n, in[b].btrow.data(), in[b].btcol.data()};
         rc[b] = analyze_block(K, B, in[b].n_primal, opt, sym[b]);
         if (rc[b]) msgs[b] = last_error();
      }
   };
   std::vector<std::thread> th;
   for (int t = 1; t < n_threads; ++t) th.emplace_back(work, t);
   work(0);
   for (auto& t : th) t.join();
   for (int b = 0; b < nblk; ++b)
      if (rc[b]) PIPS_FAIL(rc[b], "block %d: %s", b, msgs[b].c_str());
   return PIPS_OK;
}

int analyze_symbolic(const std::vector<BlockInput>& in, int S, int n_threads, AnalyzeOptions& opt, LayoutKnobs& knobs, std::vector<BlockSym>& sym) {
   bool any_border = false;
   for (const BlockInput& b : in) any_border = any_border || !b.btrow.empty();
   int rc = analyze_blocks(in, S, opt, n_threads, knobs.schur_mode != 2, sym);
   if (rc) return rc;
   knobs.schur_mode_eff = (knobs.schur_mode == 2 && any_border) ? 2 : 1;
   if (knobs.schur_mode == 0 && any_border && blocked_solves_cheaper(sym, S, opt)) {
      knobs.schur_mode_eff = 2;
      if ((rc = analyze_blocks(in, S, opt, n_threads, false, sym))) return rc;
   }
   // multifrontal head: every block's fronts must fit the LDS; the slot machinery of deterministic mode records scatters
   knobs.mf = knobs.mf_wanted && fronts_fit(sym, opt);
   if (border_split_must_go(sym, knobs.mf)) {   // every block back to full panels
      opt.mf_split_nb_max = 0;
      if ((rc = analyze_blocks(in, S, opt, n_threads, knobs.schur_mode_eff != 2, sym))) return rc;
      if (knobs.mf) knobs.mf = fronts_fit(sym, opt);   // (the fronts grew by their border columns: they must still fit)
   }
   return PIPS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the steps of build_batch_layout
// ---------------------------------------------------------------------------------------------------------------
namespace {

// per-block bases of the concatenated arrays (nblk + 1 each)
struct Bases {
   std::vector<long long> bptr, rows_base, sn_base, bmap_off, upd_base, mfU_base, mfint_base, mfLV_base;
   long long sncol = 0;
};
struct Key { int level, cls, lds, blk, loc; };

// ---- offsets
int layout_offsets(const std::vector<BlockInput>& in, const std::vector<BlockSym>& sym, bool mf, BatchLayout& o, Bases& B) {
   const int nblk = (int)in.size();
   o.h_blks.assign(nblk, BlkDesc());
   o.kptr.assign(nblk + 1, 0);
   o.x_off.assign(nblk + 1, 0);
   for (auto* v : {&B.bptr, &B.rows_base, &B.sn_base, &B.bmap_off, &B.upd_base, &B.mfU_base, &B.mfint_base, &B.mfLV_base}) v->assign(nblk + 1, 0);
   long long arena = 0, xw = 0, winv = 0, dt = 0, sncol = 0, uar = 0;
   for (int b = 0; b < nblk; ++b) {
      const BlockSym& s = sym[b];
      BlkDesc& d = o.h_blks[b];
      d.arena_off = arena;
      d.T = arena + s.T_off;
      d.sncol_off = sncol;
      d.xw_off = xw;
      d.x_off = o.x_off[b];
      d.bmap_off = B.bmap_off[b];
      d.winv_off = winv;
      d.dt_off = dt;
      d.n = s.n; d.n_head = s.n_head; d.m = s.m; d.m_pad = s.m_pad; d.nb = s.nb; d.nb_pad = s.nb_pad; d.ldT = s.ldT;
      d.ntc = s.m_pad / TILE;
      d.ntr = s.m > 0 ? s.ldT / TILE : 0;
      d.mf_split = (mf && s.mf_split) ? (s.mf_konly ? 2 : 1) : 0;   // 2: fronts on the rows of K only (k_border_rows forms their border rows)
      d.U = uar;
      uar += (long long)s.m_pad * s.m_pad;
      d.thr_rel = 0; d.repl_rel = 1e-8; d.repl_abs = 1;
      arena += s.arena;
      xw += s.n_head + s.m_pad + s.nb_pad;   // [head | padded tail | border rows (border-backward sweep only)]
      winv += (long long)d.ntc * TILE * TILE;
      dt += s.m_pad;
      sncol += s.n_head;
      o.kptr[b + 1] = o.kptr[b] + (long long)in[b].kcol.size();
      B.bptr[b + 1] = B.bptr[b] + (long long)in[b].btcol.size();
      o.x_off[b + 1] = o.x_off[b] + s.n;
      B.rows_base[b + 1] = B.rows_base[b] + (long long)s.rowidx.size();
      B.upd_base[b + 1] = B.upd_base[b] + (long long)s.upd.size();
      B.mfU_base[b + 1] = B.mfU_base[b] + (mf ? s.mf_U_total : 0);
      B.mfint_base[b + 1] = B.mfint_base[b] + (mf ? (long long)s.mf_int.size() : 0);
      B.mfLV_base[b + 1] = B.mfLV_base[b] + (mf ? s.mf_LV_total : 0);
      d.lv_off = B.mfLV_base[b];
      d.k_off = o.kptr[b]; d.b_off = B.bptr[b];
      B.sn_base[b + 1] = B.sn_base[b] + (long long)s.sn.size();
      B.bmap_off[b + 1] = B.bmap_off[b] + s.nb;
   }
   B.sncol = sncol;
   o.arena_total = arena; o.uarena_total = uar; o.xw_total = xw; o.winv_total = winv; o.dtail_total = dt;
   o.n_total = o.x_off[nblk]; o.nnzK_total = o.kptr[nblk]; o.nnzB_total = B.bptr[nblk];
   o.mfU_total = B.mfU_base[nblk]; o.mfLV_total = B.mfLV_base[nblk];
   // the concatenated CSR copies of K (refinement residual: both triangles) and of the borders are indexed with int32
   if (2 * o.nnzK_total > (long long)INT32_MAX || o.nnzB_total > (long long)INT32_MAX || o.n_total > (long long)INT32_MAX)
      PIPS_FAIL(PIPS_ERR_ARG, "batch too large for the 32-bit index arrays of one rank: sum nnz(K) %lld (limit 2^30), sum nnz(border) %lld, sum n %lld - "
                              "use more ranks or fewer blocks per batch", o.nnzK_total, o.nnzB_total, o.n_total);
   o.nsn_total = (int)B.sn_base[nblk];
   return PIPS_OK;
}

// ---- supernodes sorted by (level, size class); multifrontal head: by (level, kernel variant, LDS need)
std::vector<Key> layout_sort_keys(const std::vector<BlockSym>& sym, bool mf, long long lds_budget, int nsn_total, int& nlev) {
   const int nblk = (int)sym.size();
   std::vector<Key> keys;
   keys.reserve(nsn_total);
   nlev = 0;
   // multifrontal: a level with few fronts is latency, not throughput - all its (LDS-resident) fronts go into ONE launch of the
   // largest variant any of them needs instead of one launch per variant
   constexpr int MF_MERGE_MAX = 1024;
   std::vector<int> lev_cnt, lev_b, lev_w;
   if (mf)
      for (int b = 0; b < nblk; ++b)
         for (int l = 0; l < (int)sym[b].sn.size(); ++l) {
            const HeadSupernode& s = sym[b].sn[l];
            if (is_simple(s)) continue;
            if ((int)lev_cnt.size() <= s.level) { lev_cnt.resize(s.level + 1, 0); lev_b.resize(s.level + 1, 0); lev_w.resize(s.level + 1, 0); }
            const int c = mf_class(sym[b], l, lds_budget);
            ++lev_cnt[s.level];
            if (c < 6) { lev_b[s.level] = std::max(lev_b[s.level], c % 3); lev_w[s.level] = std::max(lev_w[s.level], c / 3); }
         }
   for (int b = 0; b < nblk; ++b)
      for (int l = 0; l < (int)sym[b].sn.size(); ++l) {
         const HeadSupernode& s = sym[b].sn[l];
         // class 0: "simple leaf" (w = 1, r <= 16, level 0) -> one thread each;
         // class 1: small (one wave); class 2: large (256 threads)
         int cls = (s.w <= 8 && s.r <= 64) ? 1 : 2, lds = 0;
         if (mf && !is_simple(s)) {
            int c = mf_class(sym[b], l, lds_budget);
            if (c < 6 && lev_cnt[s.level] <= MF_MERGE_MAX) c = lev_b[s.level] + 3 * lev_w[s.level];
            cls = 1 + c;
            lds = (int)front_lds(sym[b], l).doubles(lds_budget);
         }
         if (is_simple(s)) cls = 0;
         keys.push_back({s.level, cls, lds, b, l});
         nlev = std::max(nlev, s.level + 1);
      }
   std::stable_sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
      return a.level != b.level ? a.level < b.level : (a.cls != b.cls ? a.cls < b.cls : a.lds < b.lds);
   });
   return keys;
}

// ---- spine: the top levels that hold at most two supernodes of every block (chain-like trees of time-coupled
//      blocks).  One launch per level would be pure latency there; they go to the per-block spine kernels instead.
int layout_spine_cut(const std::vector<BlockSym>& sym, int nlev, const LayoutKnobs& knobs) {
   int lstar = nlev;
   std::vector<int> width(nlev, 0);   // max over blocks of the supernode count per level
   std::vector<int> cnt(nlev);
   for (const BlockSym& bs : sym) {
      std::fill(cnt.begin(), cnt.end(), 0);
      for (const HeadSupernode& s : bs.sn) ++cnt[s.level];
      for (int l = 0; l < nlev; ++l) width[l] = std::max(width[l], cnt[l]);
   }
   while (lstar > 0 && width[lstar - 1] <= 2) --lstar;
   if (nlev - lstar < 8 || knobs.spine == 0 || knobs.deterministic || knobs.mf) lstar = nlev;   // the spine kernels hand over through atomics
   return lstar;
}

// ---- supernode records in sorted order, level ranges and front launches; roots_of: fronts without a head parent, ascending
void layout_supernodes(const std::vector<BlockSym>& sym, const std::vector<Key>& keys, int nlev, int lstar, const Bases& B, BatchLayout& o,
                       std::vector<std::vector<int>>& sorted_id, std::vector<std::vector<int>>& roots_of) {
   const int nblk = (int)sym.size();
   const bool mf = o.mf;
   o.h_sns.assign(o.nsn_total, SnDesc());
   roots_of.assign(nblk, {});
   long long slots_acc = 0, vslots_acc = 0;
   sorted_id.assign(nblk, {});
   for (int b = 0; b < nblk; ++b) sorted_id[b].resize(sym[b].sn.size());
   o.levels.assign(lstar, LevelRange{0, 0, 0, 0, 0, 0, 0, 0});
   o.levels_top.assign(nlev - lstar, LevelRange{0, 0, 0, 0, 0, 0, 0, 0});
   o.head_wcap = 1;
   for (int i = 0; i < o.nsn_total; ++i) {
      const Key& k = keys[i];
      const HeadSupernode& s = sym[k.blk].sn[k.loc];
      o.head_wcap = std::max(o.head_wcap, s.w);
      o.h_sns[i] = SnDesc{o.h_blks[k.blk].arena_off + s.panel, B.rows_base[k.blk] + s.rows, B.upd_base[k.blk] + s.upd, s.w, s.r, s.c0, k.blk,
                          s.n_useg, s.rb, s.ld, 0, slots_acc, vslots_acc, -1, -1, -1};
      if (mf && k.cls > 0 && s.r > 0 && sym[k.blk].sn_parent[k.loc] < 0) roots_of[k.blk].push_back(i);
      if (mf) {
         const BlockSym& bs = sym[k.blk];
         if (bs.mf_U[k.loc] >= 0) o.h_sns[i].U = (k.cls == 0 ? B.mfLV_base[k.blk] : B.mfU_base[k.blk]) + bs.mf_U[k.loc];
         if (bs.mf_meta[k.loc] >= 0) o.h_sns[i].mf = B.mfint_base[k.blk] + bs.mf_meta[k.loc];
      }
      // factorisation slots: every scattering supernode; multifrontal head: only the simple leaves without a front above them scatter
      // (the fronts hand their update matrices on, k_root_assemble adds the last ones in a fixed order)
      if (!mf || (k.cls == 0 && s.n_useg == 0)) slots_acc += (long long)s.r * (s.r + 1) / 2;
      vslots_acc += s.r;
      sorted_id[k.blk][k.loc] = i;
      LevelRange& L = k.level >= lstar ? o.levels_top[k.level - lstar] : o.levels[k.level];
      if (k.cls == 0) { if (L.simple_cnt++ == 0) L.simple_begin = i; }
      else if (k.cls == 1 || mf) { if (L.small_cnt++ == 0) L.small_begin = i; }   // multifrontal: one contiguous range of fronts per level
      else { if (L.large_cnt++ == 0) L.large_begin = i; }
      if (mf && k.cls > 0) {
         // one launch per (level, variant, LDS bucket): the dynamic LDS of a launch is that of its largest front, and it decides how
         // many fronts share a compute unit
         std::vector<MfLaunch>& mf_launches = o.mf_launches;
         bool open = mf_launches.empty() || mf_launches.back().level != k.level || mf_launches.back().cls != k.cls - 1;
         if (!open) {
            const MfLaunch& m = mf_launches.back();
            const int first_lds = keys[m.begin].lds;
            {
               // how many fronts of the variant share a compute unit: the LDS decides up to the limit the registers set (123 VGPRs: four
               // waves per SIMD - four workgroups of 256 threads, sixteen of 64); a bucket = one such class, since inside a class a
               // smaller front gains nothing from a launch of its own and across a boundary every front of the launch loses a slot
               auto cls_of = [&](int lds_doubles) {
                  const int c = k.cls - 1, kmax = c == 0 ? 16 : c == 3 ? 12 : c == 1 ? 8 : c == 4 ? 6 : c == 2 ? 4 : 3;   // (154 VGPRs for the 32-wide variants)
                  return std::min(kmax, (int)(163840 / ((long long)lds_doubles * 8 + 1024)));
               };
               if (m.cnt >= 256 && cls_of(k.lds) < cls_of(first_lds)) open = true;
            }
         }
         if (open) mf_launches.push_back({k.level, k.cls - 1, i, 0, 0});
         ++mf_launches.back().cnt;
         mf_launches.back().lds_doubles = std::max(mf_launches.back().lds_doubles, k.lds);
      }
      const long long need = (long long)s.r * (s.w | 1);
      if (k.cls == 1) L.small_lds = (int)std::max<long long>(L.small_lds, std::min<long long>(need, 640));
      else if (k.cls == 2) L.large_lds = (int)std::max<long long>(L.large_lds, std::min<long long>(need, 6144));
   }
   o.slots_total = slots_acc; o.vslots_total = vslots_acc;
}

// ---- multifrontal head: root fronts per block, and the border-split batches.  Their border rows live a second time in the
//      border-row arena (per supernode w x rp doubles + w pivots, padded to even), cut into batches of up to BB_GMAX supernodes /
//      bb_stage doubles that the kernel stages as one contiguous piece
void layout_roots_and_batches(const std::vector<BlockSym>& sym, const std::vector<std::vector<int>>& sorted_id,
                              const std::vector<std::vector<int>>& roots_of, BatchLayout& o) {
   const int nblk = (int)sym.size();
   o.h_root_off.assign(nblk + 1, 0);
   for (int b = 0; b < nblk; ++b) {
      o.h_roots.insert(o.h_roots.end(), roots_of[b].begin(), roots_of[b].end());
      o.h_root_off[b + 1] = (int)o.h_roots.size();
   }
   o.n_roots = (int)o.h_roots.size();
   o.h_bb_off.assign(nblk + 1, 0);
   o.bb_stage = 3072; o.bb_nbmax = 0; o.bb_poscap = 0;
   // staging area: as much of the LDS as the packed triangle of the widest border leaves (a batch is one barrier pair and one request
   // latency whatever it holds; the supernodes of the upper levels take 2000+ doubles each), at most 6144 doubles, at least the largest
   // single supernode (bb_plan_size)
   { const BbPlanSize z = bb_plan_size(sym); o.bb_stage = z.stage; o.bb_two_per_cu = z.two_per_cu; }
   long long bb_total = o.arena_total;   // the border-row arena lives behind the panels in the same allocation (offsets like SnDesc::panel)
   for (int b = 0; b < nblk; ++b) {
      const BlockSym& bs = sym[b];
      if (bs.mf_split) {
         o.bb_nbmax = std::max(o.bb_nbmax, bs.nb);
         BbBatch cur{0, 0, 0, 0, 0, 0, 0, 0};
         walk_bb_batches(
            bs, o.bb_stage,
            [&](int l, int nbj, int rp, int sz) {
               const HeadSupernode& hs = bs.sn[l];
               if (cur.cnt == 0) { cur.src = bb_total; cur.pos = (long long)o.h_bb_pos.size(); cur.first = (int)o.h_bb_meta.size(); }
               o.h_bb_meta.push_back(BbMeta{cur.ndoubles, cur.npos, hs.w, nbj, cur.ntiles, 0, 0, 0});
               o.h_sns[sorted_id[b][l]].bb = bb_total;
               for (int a = hs.rb; a < hs.r; ++a) o.h_bb_pos.push_back(bs.rowidx[hs.rows + a] - bs.n);
               ++cur.cnt; cur.ndoubles += sz; cur.ntiles += bb_tile_count(rp); cur.npos += nbj;
               bb_total += sz;
            },
            [&]() { o.h_bb_batches.push_back(cur); o.bb_poscap = std::max(o.bb_poscap, cur.npos); cur = BbBatch{0, 0, 0, 0, 0, 0, 0, 0}; });
      }
      o.h_bb_off[b + 1] = (int)o.h_bb_batches.size();
   }
   o.n_bb = (int)o.h_bb_batches.size();
   o.bb_doubles = bb_total - o.arena_total;
}

// ---- gather-form metadata of the blocks whose fronts hold the rows of K only
int layout_konly(const std::vector<BlockSym>& sym, const std::vector<std::vector<int>>& sorted_id, BatchLayout& o) {
   const int nblk = (int)sym.size();
   std::vector<int>&h_rec = o.h_kb_rec, &h_list = o.h_kb_list, &h_tail = o.h_kb_tail;
   o.h_kb_off.assign((size_t)std::max(o.nsn_total, 1), -1);
   std::vector<std::vector<int>> by_level(o.levels.size());
   o.kb_level_pairs.assign(o.levels.size(), 0); o.kb_level_lds.assign(o.levels.size(), 0);
   bool any = false;
   for (int b = 0; b < nblk && o.mf; ++b) {
      const BlockSym& bs = sym[b];
      if (!bs.mf_konly) continue;
      any = true;
      for (int l = 0; l < (int)bs.sn.size(); ++l) {
         if (bs.kb_off[l] < 0) continue;
         const int* R = bs.kb_rec.data() + bs.kb_off[l];
         const int np = R[0], ne = R[1];
         o.h_kb_off[sorted_id[b][l]] = (long long)h_rec.size();
         h_rec.push_back(np); h_rec.push_back(ne);
         for (int q = 0; q < np; ++q) { h_rec.push_back(sorted_id[b][R[2 + 2 * q]]); h_rec.push_back(R[3 + 2 * q]); }
         h_rec.insert(h_rec.end(), R + 2 + 2 * np, R + 2 + 2 * np + 2 * ne);
         const HeadSupernode& sj = bs.sn[l];
         if (sj.level >= (int)by_level.size()) PIPS_FAIL(PIPS_ERR_STATE, "analyze: internal error, level of a front with border rows");
         by_level[sj.level].push_back(sorted_id[b][l]);
         o.kb_level_pairs[sj.level] = std::max(o.kb_level_pairs[sj.level], np);
         o.kb_level_lds[sj.level] = std::max(o.kb_level_lds[sj.level], (int)(sj.w * ((sj.r - sj.rb + 3) / 4 * 4) * sizeof(double)));
      }
      for (size_t q = 0; q + 1 < bs.kb_tail.size(); q += 2) { h_tail.push_back(sorted_id[b][bs.kb_tail[q]]); h_tail.push_back(bs.kb_tail[q + 1]); }
   }
   o.kb_level_off.assign(o.levels.size() + 1, 0);
   for (size_t l = 0; l < by_level.size(); ++l) { h_list.insert(h_list.end(), by_level[l].begin(), by_level[l].end()); o.kb_level_off[l + 1] = (int)h_list.size(); }
   o.n_kb_tail = (int)(h_tail.size() / 2);
   o.kb_any = any;
   if (any) {
      if (h_rec.empty()) h_rec.push_back(0);
      if (h_list.empty()) h_list.push_back(0);
      if (h_tail.empty()) h_tail.push_back(0);
   }
   return PIPS_OK;
}

// ---- spine lists: per block, ascending local index = postorder (children before parents)
void layout_spine_lists(const std::vector<BlockSym>& sym, const std::vector<std::vector<int>>& sorted_id, int lstar, BatchLayout& o) {
   const int nblk = (int)sym.size();
   o.h_spine_off.assign(nblk + 1, 0);
   for (int b = 0; b < nblk; ++b) {
      for (int l = 0; l < (int)sym[b].sn.size(); ++l)
         if (sym[b].sn[l].level >= lstar) o.h_spine.push_back(sorted_id[b][l]);
      o.h_spine_off[b + 1] = (int)o.h_spine.size();
   }
   o.spine_total = (int)o.h_spine.size();
}

// ---- the tails as one launch (tailkernel.hip.h; the default for batches of up to 16 blocks, slower than the column launches for the
// large ones: DESIGN.md 4.2a): multifrontal head (every producer of the tail panel goes by BlkDesc::T_in), no deterministic mode (its slot records hold
// panel addresses), room for a second copy of the tail panels
void layout_tail_single(const std::vector<BlockSym>& sym, const LayoutKnobs& knobs, BatchLayout& o) {
   const int nblk = (int)sym.size();
   long long scratch = 0;
   for (int b = 0; b < nblk; ++b) scratch += sym[b].arena - sym[b].T_off;
   const double need = 8.0 * (double)(o.arena_total + o.bb_doubles + scratch + o.uarena_total) + 4e9;
   // few blocks: the column launches are a chain of ~4 launches per tile column whatever the batch holds, and the one launch wins
   // (leaf factorisation of configs[1] blocks, profiles/r6_tail_single_by_blocks.txt: 1 block 8.41 -> 7.48 ms, 4: 13.2 -> 12.1,
   // 8: 19.3 -> 17.8, 16: 31.1 -> 30.4; from 24 blocks on it loses: 43.0 -> 43.7, 32: 54.2 -> 56.4, 64: 101 -> 110).
   const int want_single = knobs.tail_single >= 0 ? knobs.tail_single : (nblk <= 16 ? 1 : 0);
   o.tail_single = o.mf && !knobs.deterministic && scratch > 0 && want_single != 0 && need < (double)(size_t)knobs.free_device_bytes;
   o.tail_scratch = o.tail_single ? scratch : 0;
   long long at = o.arena_total + o.bb_doubles;
   for (int b = 0; b < nblk; ++b) {
      o.h_blks[b].T_in = o.tail_single ? at : o.h_blks[b].T;
      at += sym[b].arena - sym[b].T_off;
   }
}

// ---- concatenated index arrays
int layout_index_arrays(const std::vector<BlockInput>& in, const std::vector<BlockSym>& sym, const std::vector<std::vector<int>>& sorted_id,
                        const Bases& B, BatchLayout& o) {
   const int nblk = (int)in.size();
   const bool mf = o.mf;
   const std::vector<long long>&kptr = o.kptr, &x_off = o.x_off;
   o.h_upd.reserve(B.upd_base[nblk]);
   o.h_psign_off.assign(nblk, 0); o.h_perm_off.assign(nblk, 0);
   o.h_kdst.assign(o.nnzK_total, 0); o.h_bdst.assign(o.nnzB_total, 0); o.h_kdiag.assign(o.n_total, 0); o.h_rowbase.assign(o.n_total, 0);
   o.h_krowptr.assign(o.n_total + 1, 0); o.h_kcolidx.assign(o.nnzK_total, 0);
   o.h_rowidx.reserve(B.rows_base[nblk]);
   o.h_sncol.reserve(B.sncol);
   for (int b = 0; b < nblk; ++b) {
      const BlockSym& s = sym[b];
      o.h_rowidx.insert(o.h_rowidx.end(), s.rowidx.begin(), s.rowidx.end());
      o.h_upd.insert(o.h_upd.end(), s.upd.begin(), s.upd.end());
      for (int c = 0; c < s.n_head; ++c) o.h_sncol.push_back(sorted_id[b][s.sn_of_col[c]]);
      o.h_bmap.insert(o.h_bmap.end(), s.bmap.begin(), s.bmap.end());
      o.h_psign_off[b] = (long long)o.h_psign.size();
      o.h_psign.insert(o.h_psign.end(), s.psign.begin(), s.psign.end());
      o.h_perm_off[b] = (long long)o.h_perm.size();
      o.h_perm.insert(o.h_perm.end(), s.perm.begin(), s.perm.end());
      // multifrontal head: the fronts read their panel entries from the value arrays (k_front), nobody reads them from the arena
      // (entries of the tail panel land where the tail is assembled: BlkDesc::T_in)
      auto dst = [&](long long rel) { return rel >= s.T_off ? o.h_blks[b].T_in + (rel - s.T_off) : o.h_blks[b].arena_off + rel; };
      for (size_t p = 0; p < s.a_dst.size(); ++p) o.h_kdst[kptr[b] + p] = (mf && s.a_front[p]) ? -1 : dst(s.a_dst[p]);
      for (size_t p = 0; p < s.b_dst.size(); ++p) o.h_bdst[B.bptr[b] + p] = (mf && s.b_front[p]) ? -1 : dst(s.b_dst[p]);
      for (int i = 0; i < s.n; ++i) {
         long long dp = -1;
         for (int p = in[b].krow[i]; p < in[b].krow[i + 1]; ++p)
            if (in[b].kcol[p] == i) dp = kptr[b] + p;
         if (dp < 0) PIPS_FAIL(PIPS_ERR_ARG, "block %d row %d has no explicit diagonal entry (create_kkt always stores one)", b, i);
         o.h_kdiag[x_off[b] + i] = dp;
         o.h_rowbase[x_off[b] + i] = x_off[b];
         o.h_krowptr[x_off[b] + i] = (int)(kptr[b] + in[b].krow[i]);
      }
      std::copy(in[b].kcol.begin(), in[b].kcol.end(), o.h_kcolidx.begin() + kptr[b]);
   }
   o.h_krowptr[o.n_total] = (int)o.nnzK_total;
   if (mf) {
      o.h_mfint.assign((size_t)B.mfint_base[nblk], 0);
      for (int b = 0; b < nblk; ++b) {
         const BlockSym& s = sym[b];
         std::copy(s.mf_int.begin(), s.mf_int.end(), o.h_mfint.begin() + B.mfint_base[b]);
         for (int64_t pos : s.mf_fix) o.h_mfint[(size_t)(B.mfint_base[b] + pos)] = sorted_id[b][s.mf_int[(size_t)pos]];
      }
   }
   o.h_nprimal.resize(nblk);
   for (int b = 0; b < nblk; ++b) o.h_nprimal[b] = in[b].n_primal;
   o.tile_first.resize(nblk);
   for (int b = 0; b < nblk; ++b) o.tile_first[b] = &sym[b].tile_first;
   return PIPS_OK;
}

// ---- first-touch plan of the tails (layout.h): decided per batch.  It needs the multifrontal head (fronts hand their update matrices on,
// only the root fronts' reach the tail; no spine kernels) without deterministic mode (its slot records hold tail addresses and its sums
// keep today's order bit for bit), so that before the tail factorisation nothing but k_scatter, k_tail_pad_diag, the simple leaves and
// k_root_assemble writes the tails; and the tallest column has to fit the LDS budget.  Takes the tail targets out of h_kdst / h_bdst.
int layout_first_touch(const std::vector<BlockSym>& sym, const Bases& B, const LayoutKnobs& knobs, BatchLayout& o) {
   const int nblk = (int)sym.size();
   o.tail_first_touch = false;
   o.ft_ld_max = 0; o.ft_cols_max = 0;
   for (const BlkDesc& bd : o.h_blks) { o.ft_ld_max = std::max(o.ft_ld_max, bd.ldT); o.ft_cols_max = std::max(o.ft_cols_max, bd.m_pad); }
   if (knobs.tail_first_touch == 0 || !o.mf || knobs.deterministic || o.spine_total > 0 || o.ft_cols_max == 0 || o.levels.empty() ||
       8LL * o.ft_ld_max > std::min(knobs.ft_lds_bytes, FT_LDS_MAX) || o.nnzK_total >= INT_MAX || o.nnzB_total >= INT_MAX)
      return PIPS_OK;
   // the kernel zeroes and writes a column in pairs of doubles (16-byte LDS and device accesses, like k_arena_clear): every column starts
   // at an even offset and holds an even number of rows (ldT is a multiple of the tile, T_in of the panels' padding of 16)
   for (const BlkDesc& bd : o.h_blks)
      if ((bd.ldT & 1) || (bd.T_in & 1)) return PIPS_OK;
   o.h_ft_colbase.assign(nblk + 1, 0);
   for (int b = 0; b < nblk; ++b) o.h_ft_colbase[b + 1] = o.h_ft_colbase[b] + o.h_blks[b].m_pad;
   if (o.h_ft_colbase[nblk] >= INT_MAX) return PIPS_OK;
   const size_t ncols = (size_t)o.h_ft_colbase[nblk];
   struct Init { int col, row, src; };
   struct Piece { int col; FtPiece p; };
   std::vector<Init> ini;
   std::vector<Piece> pcs;
   for (int b = 0; b < nblk; ++b) {
      const BlockSym& s = sym[b];
      const BlkDesc& bd = o.h_blks[b];
      const int cb = (int)o.h_ft_colbase[b];
      auto take = [&](const std::vector<int64_t>& dst, std::vector<long long>& out, long long base, bool border) -> int {
         for (size_t p = 0; p < dst.size(); ++p) {
            if (out[(size_t)base + p] < 0 || dst[p] < s.T_off) continue;
            const long long rel = dst[p] - s.T_off;
            const int c = (int)(rel / bd.ldT), row = (int)(rel % bd.ldT);
            if (c >= bd.m_pad || row < c / TILE * TILE) PIPS_FAIL(PIPS_ERR_STATE, "analyze: internal error, entry %zu of block %d lands above the diagonal tile of tail column %d", p, b, c);
            ini.push_back(Init{cb + c, row, border ? ~(int)(base + (long long)p) : (int)(base + (long long)p)});
            out[(size_t)base + p] = -1;
         }
         return PIPS_OK;
      };
      if (int rc = take(s.a_dst, o.h_kdst, o.kptr[b], false)) return rc;
      if (o.schur_mode_eff == 1)   // (Schur mode 2 scatters no border)
         if (int rc = take(s.b_dst, o.h_bdst, B.bptr[b], true)) return rc;
      for (int q = o.h_root_off[b]; q < o.h_root_off[b + 1]; ++q) {
         const SnDesc& sn = o.h_sns[o.h_roots[q]];
         const int r = bd.mf_split == 2 ? sn.rb : sn.r;   // (fronts on the rows of K only hand over a K x K update matrix)
         const int* rows = o.h_rowidx.data() + sn.rows;
         for (int a = 0; a < r; ++a) {   // rows ascend; the first lies in the tail or the border, the last inside the column's LDS
            const int tr = rows[a] < bd.n ? rows[a] - bd.n_head : bd.m_pad + (rows[a] - bd.n);
            if (rows[a] < bd.n_head || tr >= bd.ldT || (a > 0 && rows[a] <= rows[a - 1]))
               PIPS_FAIL(PIPS_ERR_STATE, "analyze: internal error, row %d of root front %d of block %d", a, o.h_roots[q], b);
         }
         for (int bcol = 0; bcol < std::min(sn.rb, r); ++bcol)
            pcs.push_back(Piece{cb + rows[bcol] - bd.n_head,
                                FtPiece{sn.U + (long long)bcol * r - (long long)bcol * (bcol - 1) / 2, sn.rows + bcol, r - bcol, o.h_roots[q]}});
      }
   }
   // by column, in the order met (K before border; fronts ascending): counting sort
   o.h_ft_init_off.assign(ncols + 1, 0); o.h_ft_piece_off.assign(ncols + 1, 0);
   for (const Init& e : ini) ++o.h_ft_init_off[(size_t)e.col + 1];
   for (const Piece& e : pcs) ++o.h_ft_piece_off[(size_t)e.col + 1];
   for (size_t g = 0; g < ncols; ++g) { o.h_ft_init_off[g + 1] += o.h_ft_init_off[g]; o.h_ft_piece_off[g + 1] += o.h_ft_piece_off[g]; }
   o.h_ft_init.assign(ini.size(), FtInit{0, 0}); o.h_ft_piece.assign(pcs.size(), FtPiece{0, 0, 0, 0});
   {
      std::vector<int> fi(o.h_ft_init_off.begin(), o.h_ft_init_off.end() - 1), fp(o.h_ft_piece_off.begin(), o.h_ft_piece_off.end() - 1);
      for (const Init& e : ini) o.h_ft_init[(size_t)fi[(size_t)e.col]++] = FtInit{e.row, e.src};
      for (const Piece& e : pcs) o.h_ft_piece[(size_t)fp[(size_t)e.col]++] = e.p;
   }
   const LevelRange& L0 = o.levels[0];
   for (int i = L0.simple_begin; i < L0.simple_begin + L0.simple_cnt; ++i)
      if (o.h_sns[i].n_useg == 0 && o.h_sns[i].r > 0) o.h_ft_leaves.push_back(i);
   o.n_ft_leaves = (int)o.h_ft_leaves.size();
   o.tail_first_touch = true;
   return PIPS_OK;
}

// ---- both triangles, row by row: entry (i, j) of the lower CSR also appears in row j as (j, i)
void layout_full_rows(const std::vector<BlockInput>& in, const std::vector<BlockSym>& sym, BatchLayout& o) {
   const int nblk = (int)in.size();
   const std::vector<long long>&kptr = o.kptr, &x_off = o.x_off;
   std::vector<int>& frp = o.h_frowptr;
   frp.assign(o.n_total + 1, 0);
   for (int b = 0; b < nblk; ++b)
      for (int i = 0; i < sym[b].n; ++i)
         for (int p = in[b].krow[i]; p < in[b].krow[i + 1]; ++p) {
            const int j = in[b].kcol[p];
            ++frp[x_off[b] + i + 1];
            if (j != i) ++frp[x_off[b] + j + 1];
         }
   for (long long r = 0; r < o.n_total; ++r) frp[r + 1] += frp[r];
   std::vector<int>&fcol = o.h_fcol, &fsrc = o.h_fsrc;
   fcol.assign(frp[o.n_total], 0); fsrc.assign(frp[o.n_total], 0);
   std::vector<int> fill(frp.begin(), frp.end() - 1);
   for (int b = 0; b < nblk; ++b)
      for (int i = 0; i < sym[b].n; ++i)
         for (int p = in[b].krow[i]; p < in[b].krow[i + 1]; ++p) {
            const int j = in[b].kcol[p], src = (int)(kptr[b] + p);
            int q = fill[x_off[b] + i]++;
            fcol[q] = j; fsrc[q] = src;
            if (j != i) { q = fill[x_off[b] + j]++; fcol[q] = i; fsrc[q] = src; }
         }
   for (long long r = 0; r < o.n_total; ++r)
      if (frp[r + 1] - frp[r] > FULL_LONG_ROW) o.h_flong.push_back(r);
   o.n_flong = (int)o.h_flong.size();
}

// ---- border CSR, global: by (block, Schur column), the non-empty Schur columns, and the border by LEAF row (t += alpha Br x0 as a
//      gather, k_border_mult_rows): row pointers over the flat leaf space, Schur column and position in the value array of every entry
void layout_border_csr(const std::vector<BlockInput>& in, int S, const Bases& B, BatchLayout& o) {
   const int nblk = (int)in.size();
   std::vector<int>&h_bt_rowptr = o.h_bt_rowptr, &h_bt_colidx = o.h_bt_colidx, &h_bt_rowsc = o.h_bt_rowsc;
   std::vector<long long>& h_bt_xoff = o.h_bt_xoff;
   h_bt_colidx.assign(o.nnzB_total, 0);
   o.h_bval.assign(o.nnzB_total, 0.0);
   h_bt_rowptr.push_back(0);
   for (int b = 0; b < nblk; ++b) {
      if (in[b].btrow.empty()) continue;
      for (int s2 = 0; s2 < S; ++s2) {
         h_bt_rowptr.push_back((int)(B.bptr[b] + in[b].btrow[s2 + 1]));
         h_bt_rowsc.push_back(s2);
         h_bt_xoff.push_back(o.x_off[b]);
      }
      std::copy(in[b].btcol.begin(), in[b].btcol.end(), h_bt_colidx.begin() + B.bptr[b]);
      std::copy(in[b].btval.begin(), in[b].btval.end(), o.h_bval.begin() + B.bptr[b]);
   }
   o.bt_rows_total = (long long)h_bt_rowsc.size();
   o.h_bt_rownnz.assign((size_t)o.bt_rows_total, 0);
   for (long long i = 0; i < o.bt_rows_total; ++i) o.h_bt_rownnz[(size_t)i] = h_bt_rowptr[i + 1] - h_bt_rowptr[i];
   for (int b = 0; b < nblk; ++b)
      if (!in[b].btrow.empty()) o.h_bt_rowblk.insert(o.h_bt_rowblk.end(), (size_t)S, b);
   {  // non-empty Schur columns over all blocks (the reference skips empty border columns, :870-874)
      std::vector<char> used(std::max(S, 1), 0);
      for (int b = 0; b < nblk; ++b)
         if (!in[b].btrow.empty())
            for (int s2 = 0; s2 < S; ++s2)
               if (in[b].btrow[s2 + 1] > in[b].btrow[s2]) used[s2] = 1;
      o.h_schur_slot.assign(std::max(S, 1), -1);
      for (int s2 = 0; s2 < S; ++s2)
         if (used[s2]) { o.h_schur_slot[s2] = (int)o.schur_cols.size(); o.schur_cols.push_back(s2); }
   }
   if (o.bt_rows_total > 0 && o.nnzB_total > 0 && o.nnzB_total < (1LL << 31)) {
      std::vector<int>&rp = o.h_br_rowptr, &sc = o.h_br_sc, &src = o.h_br_src;
      rp.assign((size_t)o.n_total + 1, 0);
      for (long long r = 0; r < o.bt_rows_total; ++r)
         for (int p = h_bt_rowptr[r]; p < h_bt_rowptr[r + 1]; ++p) ++rp[h_bt_xoff[r] + h_bt_colidx[p] + 1];
      for (long long i = 0; i < o.n_total; ++i) rp[i + 1] += rp[i];
      sc.assign((size_t)o.nnzB_total, 0); src.assign((size_t)o.nnzB_total, 0);
      std::vector<int> fill(rp.begin(), rp.end() - 1);
      for (long long r = 0; r < o.bt_rows_total; ++r)   // ascending (block, Schur column): the order of every row's sum
         for (int p = h_bt_rowptr[r]; p < h_bt_rowptr[r + 1]; ++p) {
            const int q = fill[h_bt_xoff[r] + h_bt_colidx[p]]++;
            sc[q] = h_bt_rowsc[r]; src[q] = p;
         }
   }
}

// ---- simple leaves that own border rows (sweeps of the augmented factor: k_leaf_border), the widest padded border, and the simple
//      leaves' L entries by target row (forward substitution as a gather, k_leaf_fwd_gather)
void layout_leaf_gather(BatchLayout& o) {
   const std::vector<SnDesc>& h_sns = o.h_sns;
   const std::vector<BlkDesc>& h_blks = o.h_blks;
   const std::vector<int>& h_rowidx = o.h_rowidx;
   const long long xw_total = o.xw_total;
   if (!o.levels.empty())
      for (int i = o.levels[0].simple_begin; i < o.levels[0].simple_begin + o.levels[0].simple_cnt; ++i)
         if (h_sns[i].rb < h_sns[i].r) o.h_lb_list.push_back(i);
   o.n_lb = (int)o.h_lb_list.size();
   o.nb_pad_max = 0;
   for (const BlkDesc& bd : h_blks) o.nb_pad_max = std::max(o.nb_pad_max, bd.nb_pad);
   const LevelRange* L0 = o.levels.empty() ? nullptr : &o.levels[0];
   if (L0 && L0->simple_cnt > 0 && xw_total < (1LL << 31) && h_rowidx.size() < (1ull << 31)) {
      std::vector<LeafDesc>& h_leaf = o.h_leafdesc;
      h_leaf.resize((size_t)L0->simple_cnt);
      for (int i = 0; i < L0->simple_cnt; ++i) {
         const SnDesc& sn = h_sns[L0->simple_begin + i];
         const BlkDesc& bd = h_blks[sn.blk];
         int r_in = 0;
         while (r_in < sn.r && h_rowidx[sn.rows + r_in] < bd.n) ++r_in;
         h_leaf[i] = LeafDesc{sn.panel, (int)sn.rows, (int)bd.xw_off, sn.c0, r_in};
      }
      std::vector<int> cnt((size_t)xw_total + 1, 0);
      long long nent = 0;
      for (int i = L0->simple_begin; i < L0->simple_begin + L0->simple_cnt; ++i) {
         const SnDesc& sn = h_sns[i];
         const BlkDesc& bd = h_blks[sn.blk];
         for (int a = 0; a < sn.r; ++a) {
            const int ra = h_rowidx[sn.rows + a];
            if (ra >= bd.n) break;
            ++cnt[bd.xw_off + ra];
            ++nent;
         }
      }
      if (nent > 0 && nent < (1LL << 31)) {
         std::vector<int>&h_rows = o.h_lf_rows, &h_ptr = o.h_lf_ptr, &h_src = o.h_lf_src, &h_pos = o.h_lf_pos;
         h_ptr.assign(1, 0); h_src.assign((size_t)nent, 0); h_pos.assign(h_rowidx.size(), -1);
         std::vector<int> slot((size_t)xw_total, -1);   // target row -> its index in the compact list
         for (long long t = 0; t < xw_total; ++t)
            if (cnt[t] > 0) { slot[t] = (int)h_rows.size(); h_rows.push_back((int)t); h_ptr.push_back(h_ptr.back() + cnt[t]); }
         std::vector<int> fill(h_ptr.begin(), h_ptr.end() - 1);
         for (int i = L0->simple_begin; i < L0->simple_begin + L0->simple_cnt; ++i) {   // ascending leaves: the order of every sum
            const SnDesc& sn = h_sns[i];
            const BlkDesc& bd = h_blks[sn.blk];
            for (int a = 0; a < sn.r; ++a) {
               const int ra = h_rowidx[sn.rows + a];
               if (ra >= bd.n) break;
               const int q = fill[slot[bd.xw_off + ra]]++;
               h_src[q] = (int)(bd.xw_off + sn.c0);
               h_pos[sn.rows + a] = q;
            }
         }
         o.lf_rows = (long long)h_rows.size(); o.lf_entries = nent;
      }
   }
}

// ---- which sweeps of the augmented factor pay
void layout_sweep_decisions(const std::vector<BlockSym>& sym, const LayoutKnobs& knobs, BatchLayout& o) {
   // border-backward sweep: worth it where the border rows of the factor (what it reads on top of a backward sweep) are no
   // more than what the forward sweep it saves would read, with a margin for the chain and the launches it also saves
   double fwd_entries = 0.0, border_entries = 0.0;
   int ntc_max = 0;
   for (const BlkDesc& bd : o.h_blks) ntc_max = std::max(ntc_max, bd.ntc);
   for (const BlockSym& sb : sym) {
      fwd_entries += 0.5 * (double)sb.m_pad * sb.m_pad;
      border_entries += (double)sb.nb_pad * sb.m_pad;
      for (const HeadSupernode& sn : sb.sn) {
         const int nbord = sn.r - sn.rb;
         fwd_entries += (double)sn.w * (sn.r - nbord) + 0.5 * sn.w * sn.w;
         border_entries += (double)sn.w * nbord;
      }
   }
   o.fwd_entries = fwd_entries; o.border_entries = border_entries;
   const bool sweep_enabled = ntc_max > 0 && !knobs.sweep_launches;   // the single-launch tail sweeps (SweepRt::build)
   const bool deterministic = knobs.deterministic;
   // (round 4: 3 x instead of 1.25 x - with compact front panels and the border-row arena the sweep reads the border rows as one piece per supernode;
   //  on the configs[3] share, ratio 1.23, the witness pass of a factorisation drops from two refined solves to one + this sweep)
   o.border_backward_ok = o.schur_mode_eff == 1 && o.nnzB_total > 0 && (sweep_enabled || ntc_max == 0) && !deterministic && border_entries <= 3.0 * fwd_entries;
   if (knobs.border_backward >= 0)
      o.border_backward_ok = knobs.border_backward != 0 && o.schur_mode_eff == 1 && o.nnzB_total > 0 && sweep_enabled && !deterministic;
   // Both halves of solveCompressed from the augmented factor (forward_augmented / backward_augmented): one forward and one backward
   // sweep that also read the border rows, instead of two full solves (two sweeps each, a residual check each, two border
   // products) - pays as long as the border rows are not several times what a sweep reads anyway
   // (deterministic mode: forward_augmented_det, if build_det_group_plan can build its lists - DetGroupPlan::aug_sweeps_ok)
   const bool aug_paths = o.schur_mode_eff == 1 && o.nnzB_total > 0 && (sweep_enabled || ntc_max == 0) && o.spine_total == 0;
   o.aug_sweeps_ok = aug_paths && border_entries <= 3.0 * fwd_entries;
   if (knobs.aug_sweeps >= 0) o.aug_sweeps_ok = knobs.aug_sweeps != 0 && aug_paths;
}

}  // namespace

int build_batch_layout(const std::vector<BlockInput>& in, const std::vector<BlockSym>& sym, int S, const LayoutKnobs& knobs,
                       BatchLayout& out) {
   out = BatchLayout();
   out.mf = knobs.mf;
   out.schur_mode_eff = knobs.schur_mode_eff;
   Bases B;
   int rc, nlev = 0;
   if ((rc = layout_offsets(in, sym, out.mf, out, B))) return rc;
   const std::vector<Key> keys = layout_sort_keys(sym, out.mf, knobs.mf_lds_doubles, out.nsn_total, nlev);
   out.n_levels_all = nlev;
   const int lstar = layout_spine_cut(sym, nlev, knobs);
   std::vector<std::vector<int>> sorted_id, roots_of;
   layout_supernodes(sym, keys, nlev, lstar, B, out, sorted_id, roots_of);
   if (out.mf) layout_roots_and_batches(sym, sorted_id, roots_of, out);
   if ((rc = layout_konly(sym, sorted_id, out))) return rc;
   layout_spine_lists(sym, sorted_id, lstar, out);
   layout_tail_single(sym, knobs, out);
   if ((rc = layout_index_arrays(in, sym, sorted_id, B, out))) return rc;
   if ((rc = layout_first_touch(sym, B, knobs, out))) return rc;
   layout_full_rows(in, sym, out);
   layout_border_csr(in, S, B, out);
   layout_leaf_gather(out);
   layout_sweep_decisions(sym, knobs, out);
   return PIPS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// invariants (pips_layout_probe)
// ---------------------------------------------------------------------------------------------------------------
#define LAYOUT_REQUIRE(cond, ...) \
   do { if (!(cond)) PIPS_FAIL(PIPS_ERR_STATE, "layout invariant " __VA_ARGS__); } while (0)

int check_batch_layout(const std::vector<BlockInput>& in, const std::vector<BlockSym>& sym, int S, const LayoutKnobs& knobs,
                       const BatchLayout& o) {
   const int nblk = (int)in.size();
   (void)S;
   auto scratch_of = [&](int b) { return sym[b].arena - sym[b].T_off; };
   // 1. block regions disjoint and ascending; where the tails are assembled
   for (int b = 0; b < nblk; ++b) {
      const BlkDesc& d = o.h_blks[b];
      const bool last = b + 1 == nblk;
      const BlockSym& s = sym[b];
      LAYOUT_REQUIRE(d.arena_off >= 0 && d.arena_off + s.arena <= (last ? o.arena_total : o.h_blks[b + 1].arena_off), "1: arena region of block %d", b);
      LAYOUT_REQUIRE(d.U + (long long)s.m_pad * s.m_pad <= (last ? o.uarena_total : o.h_blks[b + 1].U), "1: U-arena region of block %d", b);
      LAYOUT_REQUIRE(d.xw_off + s.n_head + s.m_pad + s.nb_pad <= (last ? o.xw_total : o.h_blks[b + 1].xw_off), "1: work-vector region of block %d", b);
      LAYOUT_REQUIRE(d.winv_off + (long long)d.ntc * TILE * TILE <= (last ? o.winv_total : o.h_blks[b + 1].winv_off), "1: winv region of block %d", b);
      LAYOUT_REQUIRE(d.dt_off + s.m_pad <= (last ? o.dtail_total : o.h_blks[b + 1].dt_off), "1: dtail region of block %d", b);
      if (!o.tail_single) LAYOUT_REQUIRE(d.T_in == d.T, "1: T_in of block %d differs from T without the single-launch tails", b);
      else {
         const long long end = last ? o.arena_total + o.bb_doubles + o.tail_scratch : o.h_blks[b + 1].T_in;
         LAYOUT_REQUIRE(d.T_in >= o.arena_total + o.bb_doubles && d.T_in + scratch_of(b) <= end, "1: scratch region of block %d", b);
      }
   }
   // 2. sorted order of the supernodes
   std::vector<long long> sn_base(nblk + 1, 0);
   for (int b = 0; b < nblk; ++b) sn_base[b + 1] = sn_base[b] + (long long)sym[b].sn.size();
   LAYOUT_REQUIRE((long long)o.h_sns.size() == sn_base[nblk] && o.nsn_total == (int)sn_base[nblk], "2: %zu supernode records", o.h_sns.size());
   std::vector<int> loc_of(o.h_sns.size()), level_of(o.h_sns.size()), sorted_of((size_t)sn_base[nblk], -1);
   for (size_t i = 0; i < o.h_sns.size(); ++i) {
      const SnDesc& sn = o.h_sns[i];
      LAYOUT_REQUIRE(sn.blk >= 0 && sn.blk < nblk && sn.c0 >= 0 && sn.c0 < sym[sn.blk].n_head, "2: supernode %zu names no head column", i);
      const int loc = sym[sn.blk].sn_of_col[sn.c0];
      LAYOUT_REQUIRE(sorted_of[(size_t)(sn_base[sn.blk] + loc)] < 0, "2: supernode %d of block %d appears twice in the sorted order", loc, sn.blk);
      sorted_of[(size_t)(sn_base[sn.blk] + loc)] = (int)i;
      loc_of[i] = loc; level_of[i] = sym[sn.blk].sn[loc].level;
      LAYOUT_REQUIRE(i == 0 || level_of[i - 1] <= level_of[i], "2: supernode %zu breaks the order by level", i);
      const int par = sym[sn.blk].sn_parent.empty() ? -1 : sym[sn.blk].sn_parent[loc];
      LAYOUT_REQUIRE(par < 0 || sym[sn.blk].sn[par].level > level_of[i], "2: head parent of supernode %zu is not on a higher level", i);
   }
   {
      int pos = 0;
      const int nl = (int)(o.levels.size() + o.levels_top.size());
      LAYOUT_REQUIRE(nl == o.n_levels_all, "2: %d level ranges for %d levels", nl, o.n_levels_all);
      for (int l = 0; l < nl; ++l) {
         const LevelRange& L = l < (int)o.levels.size() ? o.levels[l] : o.levels_top[l - (int)o.levels.size()];
         std::pair<int, int> rg[3] = {{L.simple_begin, L.simple_cnt}, {L.small_begin, L.small_cnt}, {L.large_begin, L.large_cnt}};
         std::sort(rg, rg + 3, [](auto& a, auto& b) { return (a.second > 0 ? a.first : INT_MAX) < (b.second > 0 ? b.first : INT_MAX); });
         for (auto& r : rg) {
            if (r.second <= 0) continue;
            LAYOUT_REQUIRE(r.first == pos, "2: ranges of level %d overlap or leave a gap at supernode %d", l, pos);
            pos += r.second;
         }
         LAYOUT_REQUIRE(pos <= o.nsn_total && (pos == 0 || level_of[pos - 1] <= l) && (pos == o.nsn_total || level_of[pos] > l), "2: ranges of level %d do not hold the level", l);
      }
      LAYOUT_REQUIRE(pos == o.nsn_total, "2: level ranges cover %d of %d supernodes", pos, o.nsn_total);
   }
   // 3. front launches
   if (o.mf) {
      std::vector<char> covered(o.h_sns.size(), 0);
      for (const MfLaunch& m : o.mf_launches) {
         LAYOUT_REQUIRE(m.begin >= 0 && m.cnt > 0 && m.begin + m.cnt <= o.nsn_total && m.lds_doubles <= MF_LDS_MAX, "3: front launch at %d (%d fronts, %d doubles of LDS)", m.begin, m.cnt, m.lds_doubles);
         for (int i = m.begin; i < m.begin + m.cnt; ++i) {
            const BlockSym& bs = sym[o.h_sns[i].blk];
            const HeadSupernode& s = bs.sn[loc_of[i]];
            LAYOUT_REQUIRE(!covered[i] && !is_simple(s) && level_of[i] == m.level, "3: supernode %d in a second launch, simple, or on another level", i);
            covered[i] = 1;
            const FrontLds f = front_lds(bs, loc_of[i]);
            const long long nf = s.w + mf_rows(bs, s);
            LAYOUT_REQUIRE(m.lds_doubles >= f.doubles(knobs.mf_lds_doubles), "3: launch of front %d has %d doubles of LDS, the front needs %lld", i, m.lds_doubles, f.doubles(knobs.mf_lds_doubles));
            const bool admits = m.cls >= 6 ? (!f.resident(knobs.mf_lds_doubles) && (m.cls == 7 || nf <= 256))
                                           : (f.resident(knobs.mf_lds_doubles) && (m.cls % 3 != 0 || nf <= 64) && (m.cls / 3 != 0 || s.w <= 16));
            LAYOUT_REQUIRE(admits && nf <= MF_MAX_FRONT, "3: class %d does not admit front %d (w %d, %lld rows)", m.cls, i, s.w, nf);
         }
      }
      for (size_t i = 0; i < o.h_sns.size(); ++i)
         LAYOUT_REQUIRE((covered[i] != 0) == !is_simple(sym[o.h_sns[i].blk].sn[loc_of[i]]), "3: front %zu is in no launch", i);
   } else
      LAYOUT_REQUIRE(o.mf_launches.empty() && o.n_bb == 0, "3: front launches without the multifrontal head");
   // 4. border-split batches
   if (o.n_bb > 0) {
      LAYOUT_REQUIRE((int)o.h_bb_off.size() == nblk + 1 && o.h_bb_off[nblk] == o.n_bb, "4: batch offsets");
      long long at = o.arena_total;
      for (int b = 0; b < nblk; ++b)
         for (int q = o.h_bb_off[b]; q < o.h_bb_off[b + 1]; ++q) {
            const BbBatch& c = o.h_bb_batches[q];
            LAYOUT_REQUIRE(c.cnt >= 1 && c.cnt <= BB_GMAX && c.ndoubles <= o.bb_stage && c.npos <= o.bb_poscap, "4: batch %d holds %d supernodes, %d doubles, %d rows", q, c.cnt, c.ndoubles, c.npos);
            LAYOUT_REQUIRE(c.src == at && sym[b].mf_split, "4: batch %d of block %d is not contiguous with the one before", q, b);
            at += c.ndoubles;
            for (int p = 0; p < c.npos; ++p) {
               const int pos = o.h_bb_pos[(size_t)(c.pos + p)];
               LAYOUT_REQUIRE(pos >= 0 && pos < sym[b].nb, "4: batch %d stages border row %d of %d", q, pos, sym[b].nb);
            }
         }
      LAYOUT_REQUIRE(at == o.arena_total + o.bb_doubles, "4: batches hold %lld of %lld doubles", at - o.arena_total, o.bb_doubles);
      std::vector<std::pair<long long, long long>> reg;
      for (const SnDesc& sn : o.h_sns)
         if (sn.bb >= 0) reg.push_back({sn.bb, (long long)sn.w * ((sn.r - sn.rb + 3) & ~3) + ((sn.w + 1) & ~1)});
      std::sort(reg.begin(), reg.end());
      for (size_t i = 0; i < reg.size(); ++i)
         LAYOUT_REQUIRE(reg[i].first >= o.arena_total && reg[i].first + reg[i].second <= (i + 1 < reg.size() ? reg[i + 1].first : o.arena_total + o.bb_doubles), "4: border-row regions overlap or leave the arena");
      BbPlanSize z; z.stage = o.bb_stage; z.poscap = o.bb_poscap; z.nbmax = o.bb_nbmax;
      LAYOUT_REQUIRE(bb_fits(z), "4: %zu bytes of LDS for k_border_schur", bb_lds_bytes(z));
   }
   // 5. scatter targets, diagonal positions, the two-triangle row structure
   std::vector<long long> bptr(nblk + 1, 0);
   for (int b = 0; b < nblk; ++b) bptr[b + 1] = bptr[b] + (long long)in[b].btcol.size();
   for (int b = 0; b < nblk; ++b) {
      const BlkDesc& d = o.h_blks[b];
      auto inside = [&](long long t) {
         return t == -1 || (t >= d.arena_off && t < d.arena_off + sym[b].arena) || (o.tail_single && t >= d.T_in && t < d.T_in + scratch_of(b));
      };
      for (long long p = o.kptr[b]; p < o.kptr[b + 1]; ++p) LAYOUT_REQUIRE(inside(o.h_kdst[(size_t)p]), "5: entry %lld of K leaves block %d", p, b);
      for (long long p = bptr[b]; p < bptr[b + 1]; ++p) LAYOUT_REQUIRE(inside(o.h_bdst[(size_t)p]), "5: border entry %lld leaves block %d", p, b);
      for (int i = 0; i < sym[b].n; ++i) {
         const long long dp = o.h_kdiag[(size_t)(o.x_off[b] + i)];
         LAYOUT_REQUIRE(dp >= o.kptr[b] + in[b].krow[i] && dp < o.kptr[b] + in[b].krow[i + 1] && o.h_kcolidx[(size_t)dp] == i, "5: diagonal position of row %d of block %d", i, b);
      }
   }
   LAYOUT_REQUIRE((long long)o.h_fcol.size() == 2 * o.nnzK_total - o.n_total && o.h_fsrc.size() == o.h_fcol.size(), "5: two-triangle structure holds %zu entries", o.h_fcol.size());
   {
      std::vector<int> row_of((size_t)o.nnzK_total);
      for (long long r = 0; r < o.n_total; ++r)
         for (int p = o.h_krowptr[(size_t)r]; p < o.h_krowptr[(size_t)r + 1]; ++p) row_of[(size_t)p] = (int)(r - o.h_rowbase[(size_t)r]);
      for (long long r = 0; r < o.n_total; ++r)
         for (int q = o.h_frowptr[(size_t)r]; q < o.h_frowptr[(size_t)r + 1]; ++q) {
            const int src = o.h_fsrc[(size_t)q], i = row_of[(size_t)src], j = o.h_kcolidx[(size_t)src], me = (int)(r - o.h_rowbase[(size_t)r]), c = o.h_fcol[(size_t)q];
            LAYOUT_REQUIRE((me == i && c == j) || (me == j && c == i), "5: entry %d of the two-triangle row %lld maps to (%d, %d)", q, r, i, j);
         }
   }
   // 6. the border by leaf row against the border by Schur column; the simple leaves' gather
   if (!o.h_br_rowptr.empty()) {
      std::vector<int> btrow_of((size_t)o.nnzB_total);
      for (long long r = 0; r < o.bt_rows_total; ++r)
         for (int p = o.h_bt_rowptr[(size_t)r]; p < o.h_bt_rowptr[(size_t)r + 1]; ++p) btrow_of[(size_t)p] = (int)r;
      std::vector<char> seen((size_t)o.nnzB_total, 0);
      LAYOUT_REQUIRE(o.h_br_rowptr[(size_t)o.n_total] == o.nnzB_total, "6: the border by leaf row holds %d of %lld entries", o.h_br_rowptr[(size_t)o.n_total], o.nnzB_total);
      for (long long i = 0; i < o.n_total; ++i)
         for (int q = o.h_br_rowptr[(size_t)i]; q < o.h_br_rowptr[(size_t)i + 1]; ++q) {
            const int p = o.h_br_src[(size_t)q];
            LAYOUT_REQUIRE(p >= 0 && p < o.nnzB_total && !seen[(size_t)p], "6: border entry %d taken twice", p);
            seen[(size_t)p] = 1;
            const int r = btrow_of[(size_t)p];
            LAYOUT_REQUIRE(o.h_bt_xoff[(size_t)r] + o.h_bt_colidx[(size_t)p] == i && o.h_bt_rowsc[(size_t)r] == o.h_br_sc[(size_t)q], "6: border entry %d sits in another leaf row or Schur column", p);
         }
   }
   if (o.lf_entries > 0) {
      std::vector<char> seen((size_t)o.lf_entries, 0);
      const LevelRange& L0 = o.levels[0];
      long long n_seen = 0;
      for (int i = L0.simple_begin; i < L0.simple_begin + L0.simple_cnt; ++i) {
         const SnDesc& sn = o.h_sns[i];
         bool in_block = true;
         for (int a = 0; a < sn.r; ++a) {
            in_block = in_block && o.h_rowidx[(size_t)(sn.rows + a)] < o.h_blks[sn.blk].n;
            const int q = o.h_lf_pos[(size_t)(sn.rows + a)];
            LAYOUT_REQUIRE(in_block ? (q >= 0 && q < o.lf_entries && !seen[(size_t)q]) : q == -1, "6: gather position of row %d of leaf %d", a, i);
            if (in_block) { seen[(size_t)q] = 1; ++n_seen; }
         }
      }
      LAYOUT_REQUIRE(n_seen == o.lf_entries, "6: %lld of %lld gather positions are taken", n_seen, o.lf_entries);
   }
   return PIPS_OK;
}

void BatchLayout::drop_uploaded() {
   auto drop = [](auto&... v) { (std::decay_t<decltype(v)>().swap(v), ...); };
   drop(h_rowidx, h_sncol, h_bmap, h_perm, h_upd, h_mfint, h_nprimal, h_psign, h_psign_off, h_perm_off, h_kdst, h_bdst, h_kdiag, h_rowbase,
        h_krowptr, h_kcolidx, h_frowptr, h_fcol, h_fsrc, h_flong, h_bt_rowptr, h_bt_colidx, h_bt_xoff, h_bval, h_br_rowptr, h_br_sc, h_br_src,
        h_schur_slot, h_leafdesc, h_lf_rows, h_lf_ptr, h_lf_src, h_lf_pos, h_lb_list, tile_first, h_roots, h_bb_batches, h_bb_meta, h_bb_pos,
        h_kb_rec, h_kb_list, h_kb_tail, h_kb_off, h_spine, h_spine_off, h_ft_colbase, h_ft_init_off, h_ft_piece_off, h_ft_init, h_ft_piece,
        h_ft_leaves);
}

void read_layout_knobs(const EngineSettings* e, AnalyzeOptions& opt, AnalyzeKnobs& knobs) {
   // Tile geometry + the cost-model / amalgamation knobs (environment overrides are for tuning runs only).
   opt.tile = TILE;
   // Supernode width cap.  16 instead of the kernels' limit of 32: on the time-coupled family (tools/config3_probe.py, 64 x 50 000)
   // narrower supernodes carry fewer explicit zeros (nnz(L) 164 M -> 151 M), halve the dependent pivot chain of a front and the
   // registers its rows take; factorisation 13.4 -> 12.5 ms, solveCompressed 9.3 -> 8.9 ms.  Random sparsity (config 2) has no
   // supernodes wider than one column in the head.
   opt.max_sn_width = 16;
   if (knob_set<K_SN_WIDTH>()) opt.max_sn_width = std::max(1, std::min(HEAD_WMAX, (int)knob_int<K_SN_WIDTH>()));
   else if (e && e->sn_width > 0) opt.max_sn_width = std::min(HEAD_WMAX, e->sn_width);
   // (a switch that is not set leaves what opt holds: the values of AnalyzeOptions, or what an earlier analysis of this engine left)
   if (knob_set<K_RELAX_ZEROS>()) opt.relax_zeros = knob_real<K_RELAX_ZEROS>();
   if (knob_set<K_ND_DEPTH>()) opt.nd_depth = (int)knob_int<K_ND_DEPTH>();
   if (knob_set<K_ND_MIN>()) opt.nd_min_size = (int)knob_int<K_ND_MIN>();
   if (knob_set<K_MF_LDS>()) opt.mf_lds_doubles = knob_int<K_MF_LDS>();
   if (knob_set<K_MF_SPLIT>()) { const int sp = (int)knob_int<K_MF_SPLIT>(); opt.mf_split_nb_max = sp == 0 ? 0 : std::min(176, std::max(sp, 2)); }
   knobs.deterministic = e && e->deterministic;
   knobs.schur_mode = e ? e->schur_mode : 0;
   // (tests: forces a Schur mode where no setter reaches - the leaf handles and the batch they are bound into - and the caller left it to the model)
   if (e && knobs.schur_mode == 0) knobs.schur_mode = std::max(0, std::min(2, (int)knob_int<K_SCHUR_MODE>()));
   knobs.mf_lds_doubles = opt.mf_lds_doubles;
   knobs.mf_wanted = knob_int<K_MF>() != 0;
   if (!knobs.mf_wanted) opt.mf_split_nb_max = 0;   // the border split (compact front panels) only exists with the multifrontal head
   // fronts on the rows of K only where the border split applies (value 1; off by default: on the configs[3] share the fronts fall
   // from 9.7 to 4.0 ms, forming the border rows afterwards costs 8.0 - DESIGN.md 4.1c): not in deterministic mode (the border rows of the dense
   // tail take their head contributions with atomics, k_border_tail) and with supernodes of at most 16 columns (k_border_rows<., 16>)
   opt.mf_konly = opt.mf_split_nb_max > 0 && !knobs.deterministic && opt.max_sn_width <= 16 && knob_int<K_MF_KONLY>() != 0;
   knobs.spine = knob_tri<K_SPINE>();
   knobs.tail_single = knob_tri<K_TAIL_SINGLE>();
   knobs.tail_first_touch = knob_tri<K_TAIL_FIRST_TOUCH>();
   static_assert(KNOBS[K_FIRST_TOUCH_LDS].dflt == FT_LDS_BUDGET, "the table's default is the layout's budget");
   knobs.ft_lds_bytes = std::min(FT_LDS_MAX, std::max(0LL, knob_int<K_FIRST_TOUCH_LDS>()));   // (never more than a workgroup can have)
   knobs.border_backward = knob_tri<K_BORDER_BACKWARD>();
   knobs.aug_sweeps = knob_tri<K_AUG_SWEEPS>();
   knobs.sweep_launches = knob_set<K_SWEEP_LAUNCHES>();   // (SweepRt::build: the single-launch sweeps are off)
   const long long poll = knob_int<K_ROOT_POLL_LIMIT>();
   knobs.tail_poll_limit = poll > 0 ? poll * 50 : 0;   // (a deep update runs a millisecond)
   knobs.tail_diag_blocked = knob_int<K_ROOT_DIAG_BARRIERS>() ? 0 : 1;
}

void sym_info(const std::vector<BlockSym>& sym, int64_t* what, int n_what) {
   int64_t v[13] = {0};
   for (const BlockSym& s : sym) {
      v[10] += (int64_t)s.upd.size() * 4;
      v[11] += s.nb;
      v[12] += (int64_t)s.a_dst.size();
      v[0] += s.nnzL; v[1] += s.n; v[2] += s.n_head; v[3] += s.m; v[4] += (int64_t)s.sn.size();
      v[5] = std::max<int64_t>(v[5], s.n_levels);
      v[6] += (int64_t)s.flops_factor; v[7] += (int64_t)s.flops_border; v[8] += s.arena * 8;
      v[9] = std::max<int64_t>(v[9], s.m_pad / TILE);
   }
   for (int i = 0; i < n_what && i < 13; ++i) what[i] = v[i];
}

}  // namespace pips

// ---- probe of the packed blocked solves' tables (CPU only): schur_pack_block as schur_pack_rows (Engine::set_sc_tables) calls it
extern "C" int pips_schur_pack_probe(int nblk, int S, const int* const* bt_rowptr, int* nb, int* nb_max, int* const* local_of_row) {
   if (nblk <= 0 || S < 0 || !bt_rowptr || !nb || !nb_max || !local_of_row) PIPS_FAIL(pips::PIPS_ERR_ARG, "pips_schur_pack_probe: bad arguments");
   *nb_max = 0;
   for (int b = 0; b < nblk; ++b) {
      if (!local_of_row[b]) PIPS_FAIL(pips::PIPS_ERR_ARG, "pips_schur_pack_probe: local_of_row[%d] is NULL", b);
      nb[b] = pips::schur_pack_block(S, bt_rowptr[b], local_of_row[b]);
      *nb_max = std::max(*nb_max, nb[b]);
   }
   return pips::PIPS_OK;
}
