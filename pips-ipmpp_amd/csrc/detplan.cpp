// Host plans of deterministic mode (detplan.h): groups, rounds and gather lists.  No device call, no environment read.
#include "detplan.h"

#include <algorithm>
#include <climits>
#include <type_traits>
#include <utility>

namespace pips {

// the recorded contributions (target, slot) are sorted, then turned into the CSR "target -> its slots"
HostGather make_gather(std::vector<SlotEntry>& e) {
   std::sort(e.begin(), e.end(), [](const SlotEntry& a, const SlotEntry& b) { return a.target != b.target ? a.target < b.target : a.slot < b.slot; });
   HostGather g;
   g.slots.resize(e.size());
   for (size_t i = 0; i < e.size(); ++i) {
      if (i == 0 || e[i].target != e[i - 1].target) { g.tgt.push_back(e[i].target); g.off.push_back((long long)i); }
      g.slots[i] = e[i].slot;
   }
   g.off.push_back((long long)e.size());
   return g;
}

// classify: Schur complement / tail of block b / head panel of a supernode at level l (targets of different blocks are disjoint)
int classify_factor_slots(const std::vector<long long>& rec, long long sc_flag, const BatchLayout& lay, const std::vector<BlockSym>& sym,
                          FactorSlotPlan& out) {
   const int nlev = (int)lay.levels.size(), nblk = (int)lay.h_blks.size();
   out = FactorSlotPlan();
   std::vector<std::vector<SlotEntry>> per_level(nlev);
   std::vector<SlotEntry> tail_e, sc_e;
   std::vector<std::vector<std::pair<long long, int>>> panel_level(nblk);   // (panel offset inside the block arena, level), ascending
   for (int b = 0; b < nblk; ++b) {
      for (const HeadSupernode& hs : sym[b].sn) panel_level[b].push_back({hs.panel, hs.level});
      std::sort(panel_level[b].begin(), panel_level[b].end());
   }
   for (int i = 0; i < lay.nsn_total; ++i) {
      const SnDesc& sn = lay.h_sns[i];
      if (lay.mf && !(sn.mf < 0 && sn.n_useg == 0)) continue;   // multifrontal head: only the leaves without a front above them own slots
      const long long cnt = (long long)sn.r * (sn.r + 1) / 2;
      const BlkDesc& bd = lay.h_blks[sn.blk];
      for (long long q = 0; q < cnt; ++q) {
         const long long t = rec[(size_t)(sn.slot + q)];
         if (t < 0) continue;
         if (t & sc_flag) { sc_e.push_back({t & ~sc_flag, sn.slot + q}); out.kept.blk.push_back(sn.blk); continue; }
         if (t >= bd.T) { tail_e.push_back({t, sn.slot + q}); continue; }
         const long long rel = t - bd.arena_off;
         auto& pl = panel_level[sn.blk];
         auto it = std::upper_bound(pl.begin(), pl.end(), std::make_pair(rel, INT_MAX));
         if (it == pl.begin()) PIPS_FAIL(PIPS_ERR_STATE, "deterministic mode: a recorded target lies outside every head panel");
         per_level[std::prev(it)->second].push_back({t, sn.slot + q});
      }
   }
   for (int l = 0; l < nlev; ++l) out.levels.push_back(make_gather(per_level[l]));
   out.kept.e = sc_e;   // (unsorted, parallel to kept.blk) for the group-wise variant of deterministic mode
   out.tail = make_gather(tail_e);
   out.sc = make_gather(sc_e);
   return PIPS_OK;
}

void classify_solve_slots(const std::vector<long long>& vrec, const BatchLayout& lay, const std::vector<BlockSym>& sym, SolveSlotPlan& out) {
   const int nlev = (int)lay.levels.size();
   out = SolveSlotPlan();
   std::vector<std::vector<SlotEntry>> v_level(nlev);
   std::vector<SlotEntry> v_tail;
   for (int i = 0; i < lay.nsn_total; ++i) {
      const SnDesc& sn = lay.h_sns[i];
      const BlkDesc& bd = lay.h_blks[sn.blk];
      for (int a = 0; a < sn.r; ++a) {
         const long long t = vrec[(size_t)(sn.vslot + a)];
         if (t < 0) continue;
         const long long col = t - bd.xw_off;
         if (col >= bd.n_head) { v_tail.push_back({t, sn.vslot + a}); continue; }
         const int loc = sym[sn.blk].sn_of_col[(size_t)col];
         v_level[sym[sn.blk].sn[loc].level].push_back({t, sn.vslot + a});
      }
   }
   for (int l = 0; l < nlev; ++l) out.levels.push_back(make_gather(v_level[l]));
   out.tail = make_gather(v_tail);
}

BorderGathers border_product_gathers(const BatchLayout& lay) {
   std::vector<SlotEntry> by_sc, by_entry;
   for (long long i = 0; i < lay.bt_rows_total; ++i) {
      if (lay.h_bt_rowptr[i + 1] > lay.h_bt_rowptr[i]) by_sc.push_back({(long long)lay.h_bt_rowsc[i], i});
      for (int q = lay.h_bt_rowptr[i]; q < lay.h_bt_rowptr[i + 1]; ++q) by_entry.push_back({lay.h_bt_xoff[i] + lay.h_bt_colidx[q], (long long)q});
   }
   BorderGathers g;
   g.btm = make_gather(by_sc);
   g.bm = make_gather(by_entry);
   return g;
}

namespace {

DetAugPlan build_det_aug(const BatchLayout& lay, const std::vector<BlockSym>& sym, int S, const std::vector<int>& grp) {
   DetAugPlan p;
   const int nblk = (int)lay.h_blks.size();
   if (!lay.aug_sweeps_ok || lay.h_sns.empty()) return p;
   std::vector<long long> tbase(nblk + 1, 0);
   for (int b = 0; b < nblk; ++b) tbase[b + 1] = tbase[b] + lay.h_blks[b].nb;
   const long long nt = tbase[nblk];
   if (nt == 0) return p;
   std::vector<long long> cnt((size_t)nt + 1, 0);
   auto for_rows = [&](auto&& fn) {
      for (size_t i = 0; i < lay.h_sns.size(); ++i) {
         const SnDesc& sn = lay.h_sns[i];
         if (sn.rb >= sn.r) continue;
         const BlockSym& bs = sym[sn.blk];
         const int loc = bs.sn_of_col[(size_t)sn.c0];
         const int* rows = bs.rowidx.data() + bs.sn[loc].rows;
         for (int a = sn.rb; a < sn.r; ++a) fn(sn, tbase[sn.blk] + (rows[a] - bs.n), a);
      }
   };
   for_rows([&](const SnDesc&, long long t, int) { ++cnt[(size_t)t + 1]; });
   for (long long t = 0; t < nt; ++t) cnt[(size_t)t + 1] += cnt[(size_t)t];
   // entries in the order of the supernode array (a supernode's border rows side by side: the threads of k_border_rowdot_det read them
   // coalesced); per target the indices of its entries, ascending
   const long long n_ent = cnt[(size_t)nt];
   if (n_ent >= (1LL << 31) || lay.xw_total >= (1LL << 32)) return p;   // (index widths of the lists; the refined path stays)
   std::vector<BgEntry> ent((size_t)n_ent);
   std::vector<int> idx((size_t)n_ent);
   std::vector<long long> fill(cnt.begin(), cnt.end() - 1);
   bool ok = true;
   long long e_next = 0;
   for_rows([&](const SnDesc& sn, long long t, int a) {
      BgEntry e;
      const bool in_panel = sn.ld >= sn.w + sn.r;
      const int stride = in_panel ? sn.ld : ((sn.r - sn.rb + 3) & ~3);
      if (!in_panel && sn.bb < 0) ok = false;
      if (stride > 65535 || sn.w > 65535) ok = false;
      e.off = in_panel ? sn.panel + sn.w + a : sn.bb + (a - sn.rb);
      e.y = (unsigned)(lay.h_blks[sn.blk].xw_off + sn.c0); e.stride = (unsigned short)stride; e.w = (unsigned short)sn.w;
      idx[(size_t)fill[(size_t)t]++] = (int)e_next;
      ent[(size_t)e_next++] = e;
   });
   if (!ok) return p;   // (a layout this sweep does not read: the refined path stays)
   std::vector<long long> slot((size_t)nt);
   std::vector<SlotEntry> col;
   for (int b = 0; b < nblk; ++b)
      for (int g = 0; g < lay.h_blks[b].nb; ++g) {
         slot[(size_t)(tbase[b] + g)] = lay.h_blks[b].xw_off + lay.h_blks[b].n_head + lay.h_blks[b].m_pad + g;
         col.push_back({(long long)grp[b] * S + sym[b].bmap[(size_t)g], slot[(size_t)(tbase[b] + g)]});
      }
   p.ent = std::move(ent); p.ptr = std::move(cnt); p.idx = std::move(idx); p.slot = std::move(slot);
   p.bslot_grp = make_gather(col);
   p.n_ent = n_ent;
   p.n_targets = nt;
   p.ready = true;
   return p;
}

// the blocks of round k = the k-th block of every group that `has` something to add: one block per group and launch
template <class Has>
void block_rounds(int nblk, int gs, Has has, std::vector<int>& blk, std::vector<int>& off) {
   blk.clear();
   off.assign(1, 0);
   for (int k = 0; k < gs; ++k) {
      for (int b = k; b < nblk; b += gs)
         if (has(b)) blk.push_back(b);
      off.push_back((int)blk.size());
   }
   if (blk.empty()) blk.push_back(0);
}

}  // namespace

DetGroupPlan build_det_group_plan(const BatchLayout& lay, const std::vector<BlockSym>& sym, int S, int rank, int n_ranks, long long gstride,
                                  const ScKept& kept, const PackedTables& packed) {
   DetGroupPlan p;
   const int nblk = (int)lay.h_blks.size();
   p.slots = (n_ranks >= 1 && n_ranks <= 8 && 8 % n_ranks == 0) ? 8 / n_ranks : 8;
   p.first_slot = p.slots == 8 ? 0 : rank * p.slots;
   p.global = n_ranks > 1 && p.slots < 8;
   const int gs = std::max(1, (nblk + p.slots - 1) / p.slots);     // blocks per group
   p.n_groups = (nblk + gs - 1) / gs;
   p.grp.assign(std::max(nblk, 1), 0);
   for (int b = 0; b < nblk; ++b) p.grp[b] = b / gs;
   const std::vector<int>& grp = p.grp;
   std::vector<std::vector<TileTask>> rounds(gs);
   for (int b = 0; b < nblk; ++b) {
      if (lay.h_blks[b].ntc <= 0 || lay.h_blks[b].nb <= 0) continue;
      const int nt = lay.h_blks[b].nb_pad / TILE;
      for (int ti = 0; ti < nt; ++ti)
         for (int tj = 0; tj <= ti; ++tj) rounds[b % gs].push_back({b, ti, tj, 0});
   }
   for (int k = 0; k < gs; ++k) {
      TaskList l;
      l.off = (long long)p.tasks.size(); l.cnt = (int)rounds[k].size();
      p.tasks.insert(p.tasks.end(), rounds[k].begin(), rounds[k].end());
      p.rounds.push_back(l);
   }
   if (p.tasks.empty()) p.tasks.push_back({-1, 0, 0, 0});
   if (lay.mf) {
      block_rounds(nblk, gs, [&](int b) { return lay.h_root_off[b + 1] > lay.h_root_off[b]; }, p.round_blk, p.round_off);
      block_rounds(nblk, gs, [&](int b) { return lay.n_bb > 0 && lay.h_bb_off[b + 1] > lay.h_bb_off[b]; }, p.bb_round_blk, p.bb_round_off);
   }
   {  // the head's own Schur contributions join their block's group buffer
      std::vector<SlotEntry> ent(kept.e.size());
      for (size_t i = 0; i < kept.e.size(); ++i) ent[i] = {(long long)grp[kept.blk[i]] * gstride + kept.e[i].target, kept.e[i].slot};
      p.sc_grp = make_gather(ent);
   }
   if (S > 0) {   // Br^T z in the same group order: rows of group g go to slot g of an 8 x S scratch matrix
      std::vector<SlotEntry> ent;
      for (long long i = 0; i < lay.bt_rows_total; ++i)
         if (lay.h_bt_rownnz[(size_t)i] > 0) ent.push_back({(long long)grp[lay.h_bt_rowblk[(size_t)i]] * S + lay.h_bt_rowsc[(size_t)i], i});
      p.btm_grp = make_gather(ent);
      p.aug = build_det_aug(lay, sym, S, grp);
   }
   // packed blocked solves: per (group, position of the value array) its contributions (border row << 24 | local column); sorted by
   // that word = by block within a target, the order k_border_tmult_chunk_packed_det adds them in
   if (packed.rows) {
      const PackRows& pk = *packed.rows;
      std::vector<SlotEntry> ent;
      for (long long i = 0; i < lay.bt_rows_total; ++i)
         for (int q = 0; q <= pk.la[(size_t)i]; ++q)
            ent.push_back({(long long)grp[lay.h_bt_rowblk[(size_t)i]] * gstride + (*packed.tab)[(size_t)(pk.tabrow[(size_t)i] + q)], (i << 24) | q});
      p.pk_grp = make_gather(ent);
   }
   // (deterministic mode takes the sweeps of the augmented factor only through forward_augmented_det)
   p.aug_sweeps_ok = lay.aug_sweeps_ok && p.aug.ready;
   return p;
}

void DetGroupPlan::drop_uploaded() {
   auto drop = [](auto&... v) { (std::decay_t<decltype(v)>().swap(v), ...); };
   drop(grp, tasks, round_blk, bb_round_blk, aug.ent, aug.ptr, aug.slot, aug.idx);
   sc_grp = btm_grp = pk_grp = aug.bslot_grp = HostGather();
}

ScPanelPlan sc_panel_plan(const BatchLayout& lay, const std::vector<BlockSym>& sym, int S, int n_panels) {
   ScPanelPlan p;
   const int nblk = (int)lay.h_blks.size();
   n_panels = std::min(n_panels, std::max(1, S / (2 * TILE)));
   if (n_panels <= 1 || lay.schur_mode_eff != 1) return p;
   for (int q = 0; q <= n_panels; ++q) p.row_begin.push_back(q == n_panels ? S : (int)((long long)S * q / n_panels) / TILE * TILE);
   std::vector<std::vector<TileTask>> g(n_panels);
   for (int b = 0; b < nblk; ++b) {
      if (lay.h_blks[b].ntc <= 0 || lay.h_blks[b].nb <= 0) continue;
      const int nt = lay.h_blks[b].nb_pad / TILE;
      for (int ti = 0; ti < nt; ++ti) {
         // a tile row belongs to the panel of its FIRST Schur row: every tile row that touches panel q then sits in a group <= q
         // (compressed border ids ascend like the Schur ids), so panel q is final once group q has run
         const int first = sym[b].bmap[std::min(ti * TILE, lay.h_blks[b].nb - 1)];
         int q = (int)(std::upper_bound(p.row_begin.begin(), p.row_begin.end(), first) - p.row_begin.begin()) - 1;
         q = std::max(0, std::min(q, n_panels - 1));
         for (int tj = 0; tj <= ti; ++tj) g[q].push_back({b, ti, tj, 0});
      }
   }
   for (int q = 0; q < n_panels; ++q) {
      TaskList l;
      l.off = (long long)p.tasks.size(); l.cnt = (int)g[q].size();
      p.tasks.insert(p.tasks.end(), g[q].begin(), g[q].end());
      p.groups.push_back(l);
   }
   if (p.tasks.empty()) p.tasks.push_back({-1, 0, 0, 0});
   return p;
}

}  // namespace pips
