// Host task plans of the tiled dense LDL^T: see tileplan.h.
#include "tileplan.h"

#include <algorithm>
#include <map>
#include <utility>

namespace pips {

namespace {

// A column plan under construction: the tasks of all lists in the order the lists are closed, and what the two builders share
struct ColumnLists {
   ColumnPlan& p;
   const std::vector<BlkDesc>& blks;
   const TileFirst* first;   // nullptr: no envelope
   const int nblk;
   std::vector<TileTask> all;

   ColumnLists(ColumnPlan& p_, const std::vector<BlkDesc>& blks_, const TileFirst* first_) : p(p_), blks(blks_), first(first_), nblk((int)blks_.size()) {
      p.ntc_max = 0;
      for (auto& b : blks) p.ntc_max = std::max(p.ntc_max, b.ntc);
      for (std::vector<TaskList>* l : {&p.upd, &p.upd_diag, &p.diag, &p.trsm, &p.fwd, &p.bwd, &p.trail, &p.trail_next}) l->assign(p.ntc_max, {});
   }
   int fst(int b, int t) const { return first ? (*(*first)[b])[t] : 0; }
   void begin(TaskList& l) { l.off = (long long)all.size(); }
   void end(TaskList& l) { l.cnt = (int)((long long)all.size() - l.off); }
   void push(int b, int ti, int tj, int pad = 0) { all.push_back({b, ti, tj, pad}); }

   // tile column j once its updates are listed: the diagonal tiles, the trsm below them, the two launch-per-column solve sweeps
   void factor_and_sweeps(int j) {
      begin(p.diag[j]);
      for (int b = 0; b < nblk; ++b)
         if (blks[b].ntc > j) push(b, j, j);
      end(p.diag[j]);
      begin(p.trsm[j]);
      for (int b = 0; b < nblk; ++b)
         if (blks[b].ntc > j)
            for (int ti = j + 1; ti < blks[b].ntr; ++ti)
               if (j >= fst(b, ti)) push(b, ti, j);
      end(p.trsm[j]);
      begin(p.fwd[j]);
      for (int b = 0; b < nblk; ++b)
         if (blks[b].ntc > j)
            for (int ti = j; ti < blks[b].ntc; ++ti)
               if (ti == j || (j >= 1 && j - 1 >= fst(b, ti))) push(b, ti, j);   // L(ti, j-1) inside the envelope
      end(p.fwd[j]);
      begin(p.bwd[j]);
      for (int b = 0; b < nblk; ++b)
         if (blks[b].ntc > j)
            for (int tj = 0; tj <= j; ++tj)
               if (tj == j || (j + 1 < blks[b].ntc && tj >= fst(b, j + 1))) push(b, tj, j);   // L(j+1, tj)
      end(p.bwd[j]);
   }
   // the Schur SYRK: the lower triangle of the border tiles of every block with a tail and a border; then the plan owns the tasks
   void finish() {
      begin(p.schur);
      for (int b = 0; b < nblk; ++b)
         if (blks[b].ntc > 0 && blks[b].nb > 0) {
            const int nt = blks[b].nb_pad / TILE;
            for (int ti = 0; ti < nt; ++ti)
               for (int tj = 0; tj <= ti; ++tj) push(b, ti, tj);
         }
      end(p.schur);
      p.h_tasks = std::move(all);
   }
};

}  // namespace

void ColumnPlan::build_leaf(const std::vector<BlkDesc>& blks, const TileFirst& first, int group) {
   ColumnLists c(*this, blks, &first);
   const int nblk = c.nblk, P = std::max(group, 1);
   for (int j = 0; j < ntc_max; ++j) {
      const int g = j / P * P, q = j - g;   // j is column q of the group that starts at g
      c.begin(upd_diag[j]);
      if (j > 0)
         for (int b = 0; b < nblk; ++b)
            if (blks[b].ntc > j) {
               const int k0 = c.fst(b, j);
               if (k0 < j) c.push(b, j, j, std::max(k0, j - 1) | (j << 16));
            }
      c.end(upd_diag[j]);
      c.begin(upd[j]);
      if (j > 0) {
         // the next diagonal tile with the columns < j (the group's own where j is not its first: the launch of column g took the rest)
         for (int b = 0; b < nblk; ++b)
            if (blks[b].ntc > j + 1) {
               const int k0 = c.fst(b, j + 1), lo = q > 0 ? std::max(k0, g) : k0;
               if (lo < j) c.push(b, j + 1, j + 1, lo | (j << 16));
            }
         // first column of a group: the diagonal tiles up to the next group's first, with everything left of the group
         if (q == 0)
            for (int b = 0; b < nblk; ++b)
               for (int d = j + 2; d <= j + P && d < blks[b].ntc; ++d) {
                  const int k0 = c.fst(b, d);
                  if (k0 < j) c.push(b, d, d, k0 | (j << 16));
               }
         for (int b = 0; b < nblk; ++b)
            if (blks[b].ntc > j)
               for (int ti = j + 1; ti < blks[b].ntr; ++ti) {
                  if (j >= c.fst(b, ti)) {                                         // (else outside the envelope: stays zero)
                     const int k0 = std::max(c.fst(b, ti), c.fst(b, j)), lo = q > 0 ? std::max(k0, g) : k0;
                     if (lo < j) c.push(b, ti, j, lo | (j << 16));
                  }
                  if (q == 0)   // ... and beside it the row's tiles in the other columns of the group, with everything left of the group
                     for (int t = j + 1; t < j + P && t < blks[b].ntc && t < ti; ++t)
                        if (t >= c.fst(b, ti)) {
                           const int k0 = std::max(c.fst(b, ti), c.fst(b, t));
                           if (k0 < j) c.push(b, ti, t, k0 | (j << 16));
                        }
               }
      }
      c.end(upd[j]);
      c.factor_and_sweeps(j);
   }
   c.finish();
}

void ColumnPlan::build_root(const std::vector<BlkDesc>& blks, int panel, bool lookahead) {
   ColumnLists c(*this, blks, nullptr);
   const int nblk = c.nblk;
   for (int j = 0; j < ntc_max; ++j) {
      const int p0 = panel > 0 ? j / panel * panel : 0;   // first tile column of j's panel
      c.begin(upd_diag[j]);
      c.end(upd_diag[j]);
      c.begin(upd[j]);
      if (j > p0)
         for (int b = 0; b < nblk; ++b)
            if (blks[b].ntc > j)
               for (int ti = j; ti < blks[b].ntr; ++ti) c.push(b, ti, j, p0 | (j << 16));
      c.end(upd[j]);
      c.factor_and_sweeps(j);
      // panel [p0, j] complete: apply it to every tile right of it
      if (panel > 0 && (j + 1) % panel == 0) {
         c.begin(trail_next[j]);
         if (lookahead)
            for (int b = 0; b < nblk; ++b)
               if (j + 1 < blks[b].ntc)
                  for (int ti = j + 1; ti < blks[b].ntr; ++ti) c.push(b, ti, j + 1, p0 | ((j + 1) << 16));
         c.end(trail_next[j]);
         c.begin(trail[j]);
         for (int b = 0; b < nblk; ++b)
            for (int tj = j + (lookahead ? 2 : 1); tj < blks[b].ntc; ++tj)
               for (int ti = tj; ti < blks[b].ntr; ++ti) c.push(b, ti, tj, p0 | ((j + 1) << 16));
         c.end(trail[j]);
      }
   }
   c.finish();
}

void GroupPlan::build(const ColumnPlan& p, int P_) {
   *this = GroupPlan();
   P = P_;
   n_groups = (p.ntc_max + P - 1) / P;
   struct Group { std::vector<TileTask> deep, pre, block_deep; std::map<std::pair<int, int>, std::vector<TileTask>> strips; };
   std::vector<Group> gs(n_groups);
   std::vector<std::vector<TileTask>> ui(p.ntc_max), ti(p.ntc_max);
   auto each = [&](const TaskList& l, auto&& f) {
      for (long long q = l.off; q < l.off + l.cnt; ++q)
         if (p.h_tasks[q].blk >= 0) f(p.h_tasks[q]);
   };
   auto update = [&](const TileTask& t) {
      const int k1 = t.pad >> 16, g = k1 / P * P;
      if (t.ti >= g + P) {
         if (k1 == g) gs[g / P].deep.push_back(t);
         else if (t.ti == t.tj) gs[t.tj / P].pre.push_back(t);
         else gs[g / P].strips[{t.blk, t.ti}].push_back(t);
      } else if (k1 == g)
         gs[g / P].block_deep.push_back(t);
      else
         ui[k1].push_back(t);
   };
   for (int j = 0; j < p.ntc_max; ++j) {
      each(p.upd_diag[j], update);
      each(p.upd[j], update);
      each(p.trsm[j], [&](const TileTask& t) {
         const int g = j / P * P;
         if (t.ti >= g + P) gs[g / P].strips[{t.blk, t.ti}].push_back(t);
         else ti[j].push_back(t);
      });
   }
   auto put = [&](TaskList& l, const std::vector<TileTask>& v) {
      l.off = (long long)h_tasks.size(); l.cnt = (int)v.size();
      h_tasks.insert(h_tasks.end(), v.begin(), v.end());
   };
   deep.assign(n_groups, {}); pre.assign(n_groups, {}); block_deep.assign(n_groups, {}); strips.assign(n_groups, {});
   upd_in.assign(p.ntc_max, {}); trsm_in.assign(p.ntc_max, {});
   // a strip's order: the update with columns < k1 before the trsm of column k1 and after that of column k1 - 1
   auto step = [](const TileTask& t) { return t.pad ? 2 * (t.pad >> 16) : 2 * t.tj + 1; };
   for (int i = 0; i < n_groups; ++i) {
      put(deep[i], gs[i].deep);
      put(pre[i], gs[i].pre);
      put(block_deep[i], gs[i].block_deep);
      strips[i].off = (long long)h_strips.size();
      for (auto& kv : gs[i].strips) {   // (block, tile row) ascending: a block's strips side by side
         std::vector<TileTask>& v = kv.second;
         std::stable_sort(v.begin(), v.end(), [&](const TileTask& a, const TileTask& b) { return step(a) != step(b) ? step(a) < step(b) : a.tj < b.tj; });
         h_strips.push_back({(int)h_tasks.size(), (int)v.size()});
         h_tasks.insert(h_tasks.end(), v.begin(), v.end());
      }
      strips[i].cnt = (int)((long long)h_strips.size() - strips[i].off);
      for (int j = i * P; j < std::min((i + 1) * P, p.ntc_max); ++j) {
         put(upd_in[j], ui[j]);
         put(trsm_in[j], ti[j]);
      }
   }
}

void SweepLists::build(const std::vector<BlkDesc>& blks, const TileFirst* first) {
   *this = SweepLists();
   const int nblk = (int)blks.size();
   int ntc_max = 0;
   for (auto& b : blks) ntc_max = std::max(ntc_max, b.ntc);
   for (int i = 0; i < ntc_max; ++i)
      for (int b = 0; b < nblk; ++b)
         if (i < blks[b].ntc) tasks.push_back({b, i, 0, 0});
   flag_off.assign(nblk, 0);
   tfirst_off.assign(nblk, 0);
   for (int b = 0; b < nblk; ++b) {
      flag_off[b] = n_flags;
      n_flags += blks[b].ntc;
      tfirst_off[b] = (long long)tfirst.size();
      if (first)   // tail rows and, behind them, the border tile rows (border-backward sweep)
         for (int i = 0; i < blks[b].ntr; ++i) tfirst.push_back(i < blks[b].ntc ? std::min(i, (*(*first)[b])[i]) : (*(*first)[b])[i]);
   }
}

void TailSingleLists::build(const ColumnPlan& p, const std::vector<BlkDesc>& blks) {
   *this = TailSingleLists();
   const int nblk = (int)blks.size();
   foff.assign(nblk + 1, 0);
   for (int b = 0; b < nblk; ++b) foff[b + 1] = foff[b] + (long long)blks[b].ntr * blks[b].ntc + blks[b].ntr + blks[b].ntc;
   n_flags = foff[nblk];
   // the template: prog of a tile = the first K its first update starts from (an update waits for prog >= its k0: the one before it has
   // stored the tile), = its tile column where it takes no update at all (trsm / the diagonal role wait for prog >= tile column)
   init.assign((size_t)std::max<long long>(n_flags, 1), 0);
   for (int b = 0; b < nblk; ++b)
      for (int ti = 0; ti < blks[b].ntr; ++ti)
         for (int tj = 0; tj < blks[b].ntc; ++tj) init[foff[b] + (long long)ti * blks[b].ntc + tj] = -1;
   std::vector<TileTask> order;
   auto take = [&](const TaskList& l, int kind) {
      for (long long q = l.off; q < l.off + l.cnt; ++q) {
         TileTask t = p.h_tasks[q];
         if (t.blk < 0) continue;
         if (kind == ROOT_UPD) {
            int& pr = init[foff[t.blk] + (long long)t.ti * blks[t.blk].ntc + t.tj];
            if (pr < 0) pr = t.pad & 0xffff;
         } else
            t.pad = 0;
         t.blk |= kind << 24;
         order.push_back(t);
      }
   };
   // first tile column of every tile row (its envelope): the trsm of a row commit in column order from there (root_do)
   std::vector<int> row_first((size_t)std::max<long long>(n_flags, 1), 1 << 20);
   for (int j = 0; j < p.ntc_max; ++j)
      for (long long q = p.trsm[j].off; q < p.trsm[j].off + p.trsm[j].cnt; ++q) {
         const TileTask& t = p.h_tasks[q];
         if (t.blk >= 0) { int& f = row_first[foff[t.blk] + t.ti]; f = std::min(f, t.tj); }
      }
   for (int j = 0; j < p.ntc_max; ++j) {
      take(p.upd_diag[j], ROOT_UPD);
      take(p.diag[j], ROOT_DIAG);
      take(p.upd[j], ROOT_UPD);
      const size_t before = order.size();
      take(p.trsm[j], ROOT_TRSM);
      for (size_t q = before; q < order.size(); ++q) order[q].pad = row_first[foff[order[q].blk & 0xffffff] + order[q].ti];
   }
   for (int b = 0; b < nblk; ++b)
      for (int ti = 0; ti < blks[b].ntr; ++ti)
         for (int tj = 0; tj < blks[b].ntc; ++tj) { int& pr = init[foff[b] + (long long)ti * blks[b].ntc + tj]; if (pr < 0) pr = tj; }
   // eight lists: runs of tasks of one (block, tile row) go to the lists round-robin, every list keeps the order
   std::vector<std::vector<TileTask>> lists(8);
   int run = -1, last_b = -2, last_i = -2;
   for (const TileTask& t : order) {
      const int b = t.blk & 0xffffff;
      if (b != last_b || t.ti != last_i) { ++run; last_b = b; last_i = t.ti; }
      lists[run & 7].push_back(t);
   }
   for (int x = 0; x < 8; ++x) { xoff[x] = (int)tasks.size(); tasks.insert(tasks.end(), lists[x].begin(), lists[x].end()); }
   xoff[8] = n_tasks = (int)tasks.size();
}

}  // namespace pips
