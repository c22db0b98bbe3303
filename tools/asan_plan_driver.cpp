// ASAN/UBSAN driver for the host task plans of the tiled LDL^T (csrc/tileplan.cpp): block descriptors and envelopes made by hand - no
// symbolic analysis - through every planner, and the rules the drivers and kernels rely on checked on what comes out.  The shapes are the
// smallest at which each rule can break: leaf batches around the group size of four tile columns with and without border rows, full and
// banded envelopes, a mixed batch with a block without a tail and one without a border; dense roots around the panel and lookahead
// thresholds of DenseLdl::init.
#include <algorithm>
#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "tileplan.h"
using namespace pips;

namespace {

struct Batch {
   std::string name;
   std::vector<BlkDesc> blks;
   std::vector<std::vector<int>> first;   // per block and tile row (ntr entries): first tile column of the row's envelope
   TileFirst ptrs() const {
      TileFirst p;
      for (auto& f : first) p.push_back(&f);
      return p;
   }
   // the first tile column whose product L(ti, k) L(tj, k)^T is not zero by structure
   int lo(int b, int ti, int tj) const { return std::max(first[b][ti], first[b][tj]); }
   bool inside(int b, int ti, int tj) const { return tj >= first[b][ti]; }
};

#define CHECK(cond, ...)                                 \
   do {                                                  \
      if (!(cond)) {                                     \
         printf("%s: %s: ", s.name.c_str(), what);       \
         printf(__VA_ARGS__);                            \
         printf("\n");                                   \
         return false;                                   \
      }                                                  \
   } while (0)

BlkDesc block(int ntc, int border) {
   BlkDesc d{};
   d.ntc = ntc; d.ntr = ntc + border;
   d.m_pad = ntc * TILE; d.m = std::max(0, d.m_pad - 3);
   d.nb_pad = border * TILE; d.nb = std::max(0, d.nb_pad - 5);
   d.ldT = d.m_pad + d.nb_pad;
   return d;
}
Batch batch(const std::string& name, const std::vector<BlkDesc>& blks, bool banded) {
   Batch s{name + (banded ? ", banded" : ", full"), blks, {}};
   for (const BlkDesc& d : blks) {
      std::vector<int> f(d.ntr, 0);
      for (int t = 0; t < d.ntr && banded; ++t) f[t] = std::max(0, t - 2);
      s.first.push_back(f);
   }
   return s;
}

bool same(const TileTask& a, const TileTask& b) { return a.blk == b.blk && a.ti == b.ti && a.tj == b.tj && a.pad == b.pad; }
bool in_range(const TaskList& l, size_t n) { return l.off >= 0 && l.cnt >= 0 && (size_t)(l.off + l.cnt) <= n; }
long long tile_key(const TileTask& t) { return ((((long long)(t.blk & 0xffffff) << 20) + t.ti) << 20) + t.tj; }

// a list against the tasks it has to hold, in their order
bool list_is(const Batch& s, const char* what, const std::vector<TileTask>& tasks, const TaskList& l, const std::vector<TileTask>& want) {
   CHECK(in_range(l, tasks.size()), "list [%lld, +%d) outside %zu tasks", l.off, l.cnt, tasks.size());
   CHECK(l.cnt == (int)want.size(), "%d tasks, %zu expected", l.cnt, want.size());
   for (int q = 0; q < l.cnt; ++q) {
      const TileTask& t = tasks[l.off + q];
      CHECK(same(t, want[q]), "task %d is (%d, %d, %d, %d), expected (%d, %d, %d, %d)", q, t.blk, t.ti, t.tj, t.pad, want[q].blk, want[q].ti, want[q].tj, want[q].pad);
   }
   return true;
}

// The updates of every tile in the order they run: their K ranges [k0, k1) adjacent and ascending from the tile's first non-zero product
// to its tile column, no update of a tile outside the envelope
struct Cover {
   const Batch& s;
   const char* what;
   std::map<long long, int> next;
   bool add(const TileTask& t) {
      const int nblk = (int)s.blks.size(), k0 = t.pad & 0xffff, k1 = t.pad >> 16;
      CHECK(t.blk >= 0 && t.blk < nblk, "update of block %d", t.blk);
      const BlkDesc& d = s.blks[t.blk];
      CHECK(t.tj >= 1 && t.tj < d.ntc && t.ti >= t.tj && t.ti < d.ntr, "update of tile (%d, %d) of block %d", t.ti, t.tj, t.blk);
      CHECK(s.inside(t.blk, t.ti, t.tj), "update of tile (%d, %d) of block %d outside the envelope", t.ti, t.tj, t.blk);
      auto it = next.find(tile_key(t));
      const int at = it == next.end() ? s.lo(t.blk, t.ti, t.tj) : it->second;
      CHECK(k0 == at && k1 > k0 && k1 <= t.tj, "tile (%d, %d) of block %d takes [%d, %d) at %d", t.ti, t.tj, t.blk, k0, k1, at);
      next[tile_key(t)] = k1;
      return true;
   }
   bool complete() const {
      size_t n = 0;
      for (int b = 0; b < (int)s.blks.size(); ++b)
         for (int tj = 1; tj < s.blks[b].ntc; ++tj)
            for (int ti = tj; ti < s.blks[b].ntr; ++ti) {
               if (!s.inside(b, ti, tj) || s.lo(b, ti, tj) >= tj) continue;
               auto it = next.find(tile_key({b, ti, tj, 0}));
               CHECK(it != next.end() && it->second == tj, "tile (%d, %d) of block %d ends at %d", ti, tj, b, it == next.end() ? -1 : it->second);
               ++n;
            }
      CHECK(n == next.size(), "%zu tiles updated, %zu expected", next.size(), n);
      return true;
   }
};
template <class F> bool each(const std::vector<TileTask>& tasks, const TaskList& l, F&& f) {
   if (!in_range(l, tasks.size())) return false;
   for (long long q = l.off; q < l.off + l.cnt; ++q)
      if (!f(tasks[q])) return false;
   return true;
}

// what both column plans promise: coverage of every tile in the launch order of tail_columns, diagonal tiles, trsm, the two sweeps, the SYRK
bool check_columns(const Batch& s, const ColumnPlan& p, bool leaf) {
   const char* what = leaf ? "leaf column plan" : "root panel plan";
   const int nblk = (int)s.blks.size();
   int ntc_max = 0;
   for (const BlkDesc& d : s.blks) ntc_max = std::max(ntc_max, d.ntc);
   CHECK(p.ntc_max == ntc_max, "ntc_max %d, expected %d", p.ntc_max, ntc_max);
   for (const std::vector<TaskList>* l : {&p.upd, &p.upd_diag, &p.diag, &p.trsm, &p.fwd, &p.bwd, &p.trail, &p.trail_next})
      CHECK((int)l->size() == ntc_max, "%zu lists for %d tile columns", l->size(), ntc_max);
   Cover cover{s, what, {}};
   auto add = [&](const TileTask& t) { return cover.add(t); };
   for (int j = 0; j < ntc_max; ++j) {
      CHECK(leaf ? p.trail[j].cnt == 0 && p.trail_next[j].cnt == 0 : p.upd_diag[j].cnt == 0, "column %d has a list of the other plan", j);
      for (const TaskList* l : {&p.upd_diag[j], &p.upd[j], &p.trail_next[j], &p.trail[j]})
         if (!each(p.h_tasks, *l, add)) { printf("%s: %s: column %d\n", s.name.c_str(), what, j); return false; }
      std::vector<TileTask> diag, trsm, fwd, bwd;
      for (int b = 0; b < nblk; ++b) {
         const BlkDesc& d = s.blks[b];
         if (j >= d.ntc) continue;
         diag.push_back({b, j, j, 0});
         for (int ti = j + 1; ti < d.ntr; ++ti)
            if (s.inside(b, ti, j)) trsm.push_back({b, ti, j, 0});
         // forward sweep, step j: x_j is finished by its diagonal tile; the tail rows below that hold a tile L(ti, j - 1) take x_{j-1}
         fwd.push_back({b, j, j, 0});
         for (int ti = j + 1; ti < d.ntc && j >= 1; ++ti)
            if (s.inside(b, ti, j - 1)) fwd.push_back({b, ti, j, 0});
         // backward sweep, step j: the rows tj <= j that tile row j + 1 of the tail reaches take x_{j+1}, then row j its diagonal tile
         for (int tj = 0; tj < j && j + 1 < d.ntc; ++tj)
            if (s.inside(b, j + 1, tj)) bwd.push_back({b, tj, j, 0});
         bwd.push_back({b, j, j, 0});
      }
      if (!list_is(s, "diag", p.h_tasks, p.diag[j], diag) || !list_is(s, "trsm", p.h_tasks, p.trsm[j], trsm)) return false;
      if (!list_is(s, "fwd", p.h_tasks, p.fwd[j], fwd) || !list_is(s, "bwd", p.h_tasks, p.bwd[j], bwd)) return false;
   }
   if (!cover.complete()) return false;
   std::map<long long, int> seen;
   long long want = 0;
   for (const BlkDesc& d : s.blks)
      if (d.ntc > 0 && d.nb > 0) want += (long long)(d.nb_pad / TILE) * (d.nb_pad / TILE + 1) / 2;
   CHECK(in_range(p.schur, p.h_tasks.size()) && p.schur.cnt == want, "schur holds %d tasks, %lld expected", p.schur.cnt, want);
   for (long long q = p.schur.off; q < p.schur.off + p.schur.cnt; ++q) {
      const TileTask& t = p.h_tasks[q];
      CHECK(t.blk >= 0 && t.blk < nblk && s.blks[t.blk].ntc > 0 && s.blks[t.blk].nb > 0, "schur task of block %d", t.blk);
      CHECK(t.tj >= 0 && t.tj <= t.ti && t.ti < s.blks[t.blk].nb_pad / TILE && t.pad == 0, "schur task (%d, %d) of block %d", t.ti, t.tj, t.blk);
      CHECK(++seen[tile_key(t)] == 1, "schur tile (%d, %d) of block %d twice", t.ti, t.tj, t.blk);
   }
   return true;
}

// the update and trsm tasks of a leaf column plan, tagged (kind 0 update, 1 trsm), counted
using Tagged = std::tuple<int, int, int, int, int>;
std::map<Tagged, int> column_tasks(const ColumnPlan& p) {
   std::map<Tagged, int> m;
   for (int j = 0; j < p.ntc_max; ++j) {
      for (const TaskList* l : {&p.upd_diag[j], &p.upd[j]})
         each(p.h_tasks, *l, [&](const TileTask& t) { ++m[{0, t.blk, t.ti, t.tj, t.pad}]; return true; });
      each(p.h_tasks, p.trsm[j], [&](const TileTask& t) { ++m[{1, t.blk, t.ti, t.tj, 0}]; return true; });
   }
   return m;
}

// the regrouping by groups of P tile columns: every task of the column plan once, every tile's updates still in order (in the order
// tail_panels launches the lists), a strip one tile row below the group in column order, a group's strips by block and tile row
bool check_groups(const Batch& s, const ColumnPlan& p, const GroupPlan& g, int P) {
   const char* what = "group plan";
   CHECK(g.P == P && g.n_groups == (p.ntc_max + P - 1) / P, "%d groups of %d columns", g.n_groups, g.P);
   CHECK((int)g.deep.size() == g.n_groups && (int)g.pre.size() == g.n_groups && (int)g.block_deep.size() == g.n_groups && (int)g.strips.size() == g.n_groups &&
            (int)g.upd_in.size() == p.ntc_max && (int)g.trsm_in.size() == p.ntc_max, "list counts");
   std::map<Tagged, int> left = column_tasks(p);
   Cover cover{s, what, {}};
   auto update = [&](const TileTask& t) { --left[{0, t.blk, t.ti, t.tj, t.pad}]; return cover.add(t); };
   auto trsm = [&](const TileTask& t) { --left[{1, t.blk, t.ti, t.tj, 0}]; return t.pad == 0; };
   for (int i = 0; i < g.n_groups; ++i) {
      bool ok = each(g.h_tasks, g.pre[i], update) && each(g.h_tasks, g.block_deep[i], update);
      for (int j = i * P; ok && j < std::min((i + 1) * P, p.ntc_max); ++j) ok = each(g.h_tasks, g.upd_in[j], update) && each(g.h_tasks, g.trsm_in[j], trsm);
      ok = ok && each(g.h_tasks, g.deep[i], update);
      CHECK(ok, "group %d", i);
      const TaskList& sl = g.strips[i];
      CHECK(sl.off >= 0 && sl.cnt >= 0 && (size_t)(sl.off + sl.cnt) <= g.h_strips.size(), "strips of group %d outside the array", i);
      std::pair<int, int> before{-1, -1};
      for (long long q = sl.off; q < sl.off + sl.cnt; ++q) {
         const TileStrip& st = g.h_strips[q];
         CHECK(st.cnt > 0 && st.off >= 0 && (size_t)(st.off + st.cnt) <= g.h_tasks.size(), "strip %lld outside the tasks", q);
         const TileTask& t0 = g.h_tasks[st.off];
         CHECK(t0.ti >= (i + 1) * P && std::make_pair(t0.blk, t0.ti) > before, "strip of row %d of block %d in group %d", t0.ti, t0.blk, i);
         before = {t0.blk, t0.ti};
         int step = -1;
         for (int k = 0; k < st.cnt; ++k) {
            const TileTask& t = g.h_tasks[st.off + k];
            // column order: trsm(ti, c) after the update of (ti, c), which ends at K = c, and before the update of (ti, c + 1)
            const int at = t.pad ? 2 * t.tj : 2 * t.tj + 1;
            CHECK(t.blk == t0.blk && t.ti == t0.ti && at > step && t.tj >= i * P && t.tj < (i + 1) * P, "strip of row %d of block %d: task %d", t0.ti, t0.blk, k);
            CHECK(t.pad ? update(t) : trsm(t), "strip of row %d of block %d: task %d", t0.ti, t0.blk, k);
            step = at;
         }
      }
   }
   for (auto& kv : left) CHECK(kv.second == 0, "a task of tile (%d, %d) of block %d is held %d times", std::get<2>(kv.first), std::get<3>(kv.first), std::get<1>(kv.first), 1 - kv.second);
   return cover.complete();
}

bool check_sweep(const Batch& s, const SweepLists& l, bool with_first) {
   const char* what = "sweep lists";
   const int nblk = (int)s.blks.size();
   std::vector<TileTask> want;
   for (int i = 0; i < 1 << 20; ++i) {
      const size_t before = want.size();
      for (int b = 0; b < nblk; ++b)
         if (i < s.blks[b].ntc) want.push_back({b, i, 0, 0});
      if (want.size() == before) break;
   }
   if (!list_is(s, what, l.tasks, TaskList{0, (int)l.tasks.size()}, want)) return false;
   CHECK((int)l.flag_off.size() == nblk && (int)l.tfirst_off.size() == nblk, "offsets for %zu blocks", l.flag_off.size());
   long long nf = 0, nt = 0;
   for (int b = 0; b < nblk; ++b) {
      const BlkDesc& d = s.blks[b];
      CHECK(l.flag_off[b] == nf && l.tfirst_off[b] == nt, "offsets of block %d", b);
      nf += d.ntc;
      if (!with_first) continue;
      CHECK((size_t)(nt + d.ntr) <= l.tfirst.size(), "tfirst of block %d", b);
      for (int i = 0; i < d.ntr; ++i) CHECK(l.tfirst[nt + i] == (i < d.ntc ? std::min(i, s.first[b][i]) : s.first[b][i]), "tfirst of row %d of block %d", i, b);
      nt += d.ntr;
   }
   CHECK(l.n_flags == nf && (long long)l.tfirst.size() == nt, "%lld flags, %zu row starts", l.n_flags, l.tfirst.size());
   return true;
}

bool check_single(const Batch& s, const ColumnPlan& p, const TailSingleLists& l) {
   const char* what = "single-launch lists";
   const int nblk = (int)s.blks.size();
   // the driver's order (tail_columns), kind in bits 24 and up; a trsm's pad: the first tile column in which its row has a trsm
   std::map<long long, int> row_first;
   for (int j = 0; j < p.ntc_max; ++j)
      each(p.h_tasks, p.trsm[j], [&](const TileTask& t) { auto it = row_first.emplace(tile_key({t.blk, t.ti, 0, 0}), t.tj).first; it->second = std::min(it->second, t.tj); return true; });
   std::vector<TileTask> order;
   std::map<long long, int> first_k0;
   for (int j = 0; j < p.ntc_max; ++j) {
      auto take = [&](const TaskList& tl, int kind) {
         each(p.h_tasks, tl, [&](TileTask t) {
            if (kind == ROOT_UPD) first_k0.emplace(tile_key(t), t.pad & 0xffff);
            t.pad = kind == ROOT_UPD ? t.pad : kind == ROOT_TRSM ? row_first[tile_key({t.blk, t.ti, 0, 0})] : 0;
            t.blk |= kind << 24;
            order.push_back(t);
            return true;
         });
      };
      take(p.upd_diag[j], ROOT_UPD); take(p.diag[j], ROOT_DIAG); take(p.upd[j], ROOT_UPD); take(p.trsm[j], ROOT_TRSM);
   }
   CHECK(l.n_tasks == (int)order.size() && l.tasks.size() == order.size() && l.xoff[0] == 0 && l.xoff[8] == l.n_tasks, "%d tasks, %zu expected", l.n_tasks, order.size());
   for (int x = 0; x < 8; ++x) CHECK(l.xoff[x] <= l.xoff[x + 1], "list %d has a negative length", x);
   // each list is a subsequence of the driver's order, all of them together the whole of it, a run of one (block, tile row) in one list
   std::vector<int> at(8), list_of(order.size(), -1);
   for (int x = 0; x < 8; ++x) at[x] = l.xoff[x];
   int last_list = -1;
   for (size_t q = 0; q < order.size(); ++q) {
      int x = 0;
      while (x < 8 && !(at[x] < l.xoff[x + 1] && same(l.tasks[at[x]], order[q]))) ++x;
      CHECK(x < 8, "task %zu of the driver's order heads no list", q);
      const bool run = q > 0 && (order[q].blk & 0xffffff) == (order[q - 1].blk & 0xffffff) && order[q].ti == order[q - 1].ti;
      CHECK(!run || x == last_list, "the run of row %d of block %d is split", order[q].ti, order[q].blk & 0xffffff);
      ++at[x];
      last_list = x;
   }
   // the flags and their template
   CHECK((int)l.foff.size() == nblk + 1 && l.foff[0] == 0, "flag offsets");
   for (int b = 0; b < nblk; ++b) CHECK(l.foff[b + 1] - l.foff[b] == (long long)s.blks[b].ntr * s.blks[b].ntc + s.blks[b].ntr + s.blks[b].ntc, "flags of block %d", b);
   CHECK(l.n_flags == l.foff[nblk] && (long long)l.init.size() == std::max<long long>(l.n_flags, 1), "%lld flags, template of %zu", l.n_flags, l.init.size());
   for (int b = 0; b < nblk; ++b) {
      const BlkDesc& d = s.blks[b];
      for (int ti = 0; ti < d.ntr; ++ti)
         for (int tj = 0; tj < d.ntc; ++tj) {
            auto it = first_k0.find(tile_key({b, ti, tj, 0}));
            const int want = it == first_k0.end() ? tj : it->second;
            CHECK(l.init[l.foff[b] + (long long)ti * d.ntc + tj] == want, "template of tile (%d, %d) of block %d", ti, tj, b);
         }
      for (long long q = l.foff[b] + (long long)d.ntr * d.ntc; q < l.foff[b + 1]; ++q) CHECK(l.init[q] == 0, "template of the row and column flags of block %d", b);
   }
   return true;
}

bool run_leaf(const Batch& s) {
   const int P = 4;
   const TileFirst first = s.ptrs();
   ColumnPlan p;
   p.build_leaf(s.blks, first, P);
   GroupPlan g;
   g.build(p, P);
   SweepLists sw;
   sw.build(s.blks, &first);
   TailSingleLists ts;
   ts.build(p, s.blks);
   return check_columns(s, p, true) && check_groups(s, p, g, P) && check_sweep(s, sw, true) && check_single(s, p, ts);
}

bool run_root(int ntc, int panel, bool lookahead) {
   const Batch s = batch("root of " + std::to_string(ntc) + " tile columns, panel " + std::to_string(panel) + (lookahead ? ", lookahead" : ""), {block(ntc, 0)}, false);
   ColumnPlan p;
   p.build_root(s.blks, panel, lookahead);
   SweepLists sw;
   sw.build(s.blks, nullptr);
   return check_columns(s, p, false) && check_sweep(s, sw, false);
}

}  // namespace

int main() {
   int n_leaf = 0, n_root = 0;
   for (int banded = 0; banded < 2; ++banded) {
      for (int ntc : {1, 2, 3, 4, 5, 8, 9})
         for (int border : {0, 1, 3}) {
            if (!run_leaf(batch("leaf of " + std::to_string(ntc) + " tile columns and " + std::to_string(border) + " border rows", {block(ntc, border)}, banded))) return 1;
            ++n_leaf;
         }
      // four blocks of different sizes, one without a tail, one without a border
      if (!run_leaf(batch("mixed batch", {block(5, 2), block(0, 1), block(9, 0), block(2, 3)}, banded))) return 1;
      ++n_leaf;
   }
   for (int ntc : {1, 2, 3})
      for (int panel : {1, 2})
         for (int lookahead = 0; lookahead < 2; ++lookahead, ++n_root)
            if (!run_root(ntc, panel, lookahead)) return 1;
   for (int ntc : {47, 48, 49, 64, 65}) {   // the rules of DenseLdl::init
      if (!run_root(ntc, ntc <= 64 ? 1 : 2, ntc >= 48)) return 1;
      ++n_root;
   }
   printf("planned %d leaf batches and %d dense roots under ASAN/UBSAN\n", n_leaf, n_root);
   return 0;
}
