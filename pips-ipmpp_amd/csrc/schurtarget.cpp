// Position tables of the leaf handles' sparse Schur entries (schurtarget.h): clique pair (la >= lb) of a block's non-empty border
// columns bm -> the caller's position of (bm[lb], bm[la]) in an upper pattern, of (bm[la], bm[lb]) in a lower one, by a binary search in
// the row; the distinct positions of all blocks, ascending, are the device's compact value array.
#include "schurtarget.h"

#include <algorithm>
#include <climits>

#include "layout.h"

namespace pips {

namespace {
struct Fnv {
   uint64_t h = 1469598103934665603ULL;
   void mix(uint64_t v) {
      for (int k = 0; k < 8; ++k) { h ^= (v >> (8 * k)) & 0xff; h *= 1099511628211ULL; }
   }
};
}  // namespace

int build_schur_target(int nblk, int S, const int* const* bt_rowptr, const int* sc_rowptr, const int* sc_colidx, int lower, SchurTarget* out,
                       SchurPatternId& id) {
   if (nblk <= 0 || S <= 0 || !bt_rowptr || !sc_rowptr || !sc_colidx) PIPS_FAIL(PIPS_ERR_ARG, "sparse Schur target: bad arguments");
   const long long nnz = sc_rowptr[S];
   if (sc_rowptr[0] != 0 || nnz < 0) PIPS_FAIL(PIPS_ERR_ARG, "sparse Schur target: the pattern's row pointers run from %d to %lld", sc_rowptr[0], nnz);
   lower = lower != 0;
   // the blocks' column sets, by the one rule of the packed solves and the sparse root (schur_pack_block)
   std::vector<int> local((size_t)S), nb((size_t)nblk, 0), cols;
   std::vector<long long> coff((size_t)nblk + 1, 0);
   std::vector<char> used((size_t)S, 0);
   for (int b = 0; b < nblk; ++b) {
      nb[b] = schur_pack_block(S, bt_rowptr[b], local.data());
      for (int s = 0; s < S; ++s)
         if (local[s] >= 0) { cols.push_back(s); used[s] = 1; }
      coff[b + 1] = (long long)cols.size();
   }
   // the consulted rows: checked, and hashed for the calls to come
   Fnv f;
   f.mix((uint64_t)S); f.mix((uint64_t)lower); f.mix((uint64_t)nnz);
   for (int r = 0; r < S; ++r) {
      if (!used[r]) continue;
      const long long a = sc_rowptr[r], e = sc_rowptr[r + 1];
      if (a < 0 || e < a || e > nnz) PIPS_FAIL(PIPS_ERR_ARG, "sparse Schur target: row %d of the pattern runs from %lld to %lld of %lld entries", r, a, e, nnz);
      f.mix((uint64_t)r); f.mix((uint64_t)a); f.mix((uint64_t)e);
      int prev = -1;
      for (long long p = a; p < e; ++p) {
         const int c = sc_colidx[p];
         if (c < 0 || c >= S) PIPS_FAIL(PIPS_ERR_ARG, "sparse Schur target: column index %d in row %d of the pattern is outside 0 .. %d", c, r, S - 1);
         if (c <= prev) PIPS_FAIL(PIPS_ERR_ARG, "sparse Schur target: row %d of the pattern does not ascend (column %d after %d)", r, c, prev);
         prev = c;
         f.mix((uint64_t)c);
      }
   }
   id.S = S; id.lower = lower; id.nnz = nnz; id.hash = f.h;
   if (!out) return PIPS_OK;

   *out = SchurTarget();
   out->nb = nb;
   out->off.assign((size_t)nblk + 1, 0);
   for (int b = 0; b < nblk; ++b) out->off[b + 1] = out->off[b] + (long long)nb[b] * nb[b];
   std::vector<long long> where((size_t)out->off[nblk], 0);   // per table entry: the caller's position
   for (int b = 0; b < nblk; ++b) {
      const int* bm = cols.data() + coff[b];
      const int n = nb[b];
      for (int la = 0; la < n; ++la)
         for (int lb = 0; lb <= la; ++lb) {
            const int row = lower ? bm[la] : bm[lb], col = lower ? bm[lb] : bm[la];
            const int* b0 = sc_colidx + sc_rowptr[row];
            const int* b1 = sc_colidx + sc_rowptr[row + 1];
            const int* it = std::lower_bound(b0, b1, col);
            if (it == b1 || *it != col)
               PIPS_FAIL(PIPS_ERR_STATE, "sparse Schur target: the pattern has no entry (%d, %d) for the border columns %d and %d of block %d (%s triangle)",
                         row, col, bm[lb], bm[la], b, lower ? "lower" : "upper");
            const long long p = (long long)(it - sc_colidx);
            where[(size_t)(out->off[b] + (long long)la * n + lb)] = p;
            out->pos.push_back(p);
         }
   }
   std::sort(out->pos.begin(), out->pos.end());
   out->pos.erase(std::unique(out->pos.begin(), out->pos.end()), out->pos.end());
   if ((long long)out->pos.size() > (long long)INT_MAX) PIPS_FAIL(PIPS_ERR_STATE, "sparse Schur target: %zu touched positions exceed the tables' 2^31", out->pos.size());
   out->tab.assign(where.size(), 0);
   for (int b = 0; b < nblk; ++b) {
      const int n = nb[b];
      for (int la = 0; la < n; ++la)
         for (int lb = 0; lb <= la; ++lb) {
            const size_t q = (size_t)(out->off[b] + (long long)la * n + lb);
            out->tab[q] = (int)(std::lower_bound(out->pos.begin(), out->pos.end(), where[q]) - out->pos.begin());
         }
   }
   return PIPS_OK;
}

}  // namespace pips

// ---- the builder without a device, as the two entries call it
extern "C" int pips_schur_target_probe(int nblk, int S, const int* const* bt_rowptr, const int* sc_rowptr, const int* sc_colidx, int lower, int* nb,
                                       long long* n_touched, long long* pos, long long cap, int* const* tab) {
   if (!nb || !n_touched) PIPS_FAIL(pips::PIPS_ERR_ARG, "pips_schur_target_probe: bad arguments");
   pips::SchurTarget t;
   pips::SchurPatternId id;
   if (int rc = pips::build_schur_target(nblk, S, bt_rowptr, sc_rowptr, sc_colidx, lower, &t, id)) return rc;
   std::copy(t.nb.begin(), t.nb.end(), nb);
   *n_touched = (long long)t.pos.size();
   if (pos && cap >= *n_touched) std::copy(t.pos.begin(), t.pos.end(), pos);
   for (int b = 0; tab && b < nblk; ++b)
      if (tab[b]) std::copy(t.tab.begin() + t.off[b], t.tab.begin() + t.off[b + 1], tab[b]);
   return pips::PIPS_OK;
}
