// Host pass of an IPM handle's creation: see ipmlayout.h.
#include "ipmlayout.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#define TRY(expr)                \
   do {                          \
      int _rc = (expr);          \
      if (_rc) return _rc;       \
   } while (0)

namespace pips {

int check_ipm_input(const IpmInput& in, int rank, int n_ranks, const char* who) {
   if (in.n_blocks < 2 || !in.blocks || in.myl < 0 || in.mzl < 0 || n_ranks < 1 || rank < 0 || rank >= n_ranks || (in.myl > 0 && !in.bL) ||
       (in.mzl > 0 && (!in.dlow || !in.dupp || !in.idlow || !in.idupp)))
      PIPS_FAIL(PIPS_ERR_ARG, "%s: bad arguments", who);
   return PIPS_OK;
}

// ---- dimensions and offsets ------------------------------------------------------------------------------------------------------
// Root inequality rows C0 x0 - s = ...: the reference eliminates them from the root system (-C0^T Omega^-1 C0 on the x0 block,
// sLinsysRootAug.C:1276-1294) and leaves the rest to dsytrf's Bunch-Kaufman pivoting.  So does the harness on the dense root, which
// pivots (k_tile_diag_bk; pips_hip_kkt_set_root_inequalities switches it on): an active row has Omega^-1 ~ 1e14, the x0 block is
// then a huge low-rank matrix plus an O(1) rest and a static pivot order reports the cancelled pivots as perturbed at every
// regularisation (2 % of the seeded general LPs ended with status 3 that way while the rows were eliminated under a static order).
// eliminate_z0 = false keeps the rows in the root system as rows of the linking-inequality kind - diagonal nOmegaInv, no
// cancellation: the sparse root, whose factorisation is the leaf engine's (static order), and PIPS_IPM_ROOT_INEQ_ELIMINATE=0.
int ipm_dims(const IpmInput& in, bool eliminate_z0, IpmLayout& L) {
   const pips_ipm_block& root = in.blocks[0];
   const int N = in.n_blocks - 1;
   L.N = N; L.n0 = root.n; L.my0 = root.my; L.mz0 = root.mz; L.myl = in.myl; L.mzl = in.mzl;
   L.ry = L.my0 + L.myl; L.rzr = L.mz0 + L.mzl;
   L.xoff.assign(N + 2, 0); L.yoff.assign(N + 2, 0); L.zoff.assign(N + 2, 0); L.koff.assign(N + 2, 0);
   L.xoff[1] = L.n0; L.yoff[1] = L.ry; L.zoff[1] = L.rzr;
   for (int i = 1; i <= N; ++i) {
      const pips_ipm_block& b = in.blocks[i];
      if (b.n < 0 || b.my < 0 || b.mz < 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_general: negative block dimension");
      L.xoff[i + 1] = L.xoff[i] + b.n; L.yoff[i + 1] = L.yoff[i] + b.my; L.zoff[i + 1] = L.zoff[i] + b.mz;
      L.koff[i + 1] = L.koff[i] + b.n + b.my + b.mz;
   }
   L.nx = L.xoff[N + 1]; L.my = L.yoff[N + 1]; L.mz = L.zoff[N + 1]; L.nleaf = L.koff[N + 1];
   L.ncp = 2LL * L.mz + 2LL * L.nx; L.nxyz = (long long)L.nx + L.my + L.mz;
   L.NP = L.nx + L.mz + L.ncp; L.ND = L.my + L.mz + L.ncp;
   L.e_mz0 = eliminate_z0 ? L.mz0 : 0;
   L.e_mzl = eliminate_z0 ? L.mzl : L.mz0 + L.mzl;
   L.S = L.n0 + L.my0 + L.myl + L.e_mzl;
   return PIPS_OK;
}

// ---- Hessians (pips_ipm_create_qp) -----------------------------------------------------------------------------------------------
// A negative diagonal entry cannot belong to a positive semidefinite matrix: a cheap necessary test, no full one - convexity is the
// caller's contract.
static int check_hessian(int i, int n, const pips_csr_view& q, LowerQ& out) {
   out.have = false;
   if (!q.rowptr) return PIPS_OK;
   if (q.rows != n || q.cols != n) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp: Q[%d] is %d x %d but block %d has %d variables", i, q.rows, q.cols, i, n);
   if (n > 0 && q.rowptr[n] > q.rowptr[0] && (!q.colidx || !q.val)) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp: Q[%d] lacks colidx / val", i);
   out.have = true;
   out.rp.assign((size_t)n + 1, 0);
   std::vector<std::pair<int, double>> row;
   for (int r = 0; r < n; ++r) {
      row.clear();
      for (int q_ = q.rowptr[r]; q_ < q.rowptr[r + 1]; ++q_) {
         const int c = q.colidx[q_];
         if (c < 0 || c >= n) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp: Q[%d] row %d has column index %d outside [0, %d)", i, r, c, n);
         if (c > r) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp: Q[%d] has entry (%d, %d) above the diagonal - lower-triangular storage expected", i, r, c);
         row.push_back({c, q.val[q_]});
      }
      std::stable_sort(row.begin(), row.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
      for (size_t k = 0; k < row.size(); ++k) {
         if (!out.ci.empty() && (int)out.ci.size() > out.rp[r] && out.ci.back() == row[k].first) out.v.back() += row[k].second;
         else { out.ci.push_back(row[k].first); out.v.push_back(row[k].second); }
      }
      out.rp[r + 1] = (int)out.ci.size();
      if (out.rp[r + 1] > out.rp[r] && out.ci.back() == r && out.v.back() < 0.0)
         PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp: Q[%d] has the negative diagonal entry %g in row %d - not positive semidefinite", i, out.v.back(), r);
   }
   out.ci.push_back(0); out.v.push_back(0.0);   // never empty arrays
   return PIPS_OK;
}

// R_i, the cross Hessian of block i >= 1 with x0 (pips_ipm_create_qp_cross): general CSR, n_i x n0.  One without a stored entry counts
// as absent.
static int check_cross(int i, int n, int n0, const pips_csr_view& r, CrossR& out) {
   out.have = false;
   if (!r.rowptr) return PIPS_OK;
   if (i == 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp_cross: R[0] is present - the root has no cross Hessian with itself (Q[0] holds its Hessian)");
   if (r.rows != n || r.cols != n0)   // (before rowptr[rows] is read)
      PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp_cross: R[%d] is %d x %d but block %d has %d variables and the root %d", i, r.rows, r.cols, i, n, n0);
   const bool stored = n > 0 && r.rowptr[n] > r.rowptr[0];
   if (n0 == 0 && stored) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp_cross: R[%d] has stored entries but n0 == 0 - there is no x0 to couple with", i);
   if (!stored) return PIPS_OK;
   if (!r.colidx || !r.val) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp_cross: R[%d] lacks colidx / val", i);
   out.have = true;
   out.rp.assign((size_t)n + 1, 0);
   std::vector<std::pair<int, double>> row;
   for (int k = 0; k < n; ++k) {
      row.clear();
      for (int q = r.rowptr[k]; q < r.rowptr[k + 1]; ++q) {
         const int c = r.colidx[q];
         if (c < 0 || c >= n0) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_qp_cross: R[%d] row %d has column index %d outside [0, %d)", i, k, c, n0);
         row.push_back({c, r.val[q]});
      }
      std::stable_sort(row.begin(), row.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
      for (size_t j = 0; j < row.size(); ++j) {
         if ((int)out.ci.size() > out.rp[k] && out.ci.back() == row[j].first) out.v.back() += row[j].second;
         else { out.ci.push_back(row[j].first); out.v.push_back(row[j].second); }
      }
      out.rp[k + 1] = (int)out.ci.size();
   }
   out.ci.push_back(0); out.v.push_back(0.0);   // never empty arrays
   return PIPS_OK;
}

int ipm_hessians(const IpmInput& in, IpmLayout& L) {
   L.hq.assign(in.n_blocks, LowerQ{});
   L.hr.assign(in.n_blocks, CrossR{});
   L.has_q = L.cross = false;
   for (int i = 0; in.Q && i < in.n_blocks; ++i) {
      TRY(check_hessian(i, in.blocks[i].n, in.Q[i], L.hq[i]));
      L.has_q = L.has_q || L.hq[i].have;
   }
   for (int i = 0; in.R && i < in.n_blocks; ++i) {
      TRY(check_cross(i, in.blocks[i].n, in.blocks[0].n, in.R[i], L.hr[i]));
      L.cross = L.cross || L.hr[i].have;
   }
   L.has_q = L.has_q || L.cross;
   return PIPS_OK;
}

// ---- rows of J = [A; C]: y rows [y0 | ylink | blocks], z rows [z0 | zlink | blocks] ------------------------------------------------
// J and J^T from the rows (sorted in place)
static void rows_to_csr(std::vector<std::vector<std::pair<int, double>>>& rows, int nx, HostCsr& h) {
   h.rp.assign(rows.size() + 1, 0);
   h.trp.assign((size_t)nx + 1, 0);
   for (size_t r = 0; r < rows.size(); ++r) {
      std::sort(rows[r].begin(), rows[r].end());
      h.rp[r + 1] = h.rp[r] + (int)rows[r].size();
      for (auto& e : rows[r]) ++h.trp[e.first + 1];
   }
   const int nnz = h.rp[rows.size()];
   h.ci.resize(nnz); h.tci.resize(nnz); h.v.resize(nnz); h.tv.resize(nnz);
   for (int j = 0; j < nx; ++j) h.trp[j + 1] += h.trp[j];
   std::vector<int> fill(h.trp.begin(), h.trp.end() - 1);
   for (size_t r = 0; r < rows.size(); ++r) {
      int q = h.rp[r];
      for (auto& e : rows[r]) {
         h.ci[q] = e.first; h.v[q] = e.second; ++q;
         const int t = fill[e.first]++;
         h.tci[t] = (int)r; h.tv[t] = e.second;
      }
   }
}
int csr_long_rows(const std::vector<int>& rp, std::vector<int>& list) {
   list.clear();
   for (size_t r = 0; r + 1 < rp.size(); ++r)
      if (rp[r + 1] - rp[r] > CSR_LONG_ROW) list.push_back((int)r);
   list.push_back(0);   // never an empty array
   return (int)list.size() - 1;
}

void ipm_rows_J(const IpmInput& in, int rank, IpmLayout& L) {
   std::vector<std::vector<std::pair<int, double>>> rows((size_t)L.my + L.mz);
   auto add = [&](const pips_csr_view& m, int row0, int col0) {
      if (!present(view(m))) return;
      for (int r = 0; r < m.rows; ++r)
         for (int q = m.rowptr[r]; q < m.rowptr[r + 1]; ++q) rows[(size_t)row0 + r].push_back({col0 + m.colidx[q], m.val[q]});
   };
   const pips_ipm_block& root = in.blocks[0];
   // root matrices enter the local J on rank 0 only: replicated rows are summed over the ranks
   if (rank == 0) { add(root.A, 0, 0); add(root.BL, L.my0, 0); add(root.C, L.my, 0); add(root.DL, L.my + L.mz0, 0); }   // A0, F0, C0, G0
   for (int i = 1; i <= L.N; ++i) {
      const pips_ipm_block& b = in.blocks[i];
      add(b.A, L.yoff[i], 0); add(b.B, L.yoff[i], L.xoff[i]); add(b.C, L.my + L.zoff[i], 0); add(b.D, L.my + L.zoff[i], L.xoff[i]);
      add(b.BL, L.my0, L.xoff[i]); add(b.DL, L.my + L.mz0, L.xoff[i]);
   }
   rows_to_csr(rows, L.nx, L.J);
   L.J.n_long = csr_long_rows(L.J.rp, L.J.long_rows);
   L.J.n_tlong = csr_long_rows(L.J.trp, L.J.long_trows);
}

// ---- leaf systems: K_i pattern / values and border for the engine ------------------------------------------------------------------
// the size-then-fill pairs of the two assemble functions
static int leaf_assemble(int nx, int my, int mz, const LowerQ& q, const View& B, const View& D, LeafSystem& s) {
   const int nk = nx + my + mz;
   std::vector<int> empty_rp_y(my + 1, 0), empty_rp_z(mz + 1, 0), dpos(nk);
   auto call = [&](int* ci, double* v, int* dp) {
      return pips_kkt_leaf_assemble(nx, my, mz, q.have ? q.rp.data() : nullptr, q.ci.data(), q.v.data(), present(B) ? B.rp : empty_rp_y.data(), B.ci,
                                    B.v, present(D) ? D.rp : empty_rp_z.data(), D.ci, D.v, s.Krp.data(), ci, v, dp);
   };
   s.Krp.assign(nk + 1, 0);
   TRY(call(nullptr, nullptr, nullptr));
   s.Kci.assign(s.Krp[nk], 0);
   s.kvals.assign(s.Krp[nk], 0.0);
   return call(s.Kci.data(), s.kvals.data(), dpos.data());
}
// r: the block's cross Hessian R_i, whose entry (k, c) lands in Schur row c (an x0 column) at the leaf's x row k - the first block of
// the reference's BorderBiBlock {R, A, C, n_empty, F^T, G^T}
static int border_assemble(int nx, int my, int mz, const IpmLayout& L, const CrossR& r, const View& a, const View& c, const View& f, const View& g,
                           LeafSystem& s) {
   auto rp = [](const View& m) { return present(m) ? m.rp : nullptr; };
   auto call = [&](int* ci, double* v) {
      return pips_border_assemble(nx, my, mz, L.n0, L.my0, L.myl, L.e_mzl, r.have ? r.rp.data() : nullptr, r.ci.data(), r.v.data(), rp(a), a.ci, a.v,
                                  rp(c), c.ci, c.v, rp(f), f.ci, f.v, rp(g), g.ci, g.v, s.Brd.data(), ci, v);
   };
   s.Brd.assign(L.S + 1, 0);
   TRY(call(nullptr, nullptr));
   s.Bci.assign(s.Brd[L.S], 0);
   s.Bv.assign(s.Brd[L.S], 0.0);
   return call(s.Bci.data(), s.Bv.data());
}

int ipm_leaf_systems(const IpmInput& in, IpmLayout& L) {
   L.leaf.assign(L.N, LeafSystem{});
   for (int i = 1; i <= L.N; ++i) {
      const pips_ipm_block& b = in.blocks[i];
      if (b.my > 0 && !present(view(b.B))) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_general: block %d has equality rows but no B matrix", i);
      // Q_i: its off-diagonal entries are constant values of K_i; the diagonal is overwritten at every factorisation (k_leaf_diag adds qdiag)
      TRY(leaf_assemble(b.n, b.my, b.mz, L.hq[i], view(b.B), view(b.D), L.leaf[i - 1]));
      View g = view(b.DL);
      std::vector<int> g_rp;
      if (L.e_mzl != L.mzl && present(g)) {   // root inequality rows ride among the linking inequalities: no leaf part
         g_rp.assign((size_t)L.e_mzl + 1, 0);
         for (int r = 0; r <= L.mzl; ++r) g_rp[(size_t)(L.e_mzl - L.mzl) + r] = g.rp[r] - g.rp[0];
         g.ci += g.rp[0]; g.v += g.rp[0];
         g.rp = g_rp.data();
         g.rows = L.e_mzl;
      }
      TRY(border_assemble(b.n, b.my, b.mz, L, L.hr[i], view(b.A), view(b.C), view(b.BL), g, L.leaf[i - 1]));
   }
   return PIPS_OK;
}

void ipm_root_matrices(const IpmInput& in, IpmLayout& L) {
   const pips_ipm_block& root = in.blocks[0];
   L.A0 = view(root.A); L.F0 = view(root.BL); L.C0 = view(root.C); L.G0 = view(root.DL);
   if (L.e_mzl == L.mzl) return;
   // G0' = [C0; G0]
   const View C0 = L.C0, G0in = L.G0;
   L.g0_rp.assign(1, 0); L.g0_ci.clear(); L.g0_v.clear();
   for (const View* m : {&C0, &G0in}) {
      const int nr = m == &C0 ? L.mz0 : L.mzl;
      for (int r = 0; r < nr; ++r) {
         if (present(*m))
            for (int q = m->rp[r]; q < m->rp[r + 1]; ++q) { L.g0_ci.push_back(m->ci[q]); L.g0_v.push_back(m->v[q]); }
         L.g0_rp.push_back((int)L.g0_ci.size());
      }
   }
   L.g0_ci.push_back(0); L.g0_v.push_back(0.0);   // never empty arrays
   L.G0 = View{L.e_mzl, L.n0, L.g0_rp.data(), L.g0_ci.data(), L.g0_v.data()};
}

// ---- vectors in the flat layout ----------------------------------------------------------------------------------------------------
int ipm_flat_vectors(const IpmInput& in, IpmLayout& L) {
   L.c.assign(L.nx, 0.0); L.b.assign(L.my, 0.0); L.M.assign(L.ncp, 0.0); L.Bd.assign(L.ncp, 0.0);
   auto put = [&](const double* src, int n, double* dst) { if (src) for (int k = 0; k < n; ++k) dst[k] = src[k]; };
   const long long oT = 0, oU = L.mz, oV = 2LL * L.mz, oW = 2LL * L.mz + L.nx;
   for (int i = 0; i <= L.N; ++i) {
      const pips_ipm_block& b = in.blocks[i];
      const int x0 = i == 0 ? 0 : L.xoff[i], y0 = i == 0 ? 0 : L.yoff[i], z0 = i == 0 ? 0 : L.zoff[i];
      if (b.n > 0 && (!b.c || !b.ixlow || !b.ixupp || !b.xlow || !b.xupp)) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_general: block %d lacks c / bounds", i);
      put(b.c, b.n, L.c.data() + x0);
      put(b.b, b.my, L.b.data() + y0);
      put(b.ixlow, b.n, L.M.data() + oV + x0); put(b.ixupp, b.n, L.M.data() + oW + x0);
      put(b.xlow, b.n, L.Bd.data() + oV + x0); put(b.xupp, b.n, L.Bd.data() + oW + x0);
      put(b.iclow, b.mz, L.M.data() + oT + z0); put(b.icupp, b.mz, L.M.data() + oU + z0);
      put(b.clow, b.mz, L.Bd.data() + oT + z0); put(b.cupp, b.mz, L.Bd.data() + oU + z0);
   }
   put(in.bL, L.myl, L.b.data() + L.my0);
   put(in.idlow, L.mzl, L.M.data() + oT + L.mz0); put(in.idupp, L.mzl, L.M.data() + oU + L.mz0);
   put(in.dlow, L.mzl, L.Bd.data() + oT + L.mz0); put(in.dupp, L.mzl, L.Bd.data() + oU + L.mz0);
   for (long long k = 0; k < L.ncp; ++k) {
      if (L.M[k] != 0.0 && L.M[k] != 1.0) PIPS_FAIL(PIPS_ERR_ARG, "pips_ipm_create_general: bound indicators must be 0 or 1");
      L.Bd[k] *= L.M[k];   // matchesNonZeroPattern (Problem.cpp:69-79)
   }
   return PIPS_OK;
}

// every matrix entry (the root's on every rank), c, b, the bounds under their indicators (a bound without indicator array counts as
// absent), and ||Q|| (Problem.cpp:81), the cross Hessians among it
double ipm_data_norm(const IpmInput& in, const std::vector<LowerQ>& hq, const std::vector<CrossR>& hr) {
   double dn = 0.0;
   auto m = [&](const pips_csr_view& a) {
      if (present(view(a))) for (int q = a.rowptr[0]; q < a.rowptr[a.rows]; ++q) dn = std::max(dn, std::fabs(a.val[q]));
   };
   auto v = [&](const double* x, int n) { if (x) for (int k = 0; k < n; ++k) dn = std::max(dn, std::fabs(x[k])); };
   auto bound = [&](const double* x, const double* ind, int n) { if (x && ind) for (int k = 0; k < n; ++k) dn = std::max(dn, std::fabs(x[k] * ind[k])); };
   for (int i = 0; i < in.n_blocks; ++i) {
      const pips_ipm_block& b = in.blocks[i];
      m(b.A); m(b.C); m(b.BL); m(b.DL);
      if (i > 0) { m(b.B); m(b.D); }
      v(b.c, b.n); v(b.b, b.my);
      bound(b.xlow, b.ixlow, b.n); bound(b.xupp, b.ixupp, b.n); bound(b.clow, b.iclow, b.mz); bound(b.cupp, b.icupp, b.mz);
   }
   v(in.bL, in.myl); bound(in.dlow, in.idlow, in.mzl); bound(in.dupp, in.idupp, in.mzl);
   for (const LowerQ& q : hq)
      for (double x : q.v) dn = std::max(dn, std::fabs(x));
   for (const CrossR& r : hr)
      for (double x : r.v) dn = std::max(dn, std::fabs(x));
   return dn;
}

// weights that count replicated root entries once (iAmSpecial, DistributedVector.C:1293-1303)
void ipm_weights(int rank, IpmLayout& L) {
   const double wroot = rank == 0 ? 1.0 : 0.0;
   const long long oT = 0, oU = L.mz, oV = 2LL * L.mz, oW = 2LL * L.mz + L.nx;
   L.wG.assign(L.ncp, 1.0); L.wGs.assign(L.ncp, 1.0); L.wXYZ.assign(L.nxyz, 1.0);
   for (int k = 0; k < L.rzr; ++k) L.wG[oT + k] = L.wG[oU + k] = wroot;
   for (int k = 0; k < L.n0; ++k) L.wG[oV + k] = L.wG[oW + k] = wroot;
   for (long long k = 0; k < L.ncp; ++k) L.wGs[k] = L.wG[k] * ((k >= oU && k < oV) || k >= oW ? -1.0 : 1.0);
   for (int k = 0; k < L.n0; ++k) L.wXYZ[k] = wroot;
   for (int k = 0; k < L.ry; ++k) L.wXYZ[(size_t)L.nx + k] = wroot;
   for (int k = 0; k < L.rzr; ++k) L.wXYZ[(size_t)L.nx + L.my + k] = wroot;
   L.pairs = 0.0;
   for (long long k = 0; k < L.ncp; ++k) L.pairs += L.wG[k] * L.M[k];
}

// maps: KKT right-hand sides <- [x|y|z], leaf diagonal codes
void ipm_maps(IpmLayout& L) {
   const long long nx = L.nx, my = L.my;
   L.pack.clear(); L.code.clear();
   L.pack.reserve((size_t)L.S + L.e_mz0 + L.nleaf);
   L.code.reserve(L.nleaf);
   for (int k = 0; k < L.n0; ++k) L.pack.push_back(k);
   for (int k = 0; k < L.my0; ++k) L.pack.push_back(nx + k);
   for (int k = 0; k < L.e_mz0; ++k) L.pack.push_back(nx + my + k);
   for (int k = 0; k < L.myl; ++k) L.pack.push_back(nx + L.my0 + k);
   for (int k = 0; k < L.e_mzl; ++k) L.pack.push_back(nx + my + L.e_mz0 + k);   // [z0 | zlink] is contiguous in the harness' z order
   for (int i = 1; i <= L.N; ++i) {
      for (int k = L.xoff[i]; k < L.xoff[i + 1]; ++k) { L.pack.push_back(k); L.code.push_back(k); }
      for (int k = L.yoff[i]; k < L.yoff[i + 1]; ++k) { L.pack.push_back(nx + k); L.code.push_back(-1); }
      for (int k = L.zoff[i]; k < L.zoff[i + 1]; ++k) { L.pack.push_back(nx + my + k); L.code.push_back(-2 - (long long)k); }
   }
}

// Q for the device: both triangles over the flat x order, expanded once, and its diagonal.  Without any block Hessian: an empty Q
// (a rank whose own blocks have none while another rank's have).  A cross Hessian's entry (r, c) goes to (xoff[i] + r, c) and to its
// mirror, both from the one stored value: the copy stays exactly symmetric.  The x0 rows then hold an entry per coupled block variable
// and go through the long-row list like the replicated columns of J.  omit_q0: the entries of the Q0 block are left out (its diagonal
// stays in qdiag) - what the ranks != 0 hold where (Q x)_0 is summed over the ranks.
void ipm_flat_hessian(const IpmInput& in, IpmLayout& L) {
   std::vector<std::vector<std::pair<int, double>>> qrows((size_t)L.nx);
   L.qdiag.assign((size_t)L.nx, 0.0);
   for (int i = 0; i <= L.N; ++i) {
      const LowerQ& h = L.hq[i];
      if (!h.have) continue;
      const int o = i == 0 ? 0 : L.xoff[i];
      const bool omit = i == 0 && L.omit_q0;
      for (int r = 0; r < in.blocks[i].n; ++r)
         for (int q = h.rp[r]; q < h.rp[r + 1]; ++q) {
            const int c = h.ci[q];
            if (c == r) L.qdiag[(size_t)o + r] = h.v[q];
            if (omit) continue;
            qrows[(size_t)o + r].push_back({o + c, h.v[q]});
            if (c != r) qrows[(size_t)o + c].push_back({o + r, h.v[q]});
         }
   }
   for (int i = 1; i <= L.N; ++i) {
      const CrossR& h = L.hr[i];
      if (!h.have) continue;
      for (int r = 0; r < in.blocks[i].n; ++r)
         for (int q = h.rp[r]; q < h.rp[r + 1]; ++q) {
            qrows[(size_t)L.xoff[i] + r].push_back({h.ci[q], h.v[q]});
            qrows[(size_t)h.ci[q]].push_back({L.xoff[i] + r, h.v[q]});
         }
   }
   L.Q_rp.assign((size_t)L.nx + 1, 0); L.Q_ci.clear(); L.Q_v.clear();
   for (int r = 0; r < L.nx; ++r) {
      std::sort(qrows[r].begin(), qrows[r].end());
      for (auto& e : qrows[r]) { L.Q_ci.push_back(e.first); L.Q_v.push_back(e.second); }
      L.Q_rp[(size_t)r + 1] = (int)L.Q_ci.size();
   }
   L.Q_nnz = (long long)L.Q_ci.size();
   L.nQ_long = csr_long_rows(L.Q_rp, L.Q_long);
   L.Q_ci.push_back(0); L.Q_v.push_back(0.0);   // never empty arrays
}

int ipm_layout(const IpmInput& in, int rank, bool eliminate_z0, bool with_J, IpmLayout& L) {
   TRY(ipm_dims(in, eliminate_z0, L));
   TRY(ipm_hessians(in, L));
   if (with_J) ipm_rows_J(in, rank, L);
   TRY(ipm_leaf_systems(in, L));
   ipm_root_matrices(in, L);
   TRY(ipm_flat_vectors(in, L));
   L.norm = ipm_data_norm(in, L.hq, L.hr);
   ipm_weights(rank, L);
   ipm_maps(L);
   L.omit_q0 = L.cross && rank != 0;
   if (L.has_q) ipm_flat_hessian(in, L);
   return PIPS_OK;
}

// ---- scaling before assembly (pips_ipm_create_general_scaled) ----------------------------------------------------------------------
void make_scaled(const IpmInput& in, const IpmLayout& L, const double* col, const double* row, ScaledData& sd) {
   const double* re = row;
   const double* ri = row + L.my;
   sd.blk.assign(in.blocks, in.blocks + in.n_blocks);
   auto mat = [&](pips_csr_view& m, const double* rf, int c0) {   // rf: factors of the matrix' rows, c0: its first column in x
      if (!m.rowptr || m.rows <= 0) return;
      sd.keep.emplace_back((size_t)m.rowptr[m.rows], 0.0);
      std::vector<double>& v = sd.keep.back();
      for (int r = 0; r < m.rows; ++r)
         for (int q = m.rowptr[r]; q < m.rowptr[r + 1]; ++q) v[q] = (m.val[q] * col[c0 + m.colidx[q]]) * rf[r];
      m.val = v.data();
   };
   auto vec = [&](const double*& x, int n, const double* f, bool div) {
      if (!x || n <= 0) return;
      sd.keep.emplace_back(x, x + n);
      std::vector<double>& v = sd.keep.back();
      for (int k = 0; k < n; ++k) v[k] = div ? v[k] / f[k] : v[k] * f[k];
      x = v.data();
   };
   for (int i = 0; i <= L.N; ++i) {
      pips_ipm_block& b = sd.blk[i];
      const int xi = i == 0 ? 0 : L.xoff[i], yi = i == 0 ? 0 : L.yoff[i], zi = i == 0 ? 0 : L.zoff[i];
      mat(b.A, re + yi, 0);
      mat(b.C, ri + zi, 0);
      if (i > 0) { mat(b.B, re + yi, xi); mat(b.D, ri + zi, xi); }
      mat(b.BL, re + L.my0, xi);
      mat(b.DL, ri + L.mz0, xi);
      vec(b.c, b.n, col + xi, false); vec(b.xlow, b.n, col + xi, true); vec(b.xupp, b.n, col + xi, true);
      vec(b.b, b.my, re + yi, false); vec(b.clow, b.mz, ri + zi, false); vec(b.cupp, b.mz, ri + zi, false);
   }
   sd.in = in;
   sd.in.blocks = sd.blk.data();
   // Q' = Cs Q Cs on the lower triangles as given: (q col_r) col_c.  The flat symmetric copy is built from these, so it stays exactly
   // symmetric ((q col_r) col_c and (q col_c) col_r round differently)
   if (in.Q) {
      sd.q.assign(in.Q, in.Q + in.n_blocks);
      for (int i = 0; i <= L.N; ++i) {
         pips_csr_view& m = sd.q[i];
         const int n = in.blocks[i].n;
         if (!m.rowptr || n <= 0 || m.rowptr[n] <= 0 || !m.colidx || !m.val) continue;
         const double* cf = col + (i == 0 ? 0 : L.xoff[i]);
         sd.keep.emplace_back((size_t)m.rowptr[n], 0.0);
         std::vector<double>& v = sd.keep.back();
         for (int r = 0; r < n; ++r)
            for (int q = m.rowptr[r]; q < m.rowptr[r + 1]; ++q) v[q] = (m.val[q] * cf[r]) * cf[m.colidx[q]];
         m.val = v.data();
      }
      sd.in.Q = sd.q.data();
   }
   // R'_i = Cs_i R_i Cs_0: (r col_{x_i row}) col_{x0 column}, the row's factor first as for Q; border and flat copy are built from these
   if (in.R) {
      sd.r.assign(in.R, in.R + in.n_blocks);
      for (int i = 1; i <= L.N; ++i) {
         pips_csr_view& m = sd.r[i];
         const int n = in.blocks[i].n;
         if (!m.rowptr || n <= 0 || m.rowptr[n] <= 0 || !m.colidx || !m.val) continue;
         const double* rf = col + L.xoff[i];
         sd.keep.emplace_back((size_t)m.rowptr[n], 0.0);
         std::vector<double>& v = sd.keep.back();
         for (int r = 0; r < n; ++r)
            for (int q = m.rowptr[r]; q < m.rowptr[r + 1]; ++q) v[q] = (m.val[q] * rf[r]) * col[m.colidx[q]];
         m.val = v.data();
      }
      sd.in.R = sd.r.data();
   }
   vec(sd.in.bL, L.myl, re + L.my0, false); vec(sd.in.dlow, L.mzl, ri + L.mz0, false); vec(sd.in.dupp, L.mzl, ri + L.mz0, false);
}

}  // namespace pips

using namespace pips;

// ---- the probe (include/pips_hip.h) ------------------------------------------------------------------------------------------------
// who: the entry's name in the messages
static int layout_probe(const char* who, IpmInput in, int rank, int n_ranks, int eliminate_z0, const double* col, const double* row, long long* dims,
                        double* scalars, long long* sizes, void* const* out) {
   TRY(check_ipm_input(in, rank, n_ranks, who));
   if (!dims || !scalars || !sizes || (col == nullptr) != (row == nullptr)) PIPS_FAIL(PIPS_ERR_ARG, "%s: bad arguments", who);
   IpmLayout L;
   ScaledData sd;
   if (col) {
      TRY(ipm_dims(in, eliminate_z0 != 0, L));
      TRY(ipm_hessians(in, L));   // make_scaled indexes the factors by Q's rows and columns: checked first
      make_scaled(in, L, col, row, sd);
      in = sd.in;
   }
   TRY(ipm_layout(in, rank, eliminate_z0 != 0, true, L));
   const long long d[PIPS_IPML_DIMS] = {L.N, L.n0, L.my0, L.mz0, L.myl, L.mzl, L.ry, L.rzr, L.nx, L.my, L.mz, L.ncp, L.nxyz, L.NP,
                                        L.ND, L.nleaf, L.e_mz0, L.e_mzl, L.S, L.has_q ? 1 : 0};
   std::memcpy(dims, d, sizeof(d));
   scalars[0] = L.pairs; scalars[1] = L.norm;
   // the per-leaf and per-block arrays back to back
   LeafSystem all;
   for (const LeafSystem& s : L.leaf) {
      all.Krp.insert(all.Krp.end(), s.Krp.begin(), s.Krp.end()); all.Kci.insert(all.Kci.end(), s.Kci.begin(), s.Kci.end());
      all.kvals.insert(all.kvals.end(), s.kvals.begin(), s.kvals.end()); all.Brd.insert(all.Brd.end(), s.Brd.begin(), s.Brd.end());
      all.Bci.insert(all.Bci.end(), s.Bci.begin(), s.Bci.end()); all.Bv.insert(all.Bv.end(), s.Bv.begin(), s.Bv.end());
   }
   LowerQ lq;
   std::vector<int> have;
   for (const LowerQ& q : L.hq) {
      have.push_back(q.have ? 1 : 0);
      if (!q.have) continue;
      lq.rp.insert(lq.rp.end(), q.rp.begin(), q.rp.end()); lq.ci.insert(lq.ci.end(), q.ci.begin(), q.ci.end() - 1);
      lq.v.insert(lq.v.end(), q.v.begin(), q.v.end() - 1);
   }
   struct Slot { const void* p; long long n; size_t w; };
   auto si = [](const std::vector<int>& v, long long n = -1) { return Slot{v.data(), n < 0 ? (long long)v.size() : n, sizeof(int)}; };
   auto sl = [](const std::vector<long long>& v) { return Slot{v.data(), (long long)v.size(), sizeof(long long)}; };
   auto sd_ = [](const std::vector<double>& v, long long n = -1) { return Slot{v.data(), n < 0 ? (long long)v.size() : n, sizeof(double)}; };
   auto nnz = [](const View& m) { return present(m) ? (long long)m.rp[m.rows] : 0LL; };
   auto vrp = [](const View& m) { return Slot{m.rp, present(m) ? m.rows + 1LL : 0LL, sizeof(int)}; };
   auto vci = [&](const View& m) { return Slot{m.ci, nnz(m), sizeof(int)}; };
   auto vv = [&](const View& m) { return Slot{m.v, nnz(m), sizeof(double)}; };
   const Slot slots[PIPS_IPML_SLOTS] = {
      si(L.xoff), si(L.yoff), si(L.zoff), sl(L.koff),
      si(L.J.rp), si(L.J.ci), sd_(L.J.v), si(L.J.trp), si(L.J.tci), sd_(L.J.tv), si(L.J.long_rows, L.J.n_long), si(L.J.long_trows, L.J.n_tlong),
      sd_(L.c), sd_(L.b), sd_(L.M), sd_(L.Bd), sd_(L.wG), sd_(L.wGs), sd_(L.wXYZ), sl(L.pack), sl(L.code),
      si(all.Krp), si(all.Kci), sd_(all.kvals), si(all.Brd), si(all.Bci), sd_(all.Bv),
      vrp(L.A0), vci(L.A0), vv(L.A0), vrp(L.F0), vci(L.F0), vv(L.F0), vrp(L.C0), vci(L.C0), vv(L.C0), vrp(L.G0), vci(L.G0), vv(L.G0),
      si(have), si(lq.rp), si(lq.ci), sd_(lq.v),
      si(L.Q_rp), si(L.Q_ci, L.Q_nnz), sd_(L.Q_v, L.Q_nnz), sd_(L.qdiag), si(L.Q_long, L.nQ_long)};
   for (int k = 0; k < PIPS_IPML_SLOTS; ++k) {
      if (!out) sizes[k] = slots[k].n;
      else if (sizes[k] != slots[k].n) PIPS_FAIL(PIPS_ERR_ARG, "%s: sizes[%d] is %lld, the layout has %lld", who, k, sizes[k], slots[k].n);
      else if (slots[k].n > 0 && !out[k]) PIPS_FAIL(PIPS_ERR_ARG, "%s: out[%d] is NULL", who, k);
      else if (slots[k].n > 0) std::memcpy(out[k], slots[k].p, (size_t)slots[k].n * slots[k].w);
   }
   return PIPS_OK;
}

extern "C" int pips_ipm_layout_probe(int n_blocks, const pips_ipm_block* blocks, const pips_csr_view* Q, int myl, int mzl, const double* bL,
                                     const double* dlow, const double* dupp, const double* idlow, const double* idupp, int rank, int n_ranks,
                                     int eliminate_z0, const double* col, const double* row, long long* dims, double* scalars, long long* sizes,
                                     void* const* out) {
   const IpmInput in{n_blocks, blocks, Q, myl, mzl, bL, dlow, dupp, idlow, idupp};
   return layout_probe("pips_ipm_layout_probe", in, rank, n_ranks, eliminate_z0, col, row, dims, scalars, sizes, out);
}

extern "C" int pips_ipm_layout_probe_cross(int n_blocks, const pips_ipm_block* blocks, const pips_csr_view* Q, const pips_csr_view* R, int myl, int mzl,
                                           const double* bL, const double* dlow, const double* dupp, const double* idlow, const double* idupp,
                                           int rank, int n_ranks, int eliminate_z0, const double* col, const double* row, long long* dims,
                                           double* scalars, long long* sizes, void* const* out) {
   const IpmInput in{n_blocks, blocks, Q, myl, mzl, bL, dlow, dupp, idlow, idupp, R};
   return layout_probe("pips_ipm_layout_probe_cross", in, rank, n_ranks, eliminate_z0, col, row, dims, scalars, sizes, out);
}
