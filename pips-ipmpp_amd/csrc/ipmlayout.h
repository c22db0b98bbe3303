// Host pass of an IPM handle's creation (harness.hip): from the caller's blocks to everything the harness uploads or hands to the
// engine - dimensions and offsets, J = [A; C] and J^T, the leaf systems K_i with their borders, the flat vectors and masks, the
// replication weights, the pack / code maps, the root's matrices and the flat Hessian.  Plain C++: no device call, no environment
// read (whether the root inequality rows are eliminated comes in as a parameter), so the pass runs and is tested without a GPU
// (pips_ipm_layout_probe, tests/test_ipm_layout_cpu.py).  DESIGN.md section 8.
#pragma once
#include <deque>
#include <utility>
#include <vector>

#include "common.h"
#include "pips_hip.h"

namespace pips {

constexpr int CSR_LONG_ROW = 512;   // rows of J, J^T and Q longer than this go to the long-row kernels (harness.hip k_spmv_long)

struct View { int rows = 0, cols = 0; const int* rp = nullptr; const int* ci = nullptr; const double* v = nullptr; };
inline View view(const pips_csr_view& m) { return View{m.rows, m.cols, m.rowptr, m.colidx, m.val}; }
inline bool present(const View& m) { return m.rp != nullptr && m.rows > 0; }

// what every creation entry point is given: block 0 is the root, Q and R may be null (include/pips_hip.h section 4c)
struct IpmInput {
   int n_blocks = 0;
   const pips_ipm_block* blocks = nullptr;
   const pips_csr_view* Q = nullptr;
   int myl = 0, mzl = 0;
   const double *bL = nullptr, *dlow = nullptr, *dupp = nullptr, *idlow = nullptr, *idupp = nullptr;
   const pips_csr_view* R = nullptr;   // cross Hessians R_i (n_i x n0) between x0 and block i >= 1 (pips_ipm_create_qp_cross)
};
// the argument check of the entry points; who: the function name the message carries
int check_ipm_input(const IpmInput& in, int rank, int n_ranks, const char* who);

// a CSR matrix with its transpose and the rows of either longer than CSR_LONG_ROW (lists padded by one entry: never empty arrays)
struct HostCsr {
   std::vector<int> rp, ci, trp, tci, long_rows, long_trows;
   std::vector<double> v, tv;
   int n_long = 0, n_tlong = 0;
};
// the rows of a CSR row pointer longer than CSR_LONG_ROW, ascending, padded by one entry; returns their count.  The one builder of
// every long-row list: J, J^T and Q of a layout, and the matrix handed to pips_ipm_probe_spmv
int csr_long_rows(const std::vector<int>& rp, std::vector<int>& list);
// One block's Hessian as the caller gave it, checked and with sorted rows (duplicates added up): lower-triangular CSR like the
// reference's SparseSymmetricMatrix.
struct LowerQ { bool have = false; std::vector<int> rp, ci; std::vector<double> v; };
// One block's cross Hessian R_i (n_i x n0, general CSR) as the caller gave it, checked and with sorted rows (duplicates added up):
// the reference's left bordering block.  have: it holds a stored entry.
struct CrossR { bool have = false; std::vector<int> rp, ci; std::vector<double> v; };
// K_i as lower CSR with its constant values, and the border of the leaf by Schur row (pips_kkt_leaf_assemble, pips_border_assemble)
struct LeafSystem {
   std::vector<int> Krp, Kci, Brd, Bci;
   std::vector<double> kvals, Bv;
};

struct IpmLayout {
   int N = 0, n0 = 0, my0 = 0, mz0 = 0, myl = 0, mzl = 0;
   int ry = 0, rzr = 0;   // replicated leading rows of y-type (my0 + myl) and z-type (mz0 + mzl) vectors
   int nx = 0, my = 0, mz = 0;
   int e_mz0 = 0, e_mzl = 0, S = 0;   // what the KKT engine is told: root inequality rows eliminated (e_mz0 = mz0) or among the linking ones
   long long ncp = 0, nxyz = 0, NP = 0, ND = 0, nleaf = 0;
   std::vector<int> xoff, yoff, zoff;   // N + 2 entries: block i covers [off[i], off[i + 1]); [0, off[1]) is the replicated part
   std::vector<long long> koff;         // rows of the leaves' K_i, back to back
   std::vector<LowerQ> hq;
   std::vector<CrossR> hr;
   bool has_q = false;                  // a Hessian of either kind among this rank's blocks
   bool cross = false;                  // a cross Hessian with a stored entry among this rank's blocks
   // several ranks with a cross Hessian on any of them: (Q x)_0 is summed over the ranks, so the flat Q of the ranks != 0 leaves the
   // Q0 block out (ipm_flat_hessian); set by ipm_layout from this rank's own blocks, by the harness once the ranks have agreed
   bool omit_q0 = false;
   HostCsr J;                           // rows [y rows | z rows] over x; root rows on rank 0 only
   std::vector<LeafSystem> leaf;
   std::vector<double> c, b, M, Bd;     // M = [iclow | icupp | ixlow | ixupp], Bd the bounds in that order, masked
   std::vector<double> wG, wGs, wXYZ;   // weights that count replicated entries once; wGs with the signs of the dual objective
   double pairs = 0.0, norm = 0.0;      // this rank's complementarity pairs and data norm
   std::vector<long long> pack, code;   // KKT right-hand sides <- [x | y | z]; leaf diagonal codes
   View A0, F0, C0, G0;                 // the root's matrices; G0 = [C0; G0] (g0_*) where the root inequality rows are kept
   std::vector<int> g0_rp, g0_ci;
   std::vector<double> g0_v;
   // Q over the flat x order, both triangles, with its diagonal and long-row list (padded like HostCsr's)
   std::vector<int> Q_rp, Q_ci, Q_long;
   std::vector<double> Q_v, qdiag;
   int nQ_long = 0;
   long long Q_nnz = 0;
};

// ---- the steps, in the order ipm_layout() runs them ------------------------------------------------------------------------------
int ipm_dims(const IpmInput& in, bool eliminate_z0, IpmLayout& L);   // dimensions and offsets
int ipm_hessians(const IpmInput& in, IpmLayout& L);                  // hq, hr, has_q, cross
void ipm_rows_J(const IpmInput& in, int rank, IpmLayout& L);         // J, J^T, long rows
int ipm_leaf_systems(const IpmInput& in, IpmLayout& L);              // K_i and border per leaf
void ipm_root_matrices(const IpmInput& in, IpmLayout& L);            // A0, F0, C0, G0
int ipm_flat_vectors(const IpmInput& in, IpmLayout& L);              // c, b, M, Bd
// max |entry| of this rank's data, bounds under their indicators
double ipm_data_norm(const IpmInput& in, const std::vector<LowerQ>& hq, const std::vector<CrossR>& hr);
void ipm_weights(int rank, IpmLayout& L);                            // wG, wGs, wXYZ, pairs
void ipm_maps(IpmLayout& L);                                         // pack, code
void ipm_flat_hessian(const IpmInput& in, IpmLayout& L);             // Q_*, qdiag
// all of them; with_J = false leaves J out (a scaled handle keeps the J its scaler scaled on the device)
int ipm_layout(const IpmInput& in, int rank, bool eliminate_z0, bool with_J, IpmLayout& L);

// The data scaled by the factors (Scaler::applyScaling): matrices (a col_j) row_i, c col, b / clow / cupp row, xlow / xupp / col, and
// the lower-triangular Hessians (q col_r) col_c and the cross Hessians (r col_{x_i row}) col_{x0 column} (x = Cs x': Q' = Cs Q Cs;
// the Hessians must have passed ipm_hessians).
// col: nx factors, row: [row_eq (my) | row_ineq (mz)].  Host copies of O(nnz); `in` points into them and into the original indices.
struct ScaledData {
   IpmInput in;
   std::vector<pips_ipm_block> blk;
   std::vector<pips_csr_view> q, r;
   std::deque<std::vector<double>> keep;
};
void make_scaled(const IpmInput& in, const IpmLayout& L, const double* col, const double* row, ScaledData& sd);

}  // namespace pips
