// The border products and the z0 elimination of solveCompressed on a panel of right-hand sides (KktSystem::solve_compressed_multi in
// kkt.hip.h; the reference: LsolveHierarchyBorder / DsolveHierarchyBorder / LtsolveHierarchyBorder on SC_BLOCKSIZE_HIERARCHICAL columns,
// sLinsysRootAug.C:1815-1940).  The single-vector kernels (kernels.hip.h "border products") launched once per column read the border's
// rowptr / colidx / val once per column; here a row's entries are loaded once per chunk of columns, kept in registers, and the loop over
// the columns runs inside.  Included once by engine.hip, inside namespace pips, after kernels.hip.h.
#pragma once

constexpr int BTP_PER_LANE = 4;                         // entries of a row of Bt a lane holds: a pass takes BT_LANES * BTP_PER_LANE = 64 of them
constexpr int BTP_PASS = BT_LANES * BTP_PER_LANE;
constexpr int BMP_PER_THREAD = 4;                       // entries of a leaf row of Br a thread holds per pass

// T(s, q) += alpha sum_p val[p] Z(xoff + col[p], q) for every row of the concatenated Bt CSR (kernels.hip.h) and every q < nr; column q of
// Z at Z + q ldz.  Sixteen lanes per row as in k_border_tmult; a lane loads its entries of the pass (value and position in the leaf vector)
// once and the lanes then walk the columns sixteen at a time: per column the lanes' partial sums meet by shuffles, lane j keeps the sum
// of column q0 + j, and after sixteen columns the lanes of the row write sixteen neighbouring doubles.
//   DET = false: out is the panel T laid out [s][q] (ldo doubles per Schur row, zeroed by the caller): one FP64 atomic per (row, pass,
//                column) - a row of up to 64 entries takes one pass - and a wave's four rows issue four contiguous 128-byte segments per
//                atomic instruction instead of one 8-byte add per row.
//   DET = true:  out is [border row][q] (ldo doubles per row of Bt, zeroed by the caller): plain read-add-stores, every (row, column)
//                owned by one lane, passes in ascending order - the row dots of k_border_rowdot on nr columns, summed in this kernel's
//                fixed tree; k_gather_rows_panel adds them group by group in list order.
// Rows without entries cost a load of two row pointers; a wave whose four rows are all empty goes on at once.
template <bool DET>
__global__ __launch_bounds__(256) void k_border_tmult_panel(const int* __restrict__ rowptr, const int* __restrict__ colidx,
                                                           const double* __restrict__ val, const int* __restrict__ row_sc,
                                                           const long long* __restrict__ row_xoff, const double* __restrict__ Z, long long ldz,
                                                           int nr, double* __restrict__ out, long long ldo, long long nrows, double alpha) {
   const int l = threadIdx.x & (BT_LANES - 1);
   const long long step = ((long long)gridDim.x * blockDim.x) / BT_LANES, i_end = (nrows + step - 1) / step * step;   // whole waves (shuffles)
   for (long long i = (blockIdx.x * (long long)blockDim.x + threadIdx.x) / BT_LANES; i < i_end; i += step) {
      int p0 = 0, p1 = 0;
      if (i < nrows) { p0 = rowptr[i]; p1 = rowptr[i + 1]; }
      const int npass = (p1 - p0 + BTP_PASS - 1) / BTP_PASS;
      int npass_w = max(npass, __shfl_xor(npass, 16));   // the wave's four rows take the passes of the longest together
      npass_w = max(npass_w, __shfl_xor(npass_w, 32));
      if (npass_w == 0) continue;
      const long long xo = npass > 0 ? row_xoff[i] : 0;
      double* dst = npass > 0 ? out + (DET ? i : (long long)row_sc[i]) * ldo : nullptr;
      for (int pass = 0; pass < npass_w; ++pass) {
         double v[BTP_PER_LANE];
         long long c[BTP_PER_LANE];   // position in a column of Z; -1: no entry
#pragma unroll
         for (int k = 0; k < BTP_PER_LANE; ++k) {
            const int p = p0 + pass * BTP_PASS + k * BT_LANES + l;
            const bool ok = p < p1;
            v[k] = ok ? val[p] : 0.0;
            c[k] = ok ? xo + colidx[p] : -1;
         }
         for (int q0 = 0; q0 < nr; q0 += BT_LANES) {
            double mine = 0.0;
#pragma unroll 4   // (four columns' loads in flight; all sixteen unrolled took 225 VGPRs)
            for (int j = 0; j < BT_LANES; ++j) {
               double s = 0.0;
               if (q0 + j < nr) {
                  const double* z = Z + (long long)(q0 + j) * ldz;
#pragma unroll
                  for (int k = 0; k < BTP_PER_LANE; ++k)
                     if (c[k] >= 0) s += v[k] * z[c[k]];
               }
               s += __shfl_xor(s, 1);
               s += __shfl_xor(s, 2);
               s += __shfl_xor(s, 4);
               s += __shfl_xor(s, 8);
               if (j == l) mine = s;
            }
            const int q = q0 + l;
            if (pass < npass && q < nr) {
               if (DET) dst[q] += alpha * mine;
               else if (mine != 0.0) atomic_add_f64(dst + q, alpha * mine);
            }
         }
      }
   }
}

// deterministic mode: G(g, q, s) += sum over the list of target t = g S + s (Engine::g_btm_grp: the border rows of group g on Schur row
// s, ascending = block order) of rowdot[row][q], in list order; group g's S x nr panel (column q at q S) at gp + g gstride.  A thread
// per (target, column), the columns fastest: neighbouring threads read neighbouring doubles of a border row's dots.
__global__ void k_gather_rows_panel(long long n_targets, const long long* __restrict__ tgt, const long long* __restrict__ off,
                                    const long long* __restrict__ rows, const double* __restrict__ rowdot, long long ldo, int nr, int S,
                                    double* __restrict__ gp, long long gstride) {
   const long long n = n_targets * nr;
   for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
      const long long t = idx / nr;
      const int q = (int)(idx - t * nr);
      double s = 0.0;
      for (long long p = off[t]; p < off[t + 1]; ++p) s += rowdot[rows[p] * ldo + q];
      const long long g = tgt[t] / S, srow = tgt[t] - g * S;
      gp[g * gstride + (long long)q * S + srow] += s;
   }
}

// R(s, q) += T(s, q) for s < S, q < nr: column q of R at R + q ldr; T(s, q) at T[s ts + q tq] - the atomics' panel is [s][q], the
// deterministic one [q][s]
__global__ void k_panel_add(double* __restrict__ R, long long ldr, const double* __restrict__ T, long long ts, long long tq, int S, int nr) {
   const long long n = (long long)S * nr;
   for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
      const long long q = idx / S, s = idx - q * S;
      R[q * ldr + s] += T[s * ts + q * tq];
   }
}

// W(i, q) = alpha sum_p val[src[p]] X0(sc[p], q) from the side of the leaf rows (Engine::d_br_rowptr / d_br_sc / d_br_src: the border
// transposed once at analyze time, every row's entries in ascending (block, Schur column)): no atomics, fixed order.  A thread per leaf
// row: it loads its entries once (four per pass; a leaf row of the border rarely holds more), then walks the columns - neighbouring
// threads store neighbouring doubles of a column of W (column q at W + q ldw; X0's at X0 + q ldx).  Every row of W is written, the rows
// without border entries with zeros: the caller need not clear W.
__global__ __launch_bounds__(256) void k_border_mult_panel(const int* __restrict__ rowptr, const int* __restrict__ sc, const int* __restrict__ src,
                                                          const double* __restrict__ val, const double* __restrict__ X0, long long ldx, int nr,
                                                          double* __restrict__ W, long long ldw, long long nrows, double alpha) {
   for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nrows; i += (long long)gridDim.x * blockDim.x) {
      const int p0 = rowptr[i], p1 = rowptr[i + 1];
      if (p0 == p1) {
         for (int q = 0; q < nr; ++q) W[(long long)q * ldw + i] = 0.0;
         continue;
      }
      for (int pb = p0; pb < p1; pb += BMP_PER_THREAD) {
         double v[BMP_PER_THREAD];
         int c[BMP_PER_THREAD];   // Schur index; -1: no entry
#pragma unroll
         for (int k = 0; k < BMP_PER_THREAD; ++k) {
            const bool ok = pb + k < p1;
            v[k] = ok ? val[src[pb + k]] : 0.0;
            c[k] = ok ? sc[pb + k] : -1;
         }
         for (int q = 0; q < nr; ++q) {
            const double* x = X0 + (long long)q * ldx;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < BMP_PER_THREAD; ++k)
               if (c[k] >= 0) s += v[k] * x[c[k]];
            double* w = W + (long long)q * ldw + i;
            *w = pb == p0 ? alpha * s : *w + alpha * s;
         }
      }
   }
}

// k_z0_elim (kkt.hip.h) with a column index (grid.y): column q of b3 at b3 + q ldb, of x1 at x1 + q ldx.  Deterministic mode launches
// mode 0 with one thread per column, as the single path launches one thread
__global__ void k_z0_elim_panel(int mode, int mz0, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ v,
                                const double* __restrict__ zdiag, double* __restrict__ b3, long long ldb, double* __restrict__ x1, long long ldx) {
   b3 += (long long)blockIdx.y * ldb;
   x1 += (long long)blockIdx.y * ldx;
   for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < mz0; k += gridDim.x * blockDim.x) {
      if (mode == 0) {
         const double t = b3[k] / zdiag[k];
         for (int p = rp[k]; p < rp[k + 1]; ++p) atomic_add_f64(x1 + ci[p], -v[p] * t);
      } else {
         double s = b3[k];
         for (int p = rp[k]; p < rp[k + 1]; ++p) s -= v[p] * x1[ci[p]];
         b3[k] = s / zdiag[k];
      }
   }
}
