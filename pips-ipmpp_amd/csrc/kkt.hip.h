// Fused two-level KKT system of one rank: leaves (Engine) + replicated root (DenseLdl, or a one-block sparse Engine) + Schur reduction.
// Mirrors DistributedRootLinearSystem::factor2 (:206-243) and DistributedLinearSystem::solveCompressed (:409-420)
// with sLinsysRootAug::{finalizeKKTdense, Lsolve, Dsolve, Ltsolve} (sLinsysRootAug.C:1769-1796, 323-365).
// Included once by engine.hip, inside namespace pips, after Engine and DenseLdl (the switches: knobs.h, which engine.hip includes); the pips_hip_kkt_* entry points there call the
// methods of KktSystem.
#pragma once

// SC[0:n0,0:n0] -= C0^T diag(zdiag)^-1 C0 (lower triangle; zdiag < 0): schur_complement_add_CTDC_block
// (sLinsysRootAug.C:1276-1338, SparseStorage::matTransDinvMultMat SparseStorage.C:1257).  One thread per row of C0.
// sc_rowptr != nullptr: SC is the value array of the sparse root's CSR pattern, whose x0 block is dense: (i, j), j <= i < n0,
// sits at sc_rowptr[i] + j
__global__ void k_ctdc(int mz0, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ v,
                       const double* __restrict__ zdiag, double* __restrict__ SC, int ld, const int* __restrict__ sc_rowptr) {
   for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < mz0; k += gridDim.x * blockDim.x) {
      const double dinv = 1.0 / zdiag[k];
      for (int p = rp[k]; p < rp[k + 1]; ++p)
         for (int q = rp[k]; q < rp[k + 1]; ++q) {
            const int i = ci[p], j = ci[q];
            if (i >= j) atomic_add_f64(sc_rowptr ? SC + sc_rowptr[i] + j : SC + i + (long long)j * ld, -v[p] * v[q] * dinv);
         }
   }
}

// solveReducedLinkCons (sLinsysRootAug.C:384-466), z0 elimination: mode 0: t_k = b3_k / zdiag_k ; rhs1 -= C0^T t
//                                                                     mode 1: b3_k = (b3_k - (C0 x1)_k) / zdiag_k
__global__ void k_z0_elim(int mode, int mz0, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ v,
                          const double* __restrict__ zdiag, double* __restrict__ b3, double* __restrict__ x1) {
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

// pack / unpack the lower triangle of the column-major S x S Schur complement (column c holds S - c entries):
// the reference reduces packed triangles too (submatrixAllReduceDiagLower, DistributedRootLinearSystem.C:1661-1707)
__global__ void k_pack_lower(const double* __restrict__ M, int ld, int S, double* __restrict__ packed, int unpack) {
   const int c = blockIdx.y;
   const long long base = (long long)c * S - (long long)c * (c - 1) / 2;
   double* col = const_cast<double*>(M) + (long long)c * ld;
   for (int r = c + blockIdx.x * blockDim.x + threadIdx.x; r < S; r += gridDim.x * blockDim.x) {
      if (unpack) col[r] = packed[base + (r - c)];
      else packed[base + (r - c)] = col[r];
   }
}

// the same for a row panel [R0, R1) of the lower triangle: column c < R1 contributes its rows max(c, R0) .. R1 - 1
__global__ void k_pack_rows(const double* __restrict__ M, int ld, int R0, int R1, double* __restrict__ packed, int unpack) {
   const int c = blockIdx.y;
   const long long h = R1 - R0;
   const long long base = c <= R0 ? (long long)c * h
                                  : (long long)R0 * h + (long long)(c - R0) * R1 - ((long long)c * (c - 1) / 2 - (long long)R0 * (R0 - 1) / 2);
   const int r_first = c > R0 ? c : R0;
   double* col = const_cast<double*>(M) + (long long)c * ld;
   for (int r = r_first + blockIdx.x * blockDim.x + threadIdx.x; r < R1; r += gridDim.x * blockDim.x) {
      if (unpack) col[r] = packed[base + (r - r_first)];
      else packed[base + (r - r_first)] = col[r];
   }
}

// Diagonal entry of row r of the Schur complement: dense column-major SC (rowptr == nullptr) or the CSR lower pattern of the sparse SC,
// whose rows end with their diagonal entry
__device__ __forceinline__ double& sc_diag(double* __restrict__ M, int ld, const int* __restrict__ rowptr, int r) {
   return rowptr ? M[rowptr[r + 1] - 1] : M[(long long)r * ld + r];
}
// diagonal_add_constant_from
__global__ void k_add_const_diag(double* __restrict__ M, int ld, const int* __restrict__ rowptr, int first, int n, double value) {
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) sc_diag(M, ld, rowptr, first + i) += value;
}
__global__ void k_add_diag(double* __restrict__ M, int ld, const int* __restrict__ rowptr, int first, const double* __restrict__ d, int n) {
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) sc_diag(M, ld, rowptr, first + i) += d[i];
}

// points a stream member somewhere else for the length of a scope (error returns included)
struct StreamSwap {
   hipStream_t& slot;
   const hipStream_t keep;
   StreamSwap(hipStream_t& s, hipStream_t to) : slot(s), keep(s) { slot = to; }
   ~StreamSwap() { slot = keep; }
};

struct KktSystem {
   Engine* leaves = nullptr;
   std::unique_ptr<DenseLdl> root;
   int n0 = 0, my0 = 0, myl = 0, mzl = 0, S = 0;
   int rank = 0, n_ranks = 1;
   void* comm = nullptr;
   DevBuf<double> d_SC, d_t, d_fin_val, d_c0_val, d_red, d_packed;
   DevBuf<long long> d_fin_idx;
   long long n_fin = 0;
   std::vector<long long> fin_idx_rows;   // the table's entries from A0 / F0 / G0 (host copy: set_root_hessian appends to them)
   std::vector<double> fin_val_rows;
   DevBuf<double> d_gall, d_gvec_all;   // deterministic mode over several ranks: all eight group slots (8 x S x S / 8 x S)
   int mz0 = 0;
   DevBuf<int> d_c0_rp, d_c0_ci;
   const double* d_zdiag0 = nullptr;   // caller-owned, set per iteration
   double root_reg_primal = 0.0, root_reg_dual = 0.0;   // pips_hip_kkt_set_root_regularization
   hipStream_t comm_stream = nullptr;   // panel-wise Schur reduction beside the leaf work
   hipEvent_t ev_reduced = nullptr;
   // The dense root is factorised on a stream of its own: it is a latency chain (S = 2000: 16 diagonal tiles, 1.9 ms with the chip
   // nearly idle) and nothing needs its factors before the Dsolve of the next solveCompressed - the leaf solves of that call's
   // Lsolve run beside it.  root_wait() joins the main stream with it (before Dsolve, the next factorisation, an inertia query).
   hipStream_t root_stream = nullptr;
   hipEvent_t ev_sc_final = nullptr, ev_root_done = nullptr;
   bool root_pending = false;
   bool root_own_stream = true;   // pips_hip_kkt_set_root_stream: a caller that asks for the root's inertia after every factorisation (the IPM
                                  // harness) has nothing to run beside the root - the second stream then only costs (measured: section 4.3b)
   bool use_rsag = false, force_reduce = false;
   bool solve_graph = false;                // pips_hip_kkt_set_solve_graph
   hipGraphExec_t graph_exec = nullptr;
   hipStream_t graph_stream = nullptr;
   // everything a captured launch sequence has baked in: buffer addresses, the Ltsolve path, the number of refinement launches, the
   // elimination of root inequality rows (zdiag0, C0), the root's pivoting mode, the analysis the leaf buffers belong to
   struct GraphKey {
      const void *b0 = nullptr, *bl = nullptr, *zdiag0 = nullptr, *c0_val = nullptr, *c0_rp = nullptr, *c0_ci = nullptr;
      int from_factor = 0, refine_steps = 0, refine_mode = 0, mz0 = 0, pivoting = 0, bk_gen = 0;
      long long analysis_gen = 0;
      bool operator==(const GraphKey& o) const {
         return b0 == o.b0 && bl == o.bl && zdiag0 == o.zdiag0 && c0_val == o.c0_val && c0_rp == o.c0_rp && c0_ci == o.c0_ci &&
                from_factor == o.from_factor && refine_steps == o.refine_steps && refine_mode == o.refine_mode && mz0 == o.mz0 &&
                pivoting == o.pivoting && bk_gen == o.bk_gen && analysis_gen == o.analysis_gen;
      }
   } graph_key;
   long long graph_captures = 0, graph_replays = 0;
   bool last_ltsolve_from_factor = false;   // which Ltsolve the last solveCompressed took (reported per solve, not only at analyze time)
   // Sweeps of the augmented factor for both halves of solveCompressed (Engine::forward_augmented / backward_augmented).  They carry no
   // refinement, so they are taken only on evidence that this factorisation is accurate: no perturbed pivot, and an earlier
   // solveCompressed on the SAME factors went the refined way and every refined leaf solve in it met the backward-error tolerance
   // without a step (aug_validated_gen == factor_gen).  The first solveCompressed after every factorisation is that witness.
   long long factor_gen = 0, aug_validated_gen = -1;
   int last_solve_path = 0;   // 0: two refined leaf solves, 1: refined Lsolve + Ltsolve from the factor, 2: augmented sweeps, 3: augmented sweeps
                              // whose result was checked (below)
   // One rank: the witness is the first sweep pair itself - its result x_i is put into the leaf rows, r_i = b_i - Br_i x0 - K_i x_i, and
   // accepted where the measure of the adaptive refinement is within the tolerance (one product with K instead of a refined solve and
   // its extra backward sweep); a result that fails is thrown away, the saved right-hand side goes the refined way and the sweeps stay
   // off for these factors (aug_failed_gen).  Several ranks keep the refined witness: the decision to repeat a solveCompressed would
   // have to be taken by all ranks together.  PIPS_HIP_AUG_WITNESS=0: the refined witness everywhere.
   long long aug_failed_gen = -1;
   bool checked_witness = knob_int<K_AUG_WITNESS>() != 0;
   // Every solveCompressed that goes by sweeps is measured like that (pips_hip_kkt_set_solve_check: every k-th one; 0 = the witness
   // only, rounds 4's behaviour): the reference's PARDISO measures and refines EVERY leaf solve (iparm[7] = 2,
   // PardisoProjectSolver.C:72), and one clean right-hand side does not bound the backward error of the next.  Several ranks decide
   // together: each solveCompressed ends with a one-number all-reduce "did any rank's check fail"; if so every rank restores its
   // right-hand side and all go the refined way (a rank's inaccurate -Br^T K^-1 b taints x0 for everybody).
   int solve_check_every = 1, sweeps_since_check = 0;
   long long solves_since_factor = 0;   // equal on every rank: which solveCompressed calls are scheduled for a measure (every solve_check_every-th)
   PinnedBuf<double> h_flag;            // pinned: the one-number exchange of settle() without a host wait before the collective
   long long checked_solves = 0, failed_checks = 0;
   DevBuf<double> d_flag;
   bool joint_aug_any = false;        // several ranks: some rank's analysis chose the sweeps (all-reduced once per analysis)
   long long joint_aug_gen = -1;
   DevBuf<double> d_bsave, d_b0save;
   bool root_pivoting_set = false;   // pips_hip_kkt_set_root_pivoting decided; else: Bunch-Kaufman iff root inequality rows are eliminated
   // phase times of one factorize and the solveCompressed calls after it (pips_hip_kkt_get_timing; on with the batch's timing switch):
   // 0 diagonals + zero SC, 1 leaf factorisation, 2 Schur reduction, 3 finalize, 4 root factorisation (its own stream),
   // 5 Lsolve leaf solves, 6 Lsolve border product + b0 reduction, 7 Dsolve, 8 Ltsolve, 9 x_i = z_i - u_i,
   // 10 panel-wise Schur reduction on its own stream (sum over the panels; phase 2 is then only what the main stream waited for it),
   // 11 the join with the root's stream before Dsolve, 12 the measure of the sweeps' result, 13 the root factorisation where it sits
   // on the main stream.  Both root kinds report the same phases: the sparse root's 0 and 3 were done but not timed before the two
   // factorisations became one, and its phase 2 is a record that stays open (begin_i) like the dense root's.
   PhaseTimer timer;
   // sparse root: SC lives as the value array of a lower-triangular CSR pattern inside a one-block sparse
   // engine, which factorises and solves it with the leaf machinery (ordering, head / dense tail, refinement)
   bool sparse = false;
   std::unique_ptr<Engine> root_sp;
   std::vector<int> sc_rowptr, sc_colidx, root_perm, root_colcount;
   int root_order_mode = 0;   // sparse root: 0 minimum degree, 1 dense-tile band, 2 dissection around the hubs
   DevBuf<int> d_sc_rowptr;   // (its rows end with their diagonal entries: the diagonals finalize() adds to)
   ~KktSystem() {
      if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
      if (graph_stream) (void)hipStreamDestroy(graph_stream);
      if (root_stream) { (void)hipStreamSynchronize(root_stream); (void)hipStreamDestroy(root_stream); }
      if (ev_sc_final) (void)hipEventDestroy(ev_sc_final);
      if (ev_root_done) (void)hipEventDestroy(ev_root_done);
      if (comm_stream) (void)hipStreamDestroy(comm_stream);
      if (ev_reduced) (void)hipEventDestroy(ev_reduced);
   }

   // ---- creation ---------------------------------------------------------------------------------------------------
   // what: the entry point's name (messages).  blk_cols_ptr / blk_cols: see pips_hip_kkt_create_sparse; used with sparse_root only.
   static int create(void** handle, Engine* e, const char* what, bool sparse_root, int n0, int my0, int myl, int mzl, const RootRows (&rows)[3],
                     int n_blocks_global, const int* blk_cols_ptr, const int* blk_cols, void* comm, int rank, int n_ranks) {
      const int S = n0 + my0 + myl + mzl;
      if (S != e->S) PIPS_FAIL(PIPS_ERR_ARG, "%s: n0+my0+myl+mzl = %d but the batch was created with S = %d", what, S, e->S);
      if (sparse_root && n_ranks > 1 && !blk_cols_ptr) PIPS_FAIL(PIPS_ERR_ARG, "%s: n_ranks > 1 needs the border column sets of all blocks", what);
      auto k = std::make_unique<KktSystem>();
      k->leaves = e; k->sparse = sparse_root;
      k->n0 = n0; k->my0 = my0; k->myl = myl; k->mzl = mzl; k->S = S;
      k->comm = comm; k->rank = rank; k->n_ranks = n_ranks;
      k->force_reduce = comm && knob_set<K_FORCE_REDUCE>();
      const int rc = sparse_root ? k->init_sparse_root(rows, n_blocks_global, blk_cols_ptr, blk_cols) : k->init_dense_root(rows);
      if (rc) return rc;
      *handle = k.release();
      return PIPS_OK;
   }
   // constant root blocks added by finalizeKKT: A0 at row n0, F0 at row n0+my0, G0 at row n0+my0+myl
   // (sLinsysRootAug.C:270-320, 1782-1796); pos(r, c): where entry (r, c) of the lower triangle sits in the Schur complement's values
   template <class Pos>
   int upload_root_entries(const RootRows (&rows)[3], Pos pos) {
      std::vector<long long> idx;
      std::vector<double> val;
      for (const RootRows& b : rows) {
         if (!b.rowptr) continue;
         for (int r = 0; r < b.nrows; ++r)
            for (int p = b.rowptr[r]; p < b.rowptr[r + 1]; ++p) { idx.push_back(pos(b.row0 + r, b.colidx[p])); val.push_back(b.val[p]); }
      }
      fin_idx_rows = idx; fin_val_rows = val;
      return upload_fin(idx, val);
   }
   int upload_fin(const std::vector<long long>& idx, const std::vector<double>& val) {
      n_fin = (long long)idx.size();
      if (int rc = d_fin_idx.upload(idx)) return rc;
      return d_fin_val.upload(val);
   }
   // Q0, the root block's Hessian (lower-triangular CSR, n0 x n0), as constant entries of the x0 block (sLinsysRootAug.C:234-261): they join
   // the table finalize() applies at every factorisation - after the reduction over the ranks, on every rank, like xdiag0.  The sparse
   // root's pattern holds the dense x0 block, so every entry has a place.  A second call replaces the first; nullptr removes the entries.
   int set_root_hessian(const int* Q0_rowptr, const int* Q0_colidx, const double* Q0_val) {
      std::vector<long long> idx = fin_idx_rows;
      std::vector<double> val = fin_val_rows;
      const long long ld = S;
      std::vector<std::pair<long long, double>> q0;   // entries given twice are added up here: one addition per address in k_add_entries
      for (int r = 0; Q0_rowptr && r < n0; ++r)
         for (int p = Q0_rowptr[r]; p < Q0_rowptr[r + 1]; ++p) {
            const int c = Q0_colidx[p];
            if (c < 0 || c > r) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_kkt_set_root_hessian: entry (%d, %d) is not in the lower triangle of the x0 block", r, c);
            const long long pos = sparse ? sc_pos(r, c) : (long long)r + (long long)c * ld;
            if (pos < 0) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_set_root_hessian: entry (%d, %d) has no place in the sparse root's pattern", r, c);
            q0.push_back({pos, Q0_val[p]});
         }
      std::stable_sort(q0.begin(), q0.end(), [](const std::pair<long long, double>& a, const std::pair<long long, double>& b) { return a.first < b.first; });
      for (size_t k = 0; k < q0.size(); ++k) {
         if (k > 0 && q0[k].first == q0[k - 1].first) val.back() += q0[k].second;
         else { idx.push_back(q0[k].first); val.push_back(q0[k].second); }
      }
      return upload_fin(idx, val);
   }
   int init_dense_root(const RootRows (&rows)[3]) {
      Engine* e = leaves;
      root = std::make_unique<DenseLdl>();
      root->n = S; root->n_primal = n0;
      root->device = e->device; root->stream = e->stream;
      root->thr_rel = e->thr_rel; root->repl_rel = e->repl_rel;
      int rc = root->init();
      if (rc) return rc;
      // several ranks: the dense root factorised column-cyclically over the ranks instead of redundantly on every one of them
      // (PIPS_HIP_ROOT_DISTRIBUTED=1; untimed - see DenseLdl::set_distributed)
      if (comm && n_ranks > 1 && knob_int<K_ROOT_DISTRIBUTED>() != 0 && (rc = root->set_distributed(comm, rank, n_ranks))) return rc;
      PIPS_TRY(d_SC.alloc((size_t)S * S));
      PIPS_TRY(d_t.alloc(std::max<size_t>((size_t)e->n_total, 1)));
      // SC is column-major with the lower triangle valid: (r,c) -> r + c*S.
      const long long ld = S;
      if ((rc = upload_root_entries(rows, [ld](int r, int c) { return (long long)r + (long long)c * ld; }))) return rc;
      // several ranks: Schur SYRK in row panels, each reduced as soon as it is final (PIPS_HIP_SC_PANELS, default 4 for S >= 1024; 1 =
      // one reduction after all leaf work); PIPS_HIP_SC_REDUCE=rsag: reduce-scatter + all-gather instead of the all-reduce
      if (e->deterministic && (rc = e->set_det_groups(rank, n_ranks))) return rc;
      if (comm && (n_ranks > 1 || force_reduce) && !e->deterministic) {
         // default: panels only where the reduction is worth hiding (S >= 4096: >= 64 MB packed; splitting the SYRK costs ~1 ms)
         int panels = S >= 4096 ? 4 : 1;
         if (knob_set<K_SC_PANELS>()) panels = (int)knob_int<K_SC_PANELS>();
         if ((rc = e->set_sc_panels(panels))) return rc;
         if (const char* m = knob_text<K_SC_REDUCE>()) use_rsag = std::string(m) == "rsag";
      }
      return PIPS_OK;
   }
   // position of entry (r, c), c <= r, in the sparse root's value array (-1: not in the pattern)
   long long sc_pos(int r, int c) const {
      const int* b0 = sc_colidx.data() + sc_rowptr[r];
      const int* b1 = sc_colidx.data() + sc_rowptr[r + 1];
      const int* it = std::lower_bound(b0, b1, c);
      return (it != b1 && *it == c) ? (long long)(it - sc_colidx.data()) : -1;
   }
   // Sparse-root variant (createSchurCompSymbSparseUpper, DistributedProblem.cpp:2235+; finalizeKKTsparse, sLinsysRootAug.C:
   // 1629-1739).  Pattern of SC (lower): the dense x0 block, for every block the clique on its non-empty border columns, the
   // root rows A0 / F0 / G0 and a full diagonal.  With 2-link structure (a linking row touches two blocks) it stays sparse.
   int init_sparse_root(const RootRows (&rows)[3], int n_blocks_global, const int* blk_cols_ptr, const int* blk_cols) {
      Engine* e = leaves;
      std::vector<std::pair<const int*, int>> cliques;
      if (blk_cols_ptr)
         for (int b = 0; b < n_blocks_global; ++b) cliques.emplace_back(blk_cols + blk_cols_ptr[b], blk_cols_ptr[b + 1] - blk_cols_ptr[b]);
      // (the blocks' non-empty border columns from the border's row pointers: BlockSym::bmap holds the same where the border took part in
      //  the symbolic analysis and is empty in Schur mode 2 - pattern, position tables and the packed solves' tables rest on one rule)
      const SchurPack& pk = e->border_pack();
      for (int b = 0; b < e->nblk; ++b) cliques.emplace_back(pk.block_cols(b), pk.nb[b]);
      sc_lower_pattern(S, n0, rows, cliques, sc_rowptr, sc_colidx);
      // ---- per-block position tables for the leaf kernels
      std::vector<int> tab;
      std::vector<long long> off(e->nblk, 0);
      for (int b = 0; b < e->nblk; ++b) {
         const int* bm = pk.block_cols(b);
         const int nb = pk.nb[b];
         off[b] = (long long)tab.size();
         tab.resize(tab.size() + (size_t)nb * nb, 0);
         for (int la = 0; la < nb; ++la)
            for (int lb = 0; lb <= la; ++lb) tab[off[b] + (long long)la * nb + lb] = (int)sc_pos(bm[la], bm[lb]);
      }
      int rc = e->set_sc_tables(tab, off, (long long)sc_rowptr[S]);
      if (rc) return rc;
      if (e->deterministic && (rc = e->set_det_groups(rank, n_ranks))) return rc;   // group buffers as long as the value array
      // ---- the root as a one-block sparse engine; its value array is the Schur complement
      root_sp = std::make_unique<Engine>();
      Engine* r = root_sp.get();
      r->nblk = 1; r->S = 0; r->device = e->device; r->stream = e->stream;
      r->thr_rel = e->thr_rel; r->repl_rel = e->repl_rel;
      r->deterministic = e->deterministic;   // (the root's own factorisation and sweeps: slots and fixed-order gathers instead of atomics)
      r->in.assign(1, BlockInput());
      r->in[0].n = S; r->in[0].n_primal = n0;
      r->in[0].krow = sc_rowptr; r->in[0].kcol = sc_colidx;
      // elimination order (sparse_root_order, rootplan.cpp)
      const bool f = knob_set<K_SPARSE_ROOT_BAND>();   // tests: force a path
      const int forced = (int)knob_int<K_SPARSE_ROOT_BAND>();
      int cut = 0;
      root_order_mode = sparse_root_order(S, n0 + my0, sc_rowptr, sc_colidx, TILE, ROOT_ND_MAX_COLCOUNT, f ? &forced : nullptr, root_perm, root_colcount, cut);
      if (root_order_mode == 2) {
         r->opt.user_perm = root_perm.data();
         r->opt.user_colcount = root_colcount.data();
         r->opt.force_n_head = cut;
         r->sn_width = HEAD_WMAX;
      } else if (root_order_mode == 1) {
         r->opt.user_perm = root_perm.data();
         r->opt.force_n_head = 0;
      } else {
         r->opt.constrain_order = my0 > 0;
      }
      if ((rc = r->analyze(4))) return rc;
      // ---- constant root entries; the diagonals added by finalize() are the last entries of the rows of d_sc_rowptr
      if ((rc = upload_root_entries(rows, [this](int rr, int c) { return sc_pos(rr, c); }))) return rc;
      if ((rc = d_sc_rowptr.upload(sc_rowptr))) return rc;
      PIPS_TRY(d_t.alloc(std::max<size_t>((size_t)e->n_total, 1)));
      return PIPS_OK;
   }
   int set_root_inequalities(int mz0_new, const int* C0_rowptr, const int* C0_colidx, const double* C0_val) {
      mz0 = mz0_new;
      // -C0^T Omega^-1 C0 in the x0 block (sLinsysRootAug.C:1276-1294): an active row makes it a huge low-rank matrix plus an O(1) rest,
      // the static pivot rule then takes the cancelled pivots for zeros - the reference leaves that to dsytrf, so does the root here
      if (root && !root_pivoting_set) root->pivoting = mz0 > 0 ? 1 : 0;
      if (mz0 == 0) return PIPS_OK;
      std::vector<int> rp(C0_rowptr, C0_rowptr + mz0 + 1), ci(C0_colidx, C0_colidx + C0_rowptr[mz0]);
      std::vector<double> v(C0_val, C0_val + C0_rowptr[mz0]);
      int rc;
      if ((rc = d_c0_rp.upload(rp)) || (rc = d_c0_ci.upload(ci)) || (rc = d_c0_val.upload(v))) return rc;
      PIPS_TRY(d_red.alloc((size_t)std::max(S, 1)));
      return PIPS_OK;
   }

   // ---- factorisation ----------------------------------------------------------------------------------------------
   // the Schur complement as both root kinds hold it: the column-major S x S array of the dense root (lower triangle valid), or the value
   // array of the sparse root's CSR pattern (ld 0, rowptr on the device)
   struct ScView { double* val; int ld; size_t count; const int* rowptr; };
   ScView sc_view() const { return sparse ? ScView{root_sp->d_kval, 0, (size_t)sc_rowptr[S], d_sc_rowptr} : ScView{d_SC, S, (size_t)S * S, nullptr}; }
   int root_wait() {
      if (root_pending) {
         if (root && root->check_pending) {   // Bunch-Kaufman root: were there indices without a pivot inside their tile?  (host wait for the
                                              // root's stream - the work queued on the main stream meanwhile keeps the device busy)
            int rc;
            { StreamSwap on_root(root->stream, root_stream); rc = root->check_pivots(); }
            if (rc) return rc;
            HIP_TRY(hipEventRecord(ev_root_done, root_stream));
         }
         HIP_TRY(hipStreamWaitEvent(leaves->stream, ev_root_done, 0));
         root_pending = false;
      } else if (root && root->check_pending) {
         // the root was factorised on the main stream (pips_hip_kkt_set_root_stream(0)): the pivot check is still owed, and it reads from the
         // device and waits - it must happen here, before a capture of the solve sequence begins, not inside DenseLdl::solve_dev
         if (const int rc = root->check_pivots()) return rc;
      }
      return PIPS_OK;
   }
   // deterministic mode over several ranks: every rank's group buffers to every rank, then ALL eight slots in the one fixed tree (the
   // leaf engine left its groups unreduced, DetGroupPlan::global) - equal bits for 1, 2, 4 and 8 ranks
   int reduce_groups(const ScView& sc) {
      Engine* e = leaves;
      const size_t gs = sc.count;
      if (!d_gall) PIPS_TRY(d_gall.alloc(8 * gs));
      HIP_TRY(hipMemsetAsync(d_gall, 0, 8 * gs * sizeof(double), e->stream));
      HIP_TRY(hipMemcpyAsync(d_gall + (size_t)e->det.first_slot * gs, e->d_gbuf, (size_t)e->det.n_groups * gs * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      // every rank's slots to every rank: 1 x the bytes (the all-reduce of zeros it replaces moved 8 x the bytes)
      if (int rc = pips_hip_all_gather(comm, d_gall, (size_t)e->det.slots * gs, 8 / e->det.slots, e->stream)) return rc;
      // the dense array column by column, the value array as one vector
      const dim3 grid = sc.rowptr ? dim3((unsigned)std::max<size_t>(1, std::min<size_t>(1024, (gs + 255) / 256)), 1) : dim3(std::max(1, std::min(64, (S + 255) / 256)), S);
      hipLaunchKernelGGL(k_reduce_groups, grid, dim3(256), 0, e->stream, sc.val, sc.ld, sc.rowptr ? (int)gs : S, d_gall, (long long)gs, 8, 0);
      return PIPS_OK;
   }
   // reduceKKT (:860-881): the sum over the ranks.  Sparse root: one all-reduce of the value array.  Dense root: only the lower triangle
   // is authoritative - S(S+1)/2 packed doubles instead of S^2, in row panels where the Schur SYRK ran in panels
   int reduce_sum(const ScView& sc) {
      Engine* e = leaves;
      if (sc.rowptr) return pips_hip_allreduce_sum(comm, sc.val, sc.count, e->stream);
      int rc;
      const size_t np = (size_t)S * (S + 1) / 2;
      const size_t n_groups = std::max<size_t>(e->scp.groups.size(), 1);
      const size_t P = (size_t)std::max(1, pips_hip_comm_size(comm));
      const size_t cap = np + (n_groups + 1) * P;   // reduce-scatter pads every piece to a multiple of the rank count
      PIPS_TRY(d_packed.reserve(cap));
      auto reduce_piece = [&](double* buf, size_t cnt, hipStream_t st) -> int {
         return use_rsag ? pips_hip_allreduce_sum_rsag(comm, buf, cnt, st) : pips_hip_allreduce_sum(comm, buf, cnt, st);
      };
      if (e->scp.groups.empty()) {
         const dim3 pg(std::max(1, std::min(64, (S + 255) / 256)), S);
         hipLaunchKernelGGL(k_pack_lower, pg, dim3(256), 0, e->stream, sc.val, S, S, d_packed, 0);
         if ((rc = reduce_piece(d_packed, np, e->stream))) return rc;
         hipLaunchKernelGGL(k_pack_lower, pg, dim3(256), 0, e->stream, sc.val, S, S, d_packed, 1);
         return PIPS_OK;
      }
      // Panel-wise: the Schur SYRK ran in row-panel groups (Engine::set_sc_panels); the rows of panel q are final on this rank
      // once group q has run, so their reduction goes out on a second stream while the leaves compute the later groups -
      // the overlap of leaf work with MPI_Allreduce that DistributedRootLinearSystem.C:860-881 cannot have (it reduces
      // after all children are done).  Everything was enqueued by e->factor(); here only the reductions are issued, in order.
      if (!comm_stream) {
         HIP_TRY(hipStreamCreateWithFlags(&comm_stream, hipStreamNonBlocking));
         HIP_TRY(hipEventCreateWithFlags(&ev_reduced, hipEventDisableTiming));
      }
      size_t off = 0;
      for (size_t q = 0; q < e->scp.groups.size(); ++q) {
         const int R0 = e->scp.row_begin[q], R1 = e->scp.row_begin[q + 1];
         if (R1 <= R0) continue;
         const size_t h = (size_t)(R1 - R0);
         const size_t cnt = (size_t)R0 * h + h * (h + 1) / 2;
         HIP_TRY(hipStreamWaitEvent(comm_stream, e->ev_sc[q], 0));
         const dim3 pg(std::max(1, std::min(64, (R1 - R0 + 255) / 256)), R1);
         const int rec_panel = timer.begin_i(comm_stream, 10);   // pack + collective + unpack of this panel, beside the leaf work
         hipLaunchKernelGGL(k_pack_rows, pg, dim3(256), 0, comm_stream, sc.val, S, R0, R1, d_packed + off, 0);
         if ((rc = reduce_piece(d_packed + off, cnt, comm_stream))) return rc;
         hipLaunchKernelGGL(k_pack_rows, pg, dim3(256), 0, comm_stream, sc.val, S, R0, R1, d_packed + off, 1);
         timer.end_i(rec_panel, comm_stream);
         off += (cnt + P - 1) / P * P;
      }
      HIP_TRY(hipEventRecord(ev_reduced, comm_stream));
      HIP_TRY(hipStreamWaitEvent(e->stream, ev_reduced, 0));
      return PIPS_OK;
   }
   // finalizeKKTdense / finalizeKKTsparse: x0 diagonal, constant A0 / F0 / G0 entries, -C0^T Omega^-1 C0, link diagonal, root regularisation
   int finalize(const ScView& sc, const double* xdiag0, const double* zdiag_link) {
      Engine* e = leaves;
      const dim3 blk(256);
      if (xdiag0 && n0 > 0) hipLaunchKernelGGL(k_add_diag, dim3(grid_for(n0, 256)), blk, 0, e->stream, sc.val, sc.ld, sc.rowptr, 0, xdiag0, n0);
      if (n_fin > 0) hipLaunchKernelGGL(k_add_entries, dim3(grid_for(n_fin, 256)), blk, 0, e->stream, sc.val, d_fin_idx, d_fin_val, n_fin);
      if (mz0 > 0) {
         if (!d_zdiag0) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_factorize: mz0 > 0 needs pips_hip_kkt_set_root_inequalities + a zdiag0 vector");
         // deterministic mode: one thread walks the rows of C0 (the kernel's atomics then arrive in row order)
         hipLaunchKernelGGL(k_ctdc, e->deterministic ? dim3(1) : dim3(grid_for(mz0, 128)), e->deterministic ? dim3(1) : dim3(128), 0, e->stream, mz0,
                            d_c0_rp, d_c0_ci, d_c0_val, d_zdiag0, sc.val, sc.ld, sc.rowptr);
      }
      if (zdiag_link && mzl > 0)
         hipLaunchKernelGGL(k_add_diag, dim3(grid_for(mzl, 256)), blk, 0, e->stream, sc.val, sc.ld, sc.rowptr, n0 + my0 + myl, zdiag_link, mzl);
      if (root_reg_primal != 0.0 && n0 > 0)
         hipLaunchKernelGGL(k_add_const_diag, dim3(grid_for(n0, 256)), blk, 0, e->stream, sc.val, sc.ld, sc.rowptr, 0, n0, root_reg_primal);
      if (root_reg_dual != 0.0 && S > n0)
         hipLaunchKernelGGL(k_add_const_diag, dim3(grid_for(S - n0, 256)), blk, 0, e->stream, sc.val, sc.ld, sc.rowptr, n0, S - n0, -root_reg_dual);
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   // factorizeKKT (:1436-1464).  `factor` is the root's factor call, `rstream` the stream member it launches on.  Either on the main
   // stream (phase 13 = the root factorisation where it sits on the critical path), or on a stream of its own: the dense root - see
   // root_stream - and the sparse root alike.  The root engine's factorisation is a chain of small launches (the dissected root: 26 levels
   // of fronts + the hubs' tile): on a stream of its own it runs beside the leaf sweeps of the next solveCompressed's Lsolve
   // (root_wait() joins before Dsolve, the next factorisation, queries): 39.9 -> 38.9 ms per unit on the configs[3] shape, 43.5 -> 42.7
   // on the 256-block chain (tools/ab_async_root.sh, alternating on one box).  Default since round 5 (PIPS_HIP_SPARSE_ROOT_ASYNC=0 /
   // PIPS_HIP_ROOT_SYNC keep the main stream): round 4 had one bench run of about two dozen with it not finish inside its time limit
   // and made it opt-in; 148 full-size runs and 60 small ones in round 5 (tools/stress_exit.sh, tools/stress_async.sh, every run under a
   // watchdog) all ended, and the mechanism is the dense root's, which has been the default since round 2.
   bool root_async() const {
      const ProcessKnobs& env = knob_process();   // PIPS_HIP_ROOT_SYNC, PIPS_HIP_SPARSE_ROOT_ASYNC: once per process
      return !env.root_sync && root_own_stream && (sparse ? env.sparse_root_async : root->dist_P <= 1);   // the distributed root issues collectives: main stream
   }
   template <class Factor>
   int factor_root(hipStream_t& rstream, Factor factor) {
      Engine* e = leaves;
      int rc;
      if (!root_async()) {
         const int rec_main = timer.begin_i(e->stream, 13);
         timer.begin(e->stream, 4);
         rc = factor();
         timer.end(e->stream);
         timer.end_i(rec_main, e->stream);
         return rc;
      }
      if (!root_stream) {
         int prio_lo = 0, prio_hi = 0;
         HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
         HIP_TRY(hipStreamCreateWithPriority(&root_stream, hipStreamNonBlocking, prio_hi));
         HIP_TRY(hipEventCreateWithFlags(&ev_sc_final, hipEventDisableTiming));
         HIP_TRY(hipEventCreateWithFlags(&ev_root_done, hipEventDisableTiming));
      }
      HIP_TRY(hipEventRecord(ev_sc_final, e->stream));
      HIP_TRY(hipStreamWaitEvent(root_stream, ev_sc_final, 0));
      {
         StreamSwap on_root(rstream, root_stream);   // (put back before the test of rc: solves and queries run on the main stream)
         timer.begin(root_stream, 4);
         rc = factor();
         timer.end(root_stream);
      }
      if (rc) return rc;
      HIP_TRY(hipEventRecord(ev_root_done, root_stream));
      root_pending = true;
      return PIPS_OK;
   }
   int factorize(const double* leaf_diag, const double* xdiag0, const double* zdiag_link) {
      Engine* e = leaves;
      ++factor_gen;
      solves_since_factor = 0;
      int rc;
      timer.on = e->timer.on;
      timer.reset();
      timer.begin(e->stream, 0);
      if (leaf_diag && (rc = pips_hip_batch_set_diagonals_dev(e, leaf_diag))) return rc;
      const ScView sc = sc_view();
      if ((rc = root_wait())) return rc;                                                // the previous root factorisation still reads SC
      HIP_TRY(hipMemsetAsync(sc.val, 0, sc.count * sizeof(double), e->stream));         // initializeKKT (:840-847)
      timer.end(e->stream);
      timer.begin(e->stream, 1);
      // PIPS_HIP_FORCE_REDUCE exercises the reduction path with a one-rank communicator (tests).
      const bool reduce = n_ranks > 1 || force_reduce;
      e->defer_group_reduce = reduce && e->deterministic && e->det.global;
      rc = e->factor(sc.val, sc.ld);                                                    // children factor2 + assembleLocalKKT
      e->defer_group_reduce = false;
      if (rc) return rc;
      timer.end(e->stream);
      const int rec_reduce = timer.begin_i(e->stream, 2);   // what the main stream waits for the reduction: its exposed part
      if (reduce) {
         if (!comm) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_factorize: n_ranks > 1 needs a communicator");
         if ((rc = e->deterministic && e->det.global && e->d_gbuf ? reduce_groups(sc) : reduce_sum(sc))) return rc;
      }
      timer.end_i(rec_reduce, e->stream);
      timer.begin(e->stream, 3);
      if ((rc = finalize(sc, xdiag0, zdiag_link))) return rc;
      timer.end(e->stream);
      if (sparse) return factor_root(root_sp->stream, [this] { return root_sp->factor(nullptr, 0); });
      return factor_root(root->stream, [this, &sc] { return root->factor_dev(sc.val, S, 0); });
   }

   // ---- solveCompressed --------------------------------------------------------------------------------------------
   // what one call works on and what it decided before its first launch
   struct SolveCall {
      double *b0, *b_leaf;   // the caller's vectors: [x0 | y0 | z0 | ylink | zlink] and the leaf rows
      double* red;           // the Schur system's vector: b0, or with mz0 > 0 the reduced [x0 | y0 | ylink | zlink] (solveReducedLinkCons, sLinsysRootAug.C:397-433)
      bool capturing;        // inside a stream capture (no host-side decisions, no waits on events recorded outside)
      bool can_measure = false, joint_check = false, scheduled = false;
      bool use_aug = false, verify = false;   // both halves by sweeps of the augmented factor; measure their result
      int lsolve_steps = 0;
   };
   // Which way this call goes.  Several ranks (or the forced reduction of the tests) decide the checks together - see solve_check_every
   int solve_decide(SolveCall& c) {
      Engine* e = leaves;
      int rc;
      const bool joint = n_ranks > 1 || force_reduce;
      c.can_measure = !c.capturing && e->refine_tol > 0.0 && e->refine_steps > 0;
      // (whether the ranks exchange the outcome may depend only on what is equal on every rank: the settings the host gives all ranks alike,
      // and "some rank's analysis chose the sweeps" - the cost model decides per rank - settled once per analysis by an all-reduce)
      if (joint && c.can_measure && solve_check_every > 0 && joint_aug_gen != e->analysis_gen) {
         if (!d_flag) PIPS_TRY(d_flag.alloc(1));
         double any = e->aug_sweeps_ok ? 1.0 : 0.0;
         HIP_TRY(hipMemcpyAsync(d_flag, &any, sizeof(double), hipMemcpyHostToDevice, e->stream));
         HIP_TRY(hipStreamSynchronize(e->stream));
         if ((rc = pips_hip_allreduce_sum(comm, d_flag, 1, e->stream))) return rc;
         HIP_TRY(hipMemcpyAsync(&any, d_flag, sizeof(double), hipMemcpyDeviceToHost, e->stream));
         HIP_TRY(hipStreamSynchronize(e->stream));
         joint_aug_any = any > 0.0;
         joint_aug_gen = e->analysis_gen;
      }
      c.joint_check = joint && c.can_measure && solve_check_every > 0 && joint_aug_any;
      // Which calls measure is decided by a counter that is equal on every rank (solveCompressed calls since the factorisation; the first one
      // is always scheduled): several ranks then exchange the outcome only on scheduled calls - none could have measured on the others -
      // instead of ending every call with a latency-bound collective and two host waits.
      c.scheduled = solve_check_every > 0 && (solves_since_factor++ % solve_check_every) == 0;
      if (c.can_measure && e->aug_sweeps_ok && aug_failed_gen != factor_gen) {
         const bool validated = aug_validated_gen == factor_gen;
         const bool may_check = !joint || c.joint_check;      // (a measure may fail: several ranks must be able to act on it together)
         if (validated || (checked_witness && may_check && (!joint || c.scheduled))) {   // the first solve after a factorisation: a checked sweep pair, or the refined pass
            int pert = 1;
            if ((rc = e->perturbed_leaf_pivots(&pert))) return rc;
            c.use_aug = pert == 0;
            const bool due = c.use_aug && validated && may_check && c.scheduled;
            c.verify = c.use_aug && (!validated || due);
         }
      }
      return PIPS_OK;
   }
   // the right-hand side as the caller gave it: needed for the check, and for the refined pass if a check fails
   int save_rhs(const SolveCall& c) {
      Engine* e = leaves;
      if (!d_bsave) PIPS_TRY(d_bsave.alloc(std::max<size_t>((size_t)e->n_total, 1)));
      if (!d_b0save) PIPS_TRY(d_b0save.alloc((size_t)(S + mz0 + 1)));
      HIP_TRY(hipMemcpyAsync(d_bsave, c.b_leaf, (size_t)e->n_total * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      HIP_TRY(hipMemcpyAsync(d_b0save, c.b0, (size_t)(S + mz0) * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      return PIPS_OK;
   }
   // deterministic Lsolve: t = -sum_i Br_i^T K_i^-1 b_i is formed on its own - group-wise in block order, the (at most eight)
   // groups in the fixed tree of k_reduce_groups, the ranks' parts by the all-reduce - and added to b0 on every rank.  Guarantee:
   // run-to-run reproducibility for any rank count, and equal bits for 1 and 2 ranks (a two-operand all-reduce has one order);
   // with 4 or 8 ranks the association of the per-rank partial sums is the all-reduce's (ring / tree, per chunk), not this tree
   int lsolve_det(SolveCall& c) {
      Engine* e = leaves;
      int rc;
      timer.begin(e->stream, 5);
      if (c.use_aug) { if ((rc = e->forward_augmented_det(c.b_leaf))) return rc; }   // (the blocks' border slots hold -L_b y = -Br^T K^-1 b)
      else {
         if ((rc = e->solve(c.b_leaf))) return rc;
         c.lsolve_steps = e->last_refine_steps;
      }
      timer.end(e->stream);
      timer.begin(e->stream, 6);
      HIP_TRY(hipMemsetAsync(e->d_gvec, 0, (size_t)8 * S * sizeof(double), e->stream));
      HIP_TRY(hipMemsetAsync(e->d_tvec, 0, (size_t)S * sizeof(double), e->stream));
      if (c.use_aug) e->gather(e->g_bslot_grp, e->d_xw, e->d_gvec);
      else if (e->bt_rows_total > 0) {
         hipLaunchKernelGGL(k_border_rowdot, dim3(grid_for(e->bt_rows_total, 256)), dim3(256), 0, e->stream, e->d_bt_rowptr, e->d_bt_colidx, e->d_bval,
                            e->d_bt_xoff, c.b_leaf, e->d_bt_tmp, e->bt_rows_total, -1.0);
         e->gather(e->g_btm_grp, e->d_bt_tmp, e->d_gvec);
      }
      const dim3 grid(std::max(1, std::min(64, (S + 255) / 256)), 1);
      if (e->det.global && n_ranks > 1) {   // all eight group slots on every rank, one tree (see reduce_groups)
         if (!d_gvec_all) PIPS_TRY(d_gvec_all.alloc((size_t)8 * S));
         HIP_TRY(hipMemsetAsync(d_gvec_all, 0, (size_t)8 * S * sizeof(double), e->stream));
         HIP_TRY(hipMemcpyAsync(d_gvec_all + (size_t)e->det.first_slot * S, e->d_gvec, (size_t)e->det.n_groups * S * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
         if ((rc = pips_hip_all_gather(comm, d_gvec_all, (size_t)e->det.slots * S, 8 / e->det.slots, e->stream))) return rc;
         hipLaunchKernelGGL(k_reduce_groups, grid, dim3(256), 0, e->stream, e->d_tvec, S, S, d_gvec_all, (long long)S, 8, 0);
      } else {
         hipLaunchKernelGGL(k_reduce_groups, grid, dim3(256), 0, e->stream, e->d_tvec, S, S, e->d_gvec, (long long)S, e->det.n_groups, e->det.first_slot);
         if ((n_ranks > 1 || force_reduce) && (rc = pips_hip_allreduce_sum(comm, e->d_tvec, (size_t)S, e->stream))) return rc;
      }
      hipLaunchKernelGGL(k_axpy, dim3(grid_for(S, 256)), dim3(256), 0, e->stream, c.red, e->d_tvec, 1.0, (long long)S);
      timer.end(e->stream);
      return PIPS_OK;
   }
   // Lsolve: ranks > 0 zero b0, every child adds -Br^T K^-1 b_i, all-reduce (sLinsysRootAug.C:323-344)
   int lsolve_atomic(SolveCall& c) {
      Engine* e = leaves;
      int rc;
      if (n_ranks > 1 && rank > 0) HIP_TRY(hipMemsetAsync(c.red, 0, (size_t)S * sizeof(double), e->stream));
      timer.begin(e->stream, 5);
      if (c.use_aug) { if ((rc = e->forward_augmented(c.b_leaf, c.red))) return rc; }
      else {
         if ((rc = e->solve(c.b_leaf))) return rc;
         c.lsolve_steps = e->last_refine_steps;
      }
      timer.end(e->stream);
      timer.begin(e->stream, 6);
      if (!c.use_aug && (rc = pips_hip_batch_border_tmult_dev(e, c.b_leaf, c.red, -1.0))) return rc;
      if ((n_ranks > 1 || force_reduce) && (rc = pips_hip_allreduce_sum(comm, c.red, (size_t)S, e->stream))) return rc;
      timer.end(e->stream);
      return PIPS_OK;
   }
   // Dsolve: eliminate z0 through C0, solve with the Schur complement, recover z0 and put the caller's vector together again
   // (solveReducedLinkCons :384-466)
   int dsolve(const SolveCall& c) {
      Engine* e = leaves;
      int rc;
      const int head = n0 + my0, tailn = myl + mzl;
      // the join with the root's stream is a phase of its own (11): what the main stream waits there is the part of the root factorisation
      // that the first Lsolve did not hide - the exposed root time, measured instead of estimated
      if (!c.capturing) {   // (a captured sequence: joined before the capture began)
         const bool pending = root_pending;
         if (pending) timer.begin(e->stream, 11);
         if ((rc = root_wait())) return rc;
         if (pending) timer.end(e->stream);
      }
      timer.begin(e->stream, 7);
      if (mz0 > 0)
         hipLaunchKernelGGL(k_z0_elim, e->deterministic ? dim3(1) : dim3(grid_for(mz0, 128)), e->deterministic ? dim3(1) : dim3(128), 0, e->stream, 0, mz0, d_c0_rp, d_c0_ci, d_c0_val,
                            d_zdiag0, c.b0 + head, c.red);
      if ((rc = sparse ? root_sp->solve(c.red) : root->solve_dev(c.red))) return rc;
      if (mz0 > 0) {
         hipLaunchKernelGGL(k_z0_elim, dim3(grid_for(mz0, 128)), dim3(128), 0, e->stream, 1, mz0, d_c0_rp, d_c0_ci, d_c0_val, d_zdiag0, c.b0 + head, c.red);
         HIP_TRY(hipMemcpyAsync(c.b0, c.red, (size_t)head * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
         HIP_TRY(hipMemcpyAsync(c.b0 + head + mz0, c.red + head, (size_t)tailn * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      }
      timer.end(e->stream);
      return PIPS_OK;
   }
   // Ltsolve by the backward sweep of the augmented factor, and - where this call verifies - the measure of the pair's result:
   // r_i = (b_i - Br_i x0) - K_i x_i over the blocks, measured like a refinement step would measure it (phase 12)
   int ltsolve_sweeps(const SolveCall& c, bool& failed) {
      Engine* e = leaves;
      int rc;
      timer.begin(e->stream, 8);
      if ((rc = e->backward_augmented(c.red, c.b_leaf))) return rc;
      last_ltsolve_from_factor = true;
      last_solve_path = 2;
      if (c.verify) {
         timer.end(e->stream);
         timer.begin(e->stream, 12);
         double worst = 0.0;
         if (e->can_measure_fused()) {
            if ((rc = e->residual_measure_fused(d_bsave, c.red, c.b_leaf, &worst))) return rc;
         } else {
            HIP_TRY(hipMemcpyAsync(d_t, d_bsave, (size_t)e->n_total * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
            if ((rc = pips_hip_batch_border_mult_dev(e, c.red, d_t, -1.0))) return rc;
            if ((rc = e->residual_measure(d_t, c.b_leaf, &worst))) return rc;
         }
         ++checked_solves;
         sweeps_since_check = 0;
         if (worst <= e->refine_tol) {
            aug_validated_gen = factor_gen;
            last_solve_path = 3;
         } else
            failed = true;   // not good enough without refinement: the refined path on the saved right-hand side, no sweeps on these factors
      }
      timer.end(e->stream);
      return PIPS_OK;
   }
   // Ltsolve: b_i -= K_i^-1 Br_i x0 (LniTransMult, DistributedLinearSystem.C:430-483).  Where the stored border rows are thin
   // enough and no pivot of the factorisation was perturbed: from the augmented factor with one backward sweep
   // (Engine::solve_border_backward); else border product + full solve with refinement.
   // The sweep carries no refinement, so it is taken only on evidence that the factors are accurate: no perturbed pivot (the
   // counters reached pinned memory with the factorisation: no wait for the solves queued behind it) AND, with adaptive refinement,
   // the refined leaf solve of this call's Lsolve - same factors - was satisfied by its first solve (backward error below the
   // tolerance without a step).  A pivot that kept its sign but is rounding noise passes the first test, not the second.
   int ltsolve_refined(const SolveCall& c) {
      Engine* e = leaves;
      int rc;
      timer.begin(e->stream, 8);
      if (!c.capturing) {
         int pert = 1;
         if ((e->border_backward_ok || e->aug_sweeps_ok) && (rc = e->perturbed_leaf_pivots(&pert))) return rc;
         const bool lsolve_clean = e->refine_tol > 0.0 ? e->last_refine_steps == 0 : true;
         last_ltsolve_from_factor = e->border_backward_ok && pert == 0 && lsolve_clean;   // (dense or sparse root: x0 comes in Schur numbering either way)
      }
      int ltsolve_steps = 0;
      if (last_ltsolve_from_factor) {
         if ((rc = e->solve_border_backward(c.red, d_t))) return rc;
      } else {
         HIP_TRY(hipMemsetAsync(d_t, 0, (size_t)e->n_total * sizeof(double), e->stream));
         if ((rc = pips_hip_batch_border_mult_dev(e, c.red, d_t, 1.0))) return rc;
         if ((rc = e->solve(d_t))) return rc;
         ltsolve_steps = e->last_refine_steps;
      }
      last_solve_path = last_ltsolve_from_factor ? 1 : 0;
      // this refined pass is the witness for the factors it ran on (see aug_validated_gen)
      // (a pass that was allowed no step proves nothing: refine_steps > 0)
      if (c.can_measure && e->aug_sweeps_ok && c.lsolve_steps == 0 && ltsolve_steps == 0) aug_validated_gen = factor_gen;
      timer.end(e->stream);
      timer.begin(e->stream, 9);
      hipLaunchKernelGGL(k_axpy, dim3(grid_for(e->n_total, 256)), dim3(256), 0, e->stream, c.b_leaf, d_t, -1.0, e->n_total);
      timer.end(e->stream);
      return PIPS_OK;
   }
   // the joint decision at the end of the call: any rank's failed check sends every rank back to its saved right-hand side
   int settle(const SolveCall& c, bool my_check_failed) {
      Engine* e = leaves;
      bool redo = my_check_failed;
      if (c.joint_check) {
         if (!d_flag) PIPS_TRY(d_flag.alloc(1));
         if (!h_flag) PIPS_TRY(h_flag.alloc(2));
         h_flag[0] = my_check_failed ? 1.0 : 0.0;   // (pinned: the copy is queued, nothing waits before the collective)
         HIP_TRY(hipMemcpyAsync(d_flag, h_flag, sizeof(double), hipMemcpyHostToDevice, e->stream));
         if (int rcf = pips_hip_allreduce_sum(comm, d_flag, 1, e->stream)) return rcf;
         HIP_TRY(hipMemcpyAsync(h_flag + 1, d_flag, sizeof(double), hipMemcpyDeviceToHost, e->stream));
         HIP_TRY(hipStreamSynchronize(e->stream));
         redo = h_flag[1] > 0.0;
      }
      if (!redo) return PIPS_OK;
      ++failed_checks;
      aug_failed_gen = factor_gen;   // no sweeps on these factors any more, on any rank
      HIP_TRY(hipMemcpyAsync(c.b_leaf, d_bsave, (size_t)e->n_total * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      HIP_TRY(hipMemcpyAsync(c.b0, d_b0save, (size_t)(S + mz0) * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      return solve_enqueue(c.b0, c.b_leaf, c.capturing);
   }
   // the launch sequence of one solveCompressed
   int solve_enqueue(double* b0_dev, double* b_leaf_dev, bool capturing) {
      Engine* e = leaves;
      int rc;
      SolveCall c{b0_dev, b_leaf_dev, b0_dev, capturing};
      if (mz0 > 0) {
         const int head = n0 + my0, tailn = myl + mzl;
         c.red = d_red;
         HIP_TRY(hipMemcpyAsync(c.red, b0_dev, (size_t)head * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
         HIP_TRY(hipMemcpyAsync(c.red + head, b0_dev + head + mz0, (size_t)tailn * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      }
      if ((rc = solve_decide(c))) return rc;
      if ((c.verify || c.joint_check) && (rc = save_rhs(c))) return rc;
      if ((rc = e->deterministic && e->d_gvec ? lsolve_det(c) : lsolve_atomic(c))) return rc;
      if ((rc = dsolve(c))) return rc;
      bool failed = false;
      if ((rc = c.use_aug ? ltsolve_sweeps(c, failed) : ltsolve_refined(c))) return rc;
      if (failed || (c.joint_check && c.scheduled)) return settle(c, failed);   // (refined pass: another rank's check may have failed)
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   // solveCompressed as a replayed HIP graph (pips_hip_kkt_set_solve_graph): the launch sequence of one call is
   // fixed between factorisations - dozens of launches on a launch-bound problem (configs[0]: ~50 kernels of a few microseconds each) -
   // so it is captured once per (right-hand-side pointers, Ltsolve path) and replayed.  What a capture cannot contain keeps the
   // direct path: adaptive refinement (it reads norms on the host between steps), reductions over several ranks, the sparse root,
   // deterministic mode, phase timing.  The single-launch sweeps take their epoch from device memory for this (k_sweep_bump).
   bool graph_eligible() const {
      const Engine* e = leaves;
      return solve_graph && !sparse && n_ranks <= 1 && !force_reduce && e->refine_tol == 0.0 && !e->deterministic && !e->timer.on && !timer.on;
   }
   int solve_compressed(double* b0_dev, double* b_leaf_dev) {
      Engine* e = leaves;
      if (!graph_eligible()) return solve_enqueue(b0_dev, b_leaf_dev, false);
      int rc;
      // host-side decisions and joins first: they are part of the key, not of the graph
      if ((rc = root_wait())) return rc;
      int pert = 1;
      if (e->border_backward_ok && (rc = e->perturbed_leaf_pivots(&pert))) return rc;
      last_ltsolve_from_factor = e->border_backward_ok && pert == 0;
      GraphKey key;
      key.b0 = b0_dev; key.bl = b_leaf_dev; key.zdiag0 = d_zdiag0; key.c0_val = d_c0_val; key.c0_rp = d_c0_rp; key.c0_ci = d_c0_ci;
      key.from_factor = last_ltsolve_from_factor ? 1 : 0; key.refine_steps = e->refine_steps; key.refine_mode = e->refine_mode; key.mz0 = mz0;
      key.pivoting = root ? root->pivoting : 0; key.analysis_gen = e->analysis_gen;
      key.bk_gen = root ? root->bk_refactorizations : 0;   // (a new pivot order: the solve permutes its right-hand side)
      if (graph_exec && !(graph_key == key)) {
         (void)hipGraphExecDestroy(graph_exec);
         graph_exec = nullptr;
      }
      if (!graph_exec) {
         // The capture runs on a stream of its own (the handle's stream may be the legacy default stream, which cannot be captured):
         // the engine's and the root's stream members point there for the duration of the enqueue; the graph is then launched into the
         // handle's own stream like any other work.
         if (!graph_stream) HIP_TRY(hipStreamCreateWithFlags(&graph_stream, hipStreamNonBlocking));
         hipGraph_t g = nullptr;
         hipError_t ec;
         {
            StreamSwap leaves_on_graph(e->stream, graph_stream), root_on_graph(root->stream, graph_stream);
            const hipError_t eb = hipStreamBeginCapture(graph_stream, hipStreamCaptureModeRelaxed);
            rc = eb == hipSuccess ? solve_enqueue(b0_dev, b_leaf_dev, true) : PIPS_OK;
            ec = eb == hipSuccess ? hipStreamEndCapture(graph_stream, &g) : eb;
         }
         if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
         if (ec != hipSuccess || !g) PIPS_FAIL(PIPS_ERR_HIP, "pips_hip_kkt_solve_compressed: stream capture failed: %s", hipGetErrorString(ec));
         const hipError_t ei = hipGraphInstantiate(&graph_exec, g, nullptr, nullptr, 0);
         (void)hipGraphDestroy(g);
         if (ei != hipSuccess) { graph_exec = nullptr; PIPS_FAIL(PIPS_ERR_HIP, "pips_hip_kkt_solve_compressed: hipGraphInstantiate: %s", hipGetErrorString(ei)); }
         graph_key = key;
         ++graph_captures;
      }
      HIP_TRY(hipGraphLaunch(graph_exec, e->stream));
      ++graph_replays;
      return PIPS_OK;
   }

   // ---- solveCompressed for several right-hand sides (pips_hip_kkt_solve_compressed_multi) ---------------------------------------------
   // = sLinsysRootAug::addBlTKiInvBrToResBlockwise's LsolveHierarchyBorder / DsolveHierarchyBorder / LtsolveHierarchyBorder on a buffer of
   // columns (sLinsysRootAug.C:1815-1940).  Below Engine::multi_knob().from columns the call IS the sequence of solve_compressed calls,
   // state and all.  From there on: the refined way 0 on panels, chunk by chunk (multiplan.h) - leaves->solve_multi, the border products
   // of borderpanel.hip.h, the root's solve_multi_dev / solve_multi.  The panel path takes no augmented sweep, captures no graph and leaves
   // what the single path decides by alone: solves_since_factor, aug_validated_gen, aug_failed_gen, last_solve_path,
   // last_ltsolve_from_factor, the check counters, the phase timer.
   DevBuf<double> d_pw;       // W = Br X0, n_total x nr (the budget of the chunks)
   DevBuf<double> d_pt;       // T = -sum_i Br_i^T Z_i, S x nr: [s][q] under the atomics, [q][s] in deterministic mode
   DevBuf<double> d_pred;     // mz0 > 0: the reduced panel [x0 | y0 | ylink | zlink], S x nr
   DevBuf<double> d_pdot;     // deterministic mode: the row dots, bt_rows_total x nr
   DevBuf<double> d_pg, d_pg_all;   // ... and the group panels (this rank's / all eight), 8 x nr x S
   DevBuf<double> d_pn;
   long long multi_info[6] = {0, 0, 0, 0, 0, 0};   // pips_hip_kkt_solve_multi_info
   long long panel_nt_max = 0, panel_nt_gen = -1;
   // the longest leaf vector of any rank: every rank cuts the same chunks (each ends in collectives of S x chunk doubles).  Once per analysis
   int panel_n_total(long long* out) {
      Engine* e = leaves;
      *out = e->n_total;
      if (n_ranks <= 1) return PIPS_OK;
      if (!comm) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_solve_compressed_multi: n_ranks > 1 needs a communicator");
      if (panel_nt_gen != e->analysis_gen) {
         std::vector<double> h((size_t)n_ranks, 0.0);
         h[(size_t)rank] = (double)e->n_total;
         PIPS_TRY(d_pn.reserve((size_t)n_ranks));
         HIP_TRY(hipMemcpyAsync(d_pn, h.data(), (size_t)n_ranks * sizeof(double), hipMemcpyHostToDevice, e->stream));
         HIP_TRY(hipStreamSynchronize(e->stream));
         if (int rc = pips_hip_allreduce_sum(comm, d_pn, (size_t)n_ranks, e->stream)) return rc;
         HIP_TRY(hipMemcpyAsync(h.data(), d_pn, (size_t)n_ranks * sizeof(double), hipMemcpyDeviceToHost, e->stream));
         HIP_TRY(hipStreamSynchronize(e->stream));
         panel_nt_max = (long long)*std::max_element(h.begin(), h.end());
         panel_nt_gen = e->analysis_gen;
      }
      *out = panel_nt_max;
      return PIPS_OK;
   }
   // one chunk of nr columns: B0 + q ld0 and BL + q ldl, q < nr
   int solve_panel(int nr, double* B0, long long ld0, double* BL, long long ldl) {
      Engine* e = leaves;
      int rc;
      const int head = n0 + my0, tailn = myl + mzl;
      const bool reduce = n_ranks > 1 || force_reduce;
      const bool det = e->deterministic && e->d_gvec;
      const size_t col = sizeof(double);
      const long long sn = (long long)S * nr;
      if (reduce && !comm) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_kkt_solve_compressed_multi: n_ranks > 1 needs a communicator");
      // 1. root inequalities: the reduced panel, as solve_enqueue copies one vector
      double* red = B0;
      long long ldr = ld0;
      if (mz0 > 0) {
         PIPS_TRY(d_pred.reserve((size_t)sn));
         red = d_pred; ldr = S;
         if (head > 0) HIP_TRY(hipMemcpy2DAsync(red, (size_t)ldr * col, B0, (size_t)ld0 * col, (size_t)head * col, nr, hipMemcpyDeviceToDevice, e->stream));
         if (tailn > 0)
            HIP_TRY(hipMemcpy2DAsync(red + head, (size_t)ldr * col, B0 + head + mz0, (size_t)ld0 * col, (size_t)tailn * col, nr, hipMemcpyDeviceToDevice, e->stream));
      }
      // 2. Lsolve: Z = K^-1 B_leaf; T = -sum_i Br_i^T Z_i formed on its own, summed over the ranks, added to the reduced panel on every rank
      if ((rc = e->solve_multi(BL, nr, ldl))) return rc;
      multi_info[3] = e->last_refine_steps;
      PIPS_TRY(d_pt.reserve((size_t)sn));
      HIP_TRY(hipMemsetAsync(d_pt, 0, (size_t)sn * col, e->stream));
      const dim3 bt_grid(grid_for(e->bt_rows_total * BT_LANES, 256, 65536));
      const dim3 vec_grid((unsigned)std::max(1LL, std::min(1024LL, (sn + 255) / 256)), 1);
      if (det) {
         const long long gstride = sn;
         PIPS_TRY(d_pg.reserve((size_t)8 * sn));
         HIP_TRY(hipMemsetAsync(d_pg, 0, (size_t)8 * sn * col, e->stream));
         if (e->bt_rows_total > 0) {
            PIPS_TRY(d_pdot.reserve((size_t)e->bt_rows_total * nr));
            HIP_TRY(hipMemsetAsync(d_pdot, 0, (size_t)e->bt_rows_total * nr * col, e->stream));
            hipLaunchKernelGGL(k_border_tmult_panel<true>, bt_grid, dim3(256), 0, e->stream, e->d_bt_rowptr, e->d_bt_colidx, e->d_bval, e->d_bt_rowsc,
                               e->d_bt_xoff, BL, ldl, nr, d_pdot, (long long)nr, e->bt_rows_total, -1.0);
            const Engine::GatherList& g = e->g_btm_grp;
            if (g.n_targets > 0)
               hipLaunchKernelGGL(k_gather_rows_panel, dim3(grid_for(g.n_targets * nr, 256, 65536)), dim3(256), 0, e->stream, g.n_targets, g.d_tgt, g.d_off,
                                  g.d_slots, d_pdot, (long long)nr, nr, S, d_pg, gstride);
         }
         // the group panels in the fixed tree of k_reduce_groups (a panel as one vector of S nr entries), as lsolve_det adds the group vectors
         if (e->det.global && n_ranks > 1) {
            PIPS_TRY(d_pg_all.reserve((size_t)8 * sn));
            HIP_TRY(hipMemsetAsync(d_pg_all, 0, (size_t)8 * sn * col, e->stream));
            HIP_TRY(hipMemcpyAsync(d_pg_all + (size_t)e->det.first_slot * sn, d_pg, (size_t)e->det.n_groups * sn * col, hipMemcpyDeviceToDevice, e->stream));
            if ((rc = pips_hip_all_gather(comm, d_pg_all, (size_t)e->det.slots * sn, 8 / e->det.slots, e->stream))) return rc;
            hipLaunchKernelGGL(k_reduce_groups, vec_grid, dim3(256), 0, e->stream, d_pt, 0, (int)sn, d_pg_all, gstride, 8, 0);
         } else {
            hipLaunchKernelGGL(k_reduce_groups, vec_grid, dim3(256), 0, e->stream, d_pt, 0, (int)sn, d_pg, gstride, e->det.n_groups, e->det.first_slot);
            if (reduce && (rc = pips_hip_allreduce_sum(comm, d_pt, (size_t)sn, e->stream))) return rc;
         }
         hipLaunchKernelGGL(k_panel_add, vec_grid, dim3(256), 0, e->stream, red, ldr, d_pt, 1LL, (long long)S, S, nr);
      } else {
         launch_border_tmult_panel(e, BL, ldl, nr, d_pt, (long long)nr, -1.0);
         if (reduce && (rc = pips_hip_allreduce_sum(comm, d_pt, (size_t)sn, e->stream))) return rc;
         hipLaunchKernelGGL(k_panel_add, vec_grid, dim3(256), 0, e->stream, red, ldr, d_pt, (long long)nr, 1LL, S, nr);
      }
      // 3. Dsolve: z0 elimination on the panel, the root's panel solve, z0 recovered, the caller's columns put together again
      if ((rc = root_wait())) return rc;
      if (mz0 > 0)
         hipLaunchKernelGGL(k_z0_elim_panel, e->deterministic ? dim3(1, nr) : dim3(grid_for(mz0, 128), nr), e->deterministic ? dim3(1) : dim3(128), 0, e->stream, 0,
                            mz0, d_c0_rp, d_c0_ci, d_c0_val, d_zdiag0, B0 + head, ld0, red, ldr);
      if ((rc = sparse ? root_sp->solve_multi(red, nr, ldr) : root->solve_multi_dev(red, nr, ldr))) return rc;
      if (mz0 > 0) {
         hipLaunchKernelGGL(k_z0_elim_panel, dim3(grid_for(mz0, 128), nr), dim3(128), 0, e->stream, 1, mz0, d_c0_rp, d_c0_ci, d_c0_val, d_zdiag0, B0 + head, ld0, red,
                            ldr);
         if (head > 0) HIP_TRY(hipMemcpy2DAsync(B0, (size_t)ld0 * col, red, (size_t)ldr * col, (size_t)head * col, nr, hipMemcpyDeviceToDevice, e->stream));
         if (tailn > 0)
            HIP_TRY(hipMemcpy2DAsync(B0 + head + mz0, (size_t)ld0 * col, red + head, (size_t)ldr * col, (size_t)tailn * col, nr, hipMemcpyDeviceToDevice, e->stream));
      }
      // 4. Ltsolve: W = Br X0 (every row of W is written), W = K^-1 W, B_leaf -= W
      PIPS_TRY(d_pw.reserve((size_t)std::max<long long>(e->n_total, 1) * nr));
      if ((rc = launch_border_mult_panel(e, red, ldr, nr, d_pw, e->n_total, 1.0))) return rc;
      if ((rc = e->solve_multi(d_pw, nr, e->n_total))) return rc;
      multi_info[4] = e->last_refine_steps;
      hipLaunchKernelGGL(k_maxpy, dim3(grid_for(e->n_total, 256, 1024), nr), dim3(256), 0, e->stream, BL, ldl, d_pw, e->n_total, -1.0, e->n_total);
      ++multi_info[5];
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
   int solve_compressed_multi(int nrhs, double* B0, long long ld0, double* BL, long long ldl) {
      Engine* e = leaves;
      int rc;
      const int from = Engine::multi_knob().from;
      const bool panels = from > 0 && nrhs >= from;
      long long nt = e->n_total;
      if (panels && (rc = panel_n_total(&nt))) return rc;
      const std::vector<KktMultiChunk> plan = kkt_multi_plan(nrhs, from, Engine::MULTI_CHUNK_MAX, nt, KKT_MULTI_BUDGET_BYTES);
      multi_info[0] = panels ? 1 : 0;
      multi_info[1] = (long long)plan.size();
      multi_info[2] = plan.empty() ? 0 : plan[0].count;
      multi_info[3] = multi_info[4] = 0;
      for (const KktMultiChunk& c : plan) {
         double* b0 = B0 + (long long)c.first * ld0;
         double* bl = BL + (long long)c.first * ldl;
         if ((rc = c.path == 0 ? solve_compressed(b0, bl) : solve_panel(c.count, b0, ld0, bl, ldl))) return rc;
      }
      return PIPS_OK;
   }
};
