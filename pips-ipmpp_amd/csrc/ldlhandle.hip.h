// The per-leaf solver handles behind pips_hip_ldl_* (INTEGRATION.md levels 1, 1.5, 1.5b): a client of Engine - factor, solve, solve_multi,
// set_sc_tables, set_det_groups, sweep.take_error and a few of its buffers.  Included once by engine.hip, inside its extern "C" block, after
// the pips_hip_batch_* entries.
#pragma once

// ---- single leaf solver handle -------------------------------------------------------------------------------------
struct LdlGroup;
// pips_hip_ldl_factor_schur of single handles: the leaf kernels address the Schur complement as a dense S x S array, but a leaf only touches
// the nb x nb entries of its non-empty border columns - one S x S scratch array per DEVICE serves every handle (a call leaves it with a
// stream synchronisation; 64 handles with an array each were 32 GB at S = 8000), and only the compact nb x nb block travels to the host.
struct SchurScratch {
   std::mutex mu;
   std::map<int, DevBuf<double>> per_device;   // device -> array
};
static SchurScratch& g_schur_scratch = *new SchurScratch;   // (never destroyed: nothing is freed while the process exits)

// C[i + j * nb] = SC[bm[i] + bm[j] * ld] (the block of a leaf's border columns, column-major; the lower triangle is what the caller reads) -
// and SC is left zero on the whole block, whichever triangle a Schur mode wrote
__global__ void k_schur_take_block(double* __restrict__ SC, int ld, const int* __restrict__ bm, int nb, double* __restrict__ C) {
   const int j = blockIdx.y;
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += gridDim.x * blockDim.x) {
      double* p = SC + bm[i] + (long long)bm[j] * ld;
      C[i + (long long)j * nb] = *p;
      *p = 0.0;
   }
}

// Where a handle's (or a bound group's) Schur term goes: the caller's dense S x S matrix (pips_hip_ldl_factor_schur / _batch) or its
// sparse one (pips_hip_ldl_factor_schur_sparse / _batch).  The first call with a Schur complement settles it for the handle's life: the
// sparse entries move the kernels' targets into position tables (Engine::set_sc_tables), the dense ones address S x S.
enum { SC_KIND_NONE = 0, SC_KIND_DENSE = 1, SC_KIND_SPARSE = 2 };
// The sparse target (schurtarget.h): T doubles on the device, the T positions they belong to in the caller's value array, and what
// identifies the pattern in later calls - nothing of size S x S or nnz
struct SparseSchurBind {
   bool bound = false;
   SchurPatternId id;
   std::vector<long long> pos;
   DevBuf<double> d_val;
   std::vector<double> h_val;
};

struct LdlHandle {
   Engine eng;
   // staging of the host-pointer solves, kept between calls (declared after eng: freed before its stream goes; a handle's n never
   // changes, so they outlive a re-analysis)
   DevBuf<double> d_hostx;        // device copy of host right-hand sides (pips_hip_ldl_solve, pips_hip_ldl_solve_sparse)
   DevBuf<double> d_hostpack;     // packed rows + their indices of pips_hip_ldl_solve_sparse
   int sc_kind = SC_KIND_NONE;
   SparseSchurBind sparse_sc;
   DevBuf<double> d_sc;           // compact nb x nb Schur term of this leaf (pips_hip_ldl_factor_schur)
   std::vector<double> h_sc;
   std::shared_ptr<LdlGroup> group;   // the leaves of a rank bound into one batch engine (pips_hip_ldl_factor_schur_batch)
   int group_index = -1;
   // which engine holds this leaf's NEWEST factors: the batch's (set for every member by pips_hip_ldl_factor_schur_batch) or the handle's
   // own (pips_hip_ldl_factor / _factor_schur clear it) - a handle can go through both over its life (matrixChanged() alone, later the
   // host's loop handed over), and solve / inertia must never answer from the older of the two
   bool newest_in_group = false;
   ~LdlHandle();
};
// Array-of-handles entries (INTEGRATION.md level 1.5b): the reference keeps one DoubleLinearSolver per leaf and loops over its children
// (sLinsysRootAug::assembleLocalKKT :210-227, Lsolve / Ltsolve :323-365).  One leaf alone is a latency chain on the device (64 leaves of
// configs[1] one after the other: 1.17 s per factorisation against 0.1 s as one batch), so the handles of a rank can be bound into ONE batch
// engine: the patterns and borders the handles were given, analysed together; factor_schur_batch / solve_batch then run all leaves in every
// launch, one S x S Schur buffer on the device and one transfer of it per factorisation instead of one per leaf.
struct LdlGroup {
   Engine eng;
   std::vector<LdlHandle*> members;
   DevBuf<double> d_sc, d_x;
   std::vector<double> h_sc;
   int sc_kind = SC_KIND_NONE;
   SparseSchurBind sparse_sc;
};
// a handle that goes away leaves an empty slot in its group: the siblings keep the batch's factors (their own solves go through
// group_solve_rows, which needs no sibling), the next array-of-handles call sees another array and binds anew
LdlHandle::~LdlHandle() {
   if (group && group_index >= 0 && group_index < (int)group->members.size() && group->members[group_index] == this) group->members[group_index] = nullptr;
}
// array-of-handles solves / queries answer from the batch's factors: refuse if a member has been factorised alone since
static int ldl_group_is_current(const LdlGroup& g, const char* who) {
   if (!g.eng.factored) PIPS_FAIL(PIPS_ERR_STATE, "%s: pips_hip_ldl_factor_schur_batch first", who);
   for (size_t i = 0; i < g.members.size(); ++i)
      if (g.members[i] && !g.members[i]->newest_in_group)
         PIPS_FAIL(PIPS_ERR_STATE, "%s: handle %d was factorised on its own after the batch's factorisation - factorise the array again", who, (int)i);
   return PIPS_OK;
}
static inline bool ldl_uses_group(const LdlHandle* h) { return h->group && h->newest_in_group && h->group->eng.factored; }
// one member's right-hand sides through the batch engine (every block in every launch, the others with zeros - correct, and as long as
// a batch solve: hosts that loop over their leaves should hand the loop over, pips_hip_ldl_solve_batch).  rhs: nrhs rows of length ld,
// on the host or on the device
static int group_solve_rows(LdlGroup& g, int index, int nrhs, double* rhs, long long ld, bool on_device, const char* who) {
   Engine& e = g.eng;
   HIP_TRY(hipSetDevice(e.device));
   if (!g.d_x) PIPS_TRY(g.d_x.alloc((size_t)std::max<long long>(e.n_total, 1)));
   const size_t cnt = (size_t)(e.x_off[index + 1] - e.x_off[index]) * sizeof(double);
   for (int r = 0; r < nrhs; ++r) {
      HIP_TRY(hipMemsetAsync(g.d_x, 0, (size_t)e.n_total * sizeof(double), e.stream));
      HIP_TRY(hipMemcpyAsync(g.d_x + e.x_off[index], rhs + (size_t)r * ld, cnt, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e.stream));
      int rc = e.solve(g.d_x);
      if (rc) return rc;
      HIP_TRY(hipMemcpyAsync(rhs + (size_t)r * ld, g.d_x + e.x_off[index], cnt, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e.stream));
   }
   if (!on_device) HIP_TRY(hipStreamSynchronize(e.stream));
   return e.sweep.take_error(who);
}

int pips_hip_ldl_create(void** handle, int n, const int* krow, const int* jcol, int device, int flags) {
   (void)flags;
   if (!handle || n <= 0 || !krow || !jcol) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_create: bad arguments");
   auto h = std::make_unique<LdlHandle>();
   h->eng.nblk = 1;
   h->eng.S = 0;
   h->eng.device = device;
   h->eng.in.assign(1, BlockInput());
   BlockInput& in = h->eng.in[0];
   in.n = n;
   in.krow.assign(krow, krow + n + 1);
   in.kcol.assign(jcol, jcol + krow[n]);
   *handle = h.release();
   return PIPS_OK;
}

int pips_hip_ldl_set_inertia_hint(void* handle, int n_primal) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   h->eng.in[0].n_primal = n_primal;
   return PIPS_OK;
}

int pips_hip_ldl_set_pivot_rule(void* handle, double thr_rel, double repl_rel) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   h->eng.thr_rel = thr_rel;
   h->eng.repl_rel = repl_rel;
   return PIPS_OK;
}

int pips_hip_ldl_set_refinement(void* handle, int max_steps, double tol) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   h->eng.refine_steps = max_steps;
   h->eng.refine_tol = tol;
   h->eng.refine_mode = 0;
   return PIPS_OK;
}

int pips_hip_ldl_set_deterministic(void* handle, int on) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   if (h->eng.analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_set_deterministic: before the first factorisation (the symbolic phase builds the slot lists)");
   h->eng.deterministic = on != 0;
   return PIPS_OK;
}

int pips_hip_ldl_set_refinement_backward_error(void* handle, int max_steps, double tol) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || max_steps < 0 || tol < 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_set_refinement_backward_error: bad arguments");
   h->eng.refine_steps = max_steps;
   h->eng.refine_tol = tol;
   h->eng.refine_mode = 1;
   return PIPS_OK;
}

int pips_hip_ldl_analyze(void* handle) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   return pips_hip_batch_analyze(&h->eng, 1);
}

int pips_hip_ldl_factor(void* handle, const double* vals_host) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || !vals_host) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_factor: bad arguments");
   if (!h->eng.analyzed) {
      int rc = pips_hip_ldl_analyze(handle);
      if (rc) return rc;
   }
   int rc = pips_hip_batch_set_values(&h->eng, 0, vals_host);
   if (rc) return rc;
   rc = h->eng.factor(nullptr, 0);
   if (rc) return rc;
   h->newest_in_group = false;      // (the batch's copy of this leaf is the older one now)
   HIP_TRY(hipStreamSynchronize(h->eng.stream));
   return PIPS_OK;
}

// The values alone: the twin of pips_hip_batch_set_values for a leaf handle.  The factors stay as they are - the solve sweeps read only
// them - and the residual and the measure of the refinement read the new values: later solves refine against these values with the
// factors they have.  (A handle whose newest factors are a group's has its values there, not here.)
int pips_hip_ldl_set_values(void* handle, const double* K_val_host) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || !K_val_host) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_set_values: bad arguments");
   if (ldl_uses_group(h)) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_set_values: the newest factors of this handle are a batch's (pips_hip_ldl_factor_schur_batch)");
   if (!h->eng.factored) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_set_values: factor first");
   return pips_hip_batch_set_values(&h->eng, 0, K_val_host);
}

// The leaf's Schur term without dense border columns over PCIe.  The border Br_i^T (S x n CSR, rows = Schur column ids: the
// reference's border_left_transp, DistributedLeafLinearSystem.C:214-252) is declared before the analysis; factor_schur factorises
// K_i and adds  -Br_i^T K_i^-1 Br_i  to the caller's Schur complement: what the K4-K6 chunk loop
// (addBiTLeftKiBiRightToResBlockedParallelSolvers, DistributedLinearSystem.C:766-1047: densify <= 20 T border columns,
// solve(nrhs, ...), sparse product back) computes, but with only the CSR values going up and the S x S term coming down.
int pips_hip_ldl_set_border(void* handle, int S, const int* Bt_rowptr, const int* Bt_colidx) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || S <= 0 || !Bt_rowptr || !Bt_colidx) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_set_border: bad arguments");
   if (h->eng.analyzed) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_set_border: declare the border before pips_hip_ldl_analyze / the first factor");
   BlockInput& in = h->eng.in[0];
   for (int p = 0; p < Bt_rowptr[S]; ++p)
      if (Bt_colidx[p] < 0 || Bt_colidx[p] >= in.n) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_set_border: column %d outside the leaf (n = %d)", Bt_colidx[p], in.n);
   h->eng.S = S;
   in.btrow.assign(Bt_rowptr, Bt_rowptr + S + 1);
   in.btcol.assign(Bt_colidx, Bt_colidx + Bt_rowptr[S]);
   in.btval.assign((size_t)Bt_rowptr[S], 0.0);
   return PIPS_OK;
}

// ---- host-pointer solves with several right-hand sides: pips_hip_ldl_solve finds the non-zero ones on the device, pips_hip_ldl_solve_sparse
// packs their marked rows on the host; both end in ldl_host_solve_tail
// The staging buffers stay with the handle (the reference's loop calls these entries hundreds of times per factorisation with the same chunk
// size; an allocation and a release per call were a fifth of a millisecond each).  One that must grow is not freed under a solve still running.
static int ldl_reserve_staging(const Engine& e, DevBuf<double>& buf, size_t doubles) {
   if (buf.size() >= doubles) return PIPS_OK;
   if (buf) HIP_TRY(hipStreamSynchronize(e.stream));
   return buf.reserve(doubles);
}
// d_X holds the right-hand sides rhs[nz[0]], rhs[nz[1]], .. (rows ld apart on the host, n apart on the device) or err why it does not: solve
// them, copy the solutions back to their rows - in one 2-D copy where every row of rhs is among them - and wait (what the caller staged on
// the host lives until then)
static int ldl_host_solve_tail(Engine& e, hipError_t err, double* d_X, const std::vector<int>& nz, int nrhs, double* rhs, int ld, const char* who) {
   const int nq = (int)nz.size();
   const size_t row = (size_t)e.n_total * sizeof(double);
   int rc = PIPS_OK;
   if (err == hipSuccess) {
      rc = nq == 1 ? e.solve(d_X) : e.solve_multi(d_X, nq, e.n_total);
      if (!rc && nq == nrhs)
         err = hipMemcpy2DAsync(rhs, (size_t)ld * sizeof(double), d_X, row, row, nrhs, hipMemcpyDeviceToHost, e.stream);
      else
         for (int q = 0; q < nq && !rc && err == hipSuccess; ++q)
            err = hipMemcpyAsync(rhs + (size_t)nz[q] * ld, d_X + (size_t)q * e.n_total, row, hipMemcpyDeviceToHost, e.stream);
      if (err == hipSuccess) err = hipStreamSynchronize(e.stream);
   }
   if (rc) return rc;
   if (err != hipSuccess) PIPS_FAIL(PIPS_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
   return PIPS_OK;
}

// flags[q] = 1 where column q of X (ld apart, n entries) has an entry that is not zero (a NaN counts)
__global__ __launch_bounds__(256) void k_columns_nonzero(const double* __restrict__ X, long long ld, int n, int* __restrict__ flags) {
   const double* v = X + ld * blockIdx.x;
   int any = 0;
   for (int i = threadIdx.x; i < n; i += 256) any |= (v[i] != 0.0) ? 1 : 0;
   any = __syncthreads_or(any);
   if (threadIdx.x == 0) flags[blockIdx.x] = any ? 1 : 0;
}

int pips_hip_ldl_solve(void* handle, int nrhs, double* rhs, int ld) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || nrhs < 0 || !rhs || ld < h->eng.in[0].n) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_solve: bad arguments");
   if (ldl_uses_group(h))   // the newest factors of this leaf are the batch's
      return group_solve_rows(*h->group, h->group_index, nrhs, rhs, ld, false, "pips_hip_ldl_solve");
   Engine& e = h->eng;
   if (!e.factored) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_solve: factor first");
   if (nrhs == 0) return PIPS_OK;
   HIP_TRY(hipSetDevice(e.device));
   const size_t row = (size_t)e.n_total * sizeof(double);
   if (nrhs == 1) {
      HIP_TRY(hipMemcpyAsync(e.d_stage, rhs, row, hipMemcpyHostToDevice, e.stream));
      int rc = e.solve(e.d_stage);
      if (rc) return rc;
      HIP_TRY(hipMemcpyAsync(rhs, e.d_stage, row, hipMemcpyDeviceToHost, e.stream));
      HIP_TRY(hipStreamSynchronize(e.stream));
      return PIPS_OK;
   }
   // all right-hand sides in one pass (one RHS per row of length ld).  Like PardisoSolver::solve (PardisoSolver.C:276-352) only the non-zero
   // right-hand sides are solved.  Which ones those are is found on the device AFTER the upload: a scan on the host walks every column up
   // to its first entry - the border columns of a chunk have theirs in the dual rows, behind 10 000 zeros each, 1.3 ms per call of 160 -
   // while the whole chunk crosses the link in 0.35 ms and the flags come back with one small copy.
   const size_t flag_bytes = ((size_t)nrhs * sizeof(int) + 15) & ~(size_t)15;
   PIPS_TRY(ldl_reserve_staging(e, h->d_hostx, ((size_t)nrhs * row + flag_bytes) / sizeof(double)));
   double* d_X = h->d_hostx;
   int* d_flags = (int*)(d_X + (size_t)nrhs * e.n_total);
   std::vector<int> flags((size_t)nrhs), nz;
   HIP_TRY(hipMemcpy2DAsync(d_X, row, rhs, (size_t)ld * sizeof(double), row, nrhs, hipMemcpyHostToDevice, e.stream));
   hipLaunchKernelGGL(k_columns_nonzero, dim3(nrhs), dim3(256), 0, e.stream, d_X, (long long)e.n_total, (int)e.n_total, d_flags);
   HIP_TRY(hipMemcpyAsync(flags.data(), d_flags, (size_t)nrhs * sizeof(int), hipMemcpyDeviceToHost, e.stream));
   HIP_TRY(hipStreamSynchronize(e.stream));
   nz.reserve(nrhs);
   for (int r = 0; r < nrhs; ++r) if (flags[r]) nz.push_back(r);
   if (nz.empty()) return PIPS_OK;
   hipError_t err = hipSuccess;   // the non-zero columns move to the front (ascending: a column never lands on one that is still to move)
   for (int q = 0; q < (int)nz.size() && err == hipSuccess; ++q)
      if (nz[q] != q) err = hipMemcpyAsync(d_X + (size_t)q * e.n_total, d_X + (size_t)nz[q] * e.n_total, row, hipMemcpyDeviceToDevice, e.stream);
   return ldl_host_solve_tail(e, err, d_X, nz, nrhs, rhs, ld, "pips_hip_ldl_solve");
}

// ---- device-pointer and sparse-row variants of the per-leaf solve
int pips_hip_ldl_solve_dev(void* handle, int nrhs, double* rhs_inout_dev, long long ld) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || nrhs < 1 || !rhs_inout_dev || ld < h->eng.in[0].n) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_solve_dev: bad arguments");
   if (ldl_uses_group(h)) return group_solve_rows(*h->group, h->group_index, nrhs, rhs_inout_dev, ld, true, "pips_hip_ldl_solve_dev");
   Engine& e = h->eng;
   if (!e.factored) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_solve_dev: factor first");
   HIP_TRY(hipSetDevice(e.device));
   return nrhs == 1 ? e.solve(rhs_inout_dev) : e.solve_multi(rhs_inout_dev, nrhs, ld);
}

// rows[i] = rhs row (0 <= row < n) of packed entry i: X[q * ld + rows[i]] = packed[q * n_rows + i]
__global__ void k_expand_rows(const int* __restrict__ rows, int n_rows, const double* __restrict__ packed, double* __restrict__ X, long long ld, int nrhs) {
   const long long total = (long long)n_rows * nrhs;
   for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
      const int q = (int)(idx / n_rows), i = (int)(idx - (long long)q * n_rows);
      X[q * ld + rows[i]] = packed[idx];
   }
}

// = DoubleLinearSolver::solve(int nrhss, double* rhss, int* colSparsity) with the third argument honoured: colSparsity[i] != 0 marks the rows
// that can be non-zero in any of the right-hand sides (the caller's border_left_transp pattern, DistributedLinearSystem.C:903).  Only those
// rows of the non-zero right-hand sides travel to the device (the solutions come back dense: K^-1 fills them).
int pips_hip_ldl_solve_sparse(void* handle, int nrhs, double* rhs, int ld, const int* col_sparsity) {
   if (!col_sparsity) return pips_hip_ldl_solve(handle, nrhs, rhs, ld);
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || nrhs < 0 || !rhs || ld < h->eng.in[0].n) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_solve_sparse: bad arguments");
   if (ldl_uses_group(h)) return pips_hip_ldl_solve(handle, nrhs, rhs, ld);   // (through the batch every row travels: colSparsity saves nothing there)
   Engine& e = h->eng;
   if (!e.factored) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_solve_sparse: factor first");
   HIP_TRY(hipSetDevice(e.device));
   const int n = (int)e.n_total;
   std::vector<int> rows, nz;
   for (int i = 0; i < n; ++i) if (col_sparsity[i]) rows.push_back(i);
   // where most rows are marked the whole columns travel faster than a pack on the host (the union over a chunk of 160 border columns of
   // configs[1] marks a fifth of the rows; 19 MB cross the link in 0.35 ms): the pack pays below an eighth
   if ((long long)rows.size() * 8 >= n) return pips_hip_ldl_solve(handle, nrhs, rhs, ld);
   for (int r = 0; r < nrhs; ++r) {
      const double* v = rhs + (size_t)r * ld;
      bool any = false;
      for (int i : rows) if (v[i] != 0.0) { any = true; break; }
      if (any) nz.push_back(r);
   }
   const int nq = (int)nz.size(), nr = (int)rows.size();
   if (nq == 0) return PIPS_OK;
   std::vector<double> packed((size_t)nq * nr);
   for (int q = 0; q < nq; ++q) {
      const double* v = rhs + (size_t)nz[q] * ld;
      for (int i = 0; i < nr; ++i) packed[(size_t)q * nr + i] = v[rows[i]];
   }
   const size_t pack_bytes = packed.size() * sizeof(double) + (size_t)nr * sizeof(int);
   PIPS_TRY(ldl_reserve_staging(e, h->d_hostx, (size_t)nq * n));
   PIPS_TRY(ldl_reserve_staging(e, h->d_hostpack, (pack_bytes + sizeof(double) - 1) / sizeof(double)));
   double *d_X = h->d_hostx, *d_packed = h->d_hostpack;
   int* d_rows = (int*)(d_packed + packed.size());
   hipError_t err = hipMemcpyAsync(d_packed, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice, e.stream);
   if (err == hipSuccess) err = hipMemcpyAsync(d_rows, rows.data(), (size_t)nr * sizeof(int), hipMemcpyHostToDevice, e.stream);
   if (err == hipSuccess) err = hipMemsetAsync(d_X, 0, (size_t)nq * n * sizeof(double), e.stream);
   if (err == hipSuccess)
      hipLaunchKernelGGL(k_expand_rows, dim3(grid_for((long long)nq * nr, 256)), dim3(256), 0, e.stream, d_rows, nr, d_packed, d_X, (long long)n, nq);
   return ldl_host_solve_tail(e, err, d_X, nz, nrhs, rhs, ld, "pips_hip_ldl_solve_sparse");
}

// ---- array-of-handles entries
// want_det (the sparse entries): the batch engine in deterministic mode - a binding that is not is replaced
static int ldl_group_of(void* const* handles, int n, std::shared_ptr<LdlGroup>& out, bool want_det = false) {
   if (!handles || n <= 0) PIPS_FAIL(PIPS_ERR_ARG, "array of leaf handles: bad arguments");
   LdlHandle* h0 = (LdlHandle*)handles[0];
   if (!h0) PIPS_FAIL(PIPS_ERR_ARG, "array of leaf handles: null handle");
   bool same = h0->group && (int)h0->group->members.size() == n && (!want_det || h0->group->eng.deterministic);
   for (int i = 0; i < n && same; ++i) same = handles[i] && h0->group->members[i] == (LdlHandle*)handles[i];
   if (same) { out = h0->group; return PIPS_OK; }
   // bind: one batch engine over the patterns (and borders) the handles hold
   auto g = std::make_shared<LdlGroup>();
   Engine& e = g->eng;
   e.nblk = n;
   e.S = h0->eng.S;
   e.device = h0->eng.device;
   e.thr_rel = h0->eng.thr_rel; e.repl_rel = h0->eng.repl_rel;
   e.refine_steps = h0->eng.refine_steps; e.refine_tol = h0->eng.refine_tol; e.refine_mode = h0->eng.refine_mode;
   e.deterministic = want_det;
   e.in.resize(n);
   for (int i = 0; i < n; ++i) {
      LdlHandle* h = (LdlHandle*)handles[i];
      if (!h) PIPS_FAIL(PIPS_ERR_ARG, "array of leaf handles: null handle at %d", i);
      if (h->eng.S != e.S) PIPS_FAIL(PIPS_ERR_ARG, "array of leaf handles: handle %d declares Schur dimension %d, handle 0 %d", i, h->eng.S, e.S);
      if (h->eng.device != e.device) PIPS_FAIL(PIPS_ERR_ARG, "array of leaf handles: handles on different devices");
      e.in[i] = h->eng.in[0];
      g->members.push_back(h);
   }
   int rc = pips_hip_batch_analyze(&e, std::min(n, 16));
   if (rc) return rc;
   for (int i = 0; i < n; ++i) { ((LdlHandle*)handles[i])->group = g; ((LdlHandle*)handles[i])->group_index = i; }
   out = g;
   return PIPS_OK;
}

// ---- the sparse Schur entries (INTEGRATION.md levels 1.5 / 1.5b for hosts with hasSparseKkt): the branch sparse_res = true of
// addBiTLeftKiBiRightToResBlockedParallelSolvers (DistributedLinearSystem.C:766-770, 1050-1113, 1180-1190), which adds the term into a
// SparseSymmetricMatrix.  The first call builds the position tables of the engine's blocks against the caller's pattern (schurtarget.cpp)
// and hands them to set_sc_tables: from then on every kernel that writes the Schur complement - tile SYRK, head scatters,
// k_border_schur_add, the packed blocked solves of Schur mode 2, deterministic mode's group buffers - addresses T doubles, the distinct
// pattern positions the blocks' cliques touch.  Later calls compare S, nnz, the triangle and the hash of the consulted rows.
static int sparse_schur_bind(Engine& e, SparseSchurBind& sb, int S, const int* sc_rowptr, const int* sc_colidx, int lower, const char* who) {
   std::vector<const int*> bt((size_t)e.nblk, nullptr);
   for (int b = 0; b < e.nblk; ++b) if (!e.in[b].btrow.empty()) bt[b] = e.in[b].btrow.data();
   SchurPatternId id;
   int rc;
   if (sb.bound) {
      if ((rc = build_schur_target(e.nblk, S, bt.data(), sc_rowptr, sc_colidx, lower, nullptr, id))) return rc;
      if (!(id == sb.id))
         PIPS_FAIL(PIPS_ERR_ARG, "%s: another pattern than the first call's (S %d / %d, %lld / %lld entries, %s / %s triangle, or other consulted rows)", who, S, sb.id.S,
                   id.nnz, sb.id.nnz, id.lower ? "lower" : "upper", sb.id.lower ? "lower" : "upper");
      return PIPS_OK;
   }
   SchurTarget t;
   if ((rc = build_schur_target(e.nblk, S, bt.data(), sc_rowptr, sc_colidx, lower, &t, id))) return rc;
   // (a target of at least one double: a length of 0 reads as "dense, S x S" in det_gstride)
   if ((rc = e.set_sc_tables(t.tab, t.off, std::max<long long>((long long)t.pos.size(), 1)))) return rc;
   if (e.deterministic && (rc = e.set_det_groups(0, 1))) return rc;   // group buffers as long as the compact array
   PIPS_TRY(sb.d_val.alloc(t.pos.size()));
   sb.pos = std::move(t.pos);
   sb.id = id;
   sb.bound = true;
   return PIPS_OK;
}

// ---- the four Schur-factor entries check their arguments, name the engine (the handle's own, or the batch of ldl_group_of) and the target
// of the term on the device; ldl_factor_schur_run is the sequence.  The targets: the device's shared S x S scratch array, of which the leaf's
// compact nb x nb block travels (one handle, dense); the group's S x S buffer (handles as one batch, dense); the compact array of the
// caller's sparse pattern (either); nothing - factorise only (the batch entries without a Schur complement)
enum { SC_TO_NOTHING, SC_TO_SCRATCH, SC_TO_GROUP, SC_TO_COMPACT };
struct ScPattern { int S; const int *rowptr, *colidx; int lower; };   // the caller's sparse Schur complement (SC_TO_COMPACT)

// leaf or group: whose engine factorises (a single handle is a batch of one: K_vals / Bt_vals hold a pointer per block of that engine);
// host: SC_host, row-major with ldhost, or sc_val_host
static int ldl_factor_schur_run(const char* who, LdlHandle* leaf, LdlGroup* group, int to, const double* const* K_vals, const double* const* Bt_vals,
                                double* host, int ldhost, const ScPattern* pat) {
   Engine& e = leaf ? leaf->eng : group->eng;
   SparseSchurBind& sb = leaf ? leaf->sparse_sc : group->sparse_sc;
   LdlHandle* const* hs = leaf ? &leaf : group->members.data();
   const int n_hs = leaf ? 1 : (int)group->members.size(), S = e.S;
   int rc;
   HIP_TRY(hipSetDevice(e.device));
   // one kind of Schur target per handle and per bound group for their lives: refuse the other one - before the sparse target reaches the
   // engine (set_sc_tables: a dense-kind handle never gets tables) - else take this one
   if (to != SC_TO_NOTHING) {
      const int kind = to == SC_TO_COMPACT ? SC_KIND_SPARSE : SC_KIND_DENSE;
      bool other = group && group->sc_kind != SC_KIND_NONE && group->sc_kind != kind;
      for (int i = 0; i < n_hs; ++i) other = other || (hs[i] && hs[i]->sc_kind != SC_KIND_NONE && hs[i]->sc_kind != kind);
      if (other)
         PIPS_FAIL(PIPS_ERR_STATE, "%s: the Schur target of %s is %s: one kind per handle", who, leaf ? "this handle" : "these handles",
                   kind == SC_KIND_DENSE ? "sparse (pips_hip_ldl_factor_schur_sparse / _batch)" : "dense (pips_hip_ldl_factor_schur / _batch)");
      if (pat && (rc = sparse_schur_bind(e, sb, pat->S, pat->rowptr, pat->colidx, pat->lower, who))) return rc;
      if (group) group->sc_kind = kind;
      for (int i = 0; i < n_hs; ++i) if (hs[i]) hs[i]->sc_kind = kind;
   }
   // the values of K and, with a target, of the borders, block after block as the engine keeps them; every pointer before the first copy
   for (int i = 0; i < e.nblk; ++i) {
      if (!K_vals[i]) PIPS_FAIL(PIPS_ERR_ARG, "%s: no values for leaf %d", who, i);
      if (to != SC_TO_NOTHING && !e.in[i].btcol.empty() && !Bt_vals[i]) PIPS_FAIL(PIPS_ERR_ARG, "%s: no border values for leaf %d", who, i);
   }
   for (int i = 0; i < e.nblk; ++i)
      HIP_TRY(hipMemcpyAsync(e.d_kval + e.kptr[i], K_vals[i], (size_t)(e.kptr[i + 1] - e.kptr[i]) * sizeof(double), hipMemcpyHostToDevice, e.stream));
   if (leaf) HIP_TRY(hipStreamSynchronize(e.stream));   // (as pips_hip_batch_set_values did for a single handle: its host waits per call stay)
   long long off = 0;
   for (int i = 0; i < e.nblk && to != SC_TO_NOTHING; ++i) {
      const size_t cnt = e.in[i].btcol.size();
      if (cnt > 0) HIP_TRY(hipMemcpyAsync(e.d_bval + off, Bt_vals[i], cnt * sizeof(double), hipMemcpyHostToDevice, e.stream));
      off += (long long)cnt;
   }
   // the target, clear: d_term / h_term is what travels to the host, n_term doubles of it (0: nothing to add)
   const std::vector<int>& bmap = e.sym[0].bmap;
   const size_t nb = to == SC_TO_SCRATCH ? bmap.size() : 0, SS = (size_t)S * S;
   const size_t n_term = to == SC_TO_SCRATCH ? nb * nb : to == SC_TO_GROUP ? SS : sb.pos.size();
   DevBuf<double>& d_term = to == SC_TO_SCRATCH ? leaf->d_sc : to == SC_TO_GROUP ? group->d_sc : sb.d_val;
   std::vector<double>& h_term = to == SC_TO_SCRATCH ? leaf->h_sc : to == SC_TO_GROUP ? group->h_sc : sb.h_val;
   std::unique_lock<std::mutex> scratch_lock(g_schur_scratch.mu, std::defer_lock);
   double* d_target = nullptr;
   if (to != SC_TO_NOTHING && n_term > 0 && !d_term) PIPS_TRY(d_term.alloc(n_term));
   if (to == SC_TO_SCRATCH) {
      // zero on entry: allocated zeroed, and every call takes its block out again and leaves zeros.  Held to the end of the call: host
      // threads that factorise their leaves side by side take turns on the scratch array
      scratch_lock.lock();
      DevBuf<double>& slot = g_schur_scratch.per_device[e.device];
      if (slot.size() < SS) PIPS_TRY(slot.alloc_zero(SS));
      d_target = slot;
   } else if (to != SC_TO_NOTHING && n_term > 0) {
      HIP_TRY(hipMemsetAsync(d_term, 0, n_term * sizeof(double), e.stream));
      d_target = d_term;
   }
   if ((rc = e.factor(d_target, to == SC_TO_COMPACT ? 0 : S))) {
      if (to == SC_TO_SCRATCH) {   // (whatever reached the scratch array must not meet the next handle)
         (void)hipStreamSynchronize(e.stream);
         (void)hipMemset(d_target, 0, SS * sizeof(double));
      }
      return rc;
   }
   // which engine holds the newest factors of these leaves now: the batch's, or the handle's own (the batch's copy of it is the older one)
   for (int i = 0; i < n_hs; ++i) if (hs[i]) hs[i]->newest_in_group = group != nullptr;
   if (nb > 0)
      hipLaunchKernelGGL(k_schur_take_block, dim3(std::max(1, std::min(16, ((int)nb + 255) / 256)), (int)nb), dim3(256), 0, e.stream, d_target, S, e.d_bmap, (int)nb, d_term);
   if (d_target && n_term > 0) {
      h_term.resize(n_term);
      HIP_TRY(hipMemcpyAsync(h_term.data(), d_term, n_term * sizeof(double), hipMemcpyDeviceToHost, e.stream));
   }
   HIP_TRY(hipStreamSynchronize(e.stream));
   if ((rc = e.sweep.take_error(who))) return rc;
   if (!d_target || n_term == 0) return PIPS_OK;
   // into the caller's matrix.  Dense - device: column-major with the lower triangle valid; caller: row-major DenseSymmetricMatrix, lower
   // triangle meaningful (DenseStorage.C:64-83): entry [i][j], i >= j, takes the device's (i, j), and only the rows and columns of the
   // blocks' non-empty border columns differ from zero
   if (to == SC_TO_SCRATCH) {
      for (size_t j = 0; j < nb; ++j)
         for (size_t i = j; i < nb; ++i) host[(size_t)bmap[i] * ldhost + bmap[j]] += h_term[i + j * nb];
   } else if (to == SC_TO_GROUP) {
      std::vector<char> used(S, 0);
      for (const BlockSym& bs : e.sym) for (int c : bs.bmap) used[c] = 1;
      std::vector<int> cols;
      for (int c = 0; c < S; ++c) if (used[c]) cols.push_back(c);
      for (int cb : cols)
         for (int ra : cols)
            if (ra >= cb) host[(size_t)ra * ldhost + cb] += h_term[(size_t)ra + (size_t)cb * S];
   } else
      for (size_t t = 0; t < n_term; ++t) host[sb.pos[t]] += h_term[t];
   return PIPS_OK;
}

int pips_hip_ldl_factor_schur(void* handle, const double* K_vals_host, const double* Bt_vals_host, double* SC_host, int ldSC) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || !K_vals_host || !Bt_vals_host || !SC_host) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_factor_schur: bad arguments");
   Engine& e = h->eng;
   if (e.S <= 0 || e.in[0].btrow.empty()) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_factor_schur: no border declared (pips_hip_ldl_set_border)");
   if (ldSC < e.S) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_factor_schur: ldSC %d < S %d", ldSC, e.S);
   int rc;
   if (!e.analyzed && (rc = pips_hip_ldl_analyze(handle))) return rc;
   return ldl_factor_schur_run("pips_hip_ldl_factor_schur", h, nullptr, SC_TO_SCRATCH, &K_vals_host, &Bt_vals_host, SC_host, ldSC, nullptr);
}

int pips_hip_ldl_factor_schur_batch(void* const* handles, int n, const double* const* K_vals_host, const double* const* Bt_vals_host, double* SC_host,
                                    int ldSC) {
   std::shared_ptr<LdlGroup> g;
   int rc = ldl_group_of(handles, n, g);
   if (rc) return rc;
   if (!K_vals_host) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_factor_schur_batch: no values");
   const int S = g->eng.S;
   if (SC_host && (S <= 0 || ldSC < S || !Bt_vals_host)) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_factor_schur_batch: Schur term asked for without border / ldSC %d < S %d", ldSC, S);
   return ldl_factor_schur_run("pips_hip_ldl_factor_schur_batch", nullptr, g.get(), SC_host ? SC_TO_GROUP : SC_TO_NOTHING, K_vals_host, Bt_vals_host, SC_host, ldSC, nullptr);
}

int pips_hip_ldl_factor_schur_sparse(void* handle, const double* K_vals_host, const double* Bt_vals_host, int S, const int* sc_rowptr, const int* sc_colidx,
                                     double* sc_val_host, int lower) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || !K_vals_host || !Bt_vals_host || !sc_rowptr || !sc_colidx || !sc_val_host) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_factor_schur_sparse: bad arguments");
   Engine& e = h->eng;
   if (e.S <= 0 || e.in[0].btrow.empty()) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_factor_schur_sparse: no border declared (pips_hip_ldl_set_border)");
   if (S != e.S) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_factor_schur_sparse: S %d, the border was declared with %d", S, e.S);
   int rc;
   if (!e.analyzed) {
      if (env_deterministic()) e.deterministic = true;   // (the default, as for batches: pips_hip_batch_create)
      if ((rc = pips_hip_ldl_analyze(handle))) return rc;
   }
   const ScPattern pat = {S, sc_rowptr, sc_colidx, lower};
   return ldl_factor_schur_run("pips_hip_ldl_factor_schur_sparse", h, nullptr, SC_TO_COMPACT, &K_vals_host, &Bt_vals_host, sc_val_host, 0, &pat);
}

int pips_hip_ldl_factor_schur_sparse_batch(void* const* handles, int n, const double* const* K_vals_host, const double* const* Bt_vals_host, int S,
                                           const int* sc_rowptr, const int* sc_colidx, double* sc_val_host, int lower) {
   const char* who = "pips_hip_ldl_factor_schur_sparse_batch";
   std::shared_ptr<LdlGroup> g;
   const bool want_det = handles && n > 0 && handles[0] && (((LdlHandle*)handles[0])->eng.deterministic || env_deterministic());
   int rc = ldl_group_of(handles, n, g, want_det);
   if (rc) return rc;
   if (!K_vals_host) PIPS_FAIL(PIPS_ERR_ARG, "%s: no values", who);
   if (!sc_val_host) return ldl_factor_schur_run(who, nullptr, g.get(), SC_TO_NOTHING, K_vals_host, Bt_vals_host, nullptr, 0, nullptr);
   if (g->eng.S <= 0 || !Bt_vals_host || !sc_rowptr || !sc_colidx) PIPS_FAIL(PIPS_ERR_ARG, "%s: Schur term asked for without border or pattern", who);
   if (S != g->eng.S) PIPS_FAIL(PIPS_ERR_ARG, "%s: S %d, the borders were declared with %d", who, S, g->eng.S);
   const ScPattern pat = {S, sc_rowptr, sc_colidx, lower};
   return ldl_factor_schur_run(who, nullptr, g.get(), SC_TO_COMPACT, K_vals_host, Bt_vals_host, sc_val_host, 0, &pat);
}

int pips_hip_ldl_solve_batch_dev(void* const* handles, int n, double* x_dev) {
   std::shared_ptr<LdlGroup> g;
   int rc = ldl_group_of(handles, n, g);
   if (rc) return rc;
   if (!x_dev) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_solve_batch_dev: null vector");
   if ((rc = ldl_group_is_current(*g, "pips_hip_ldl_solve_batch_dev"))) return rc;
   HIP_TRY(hipSetDevice(g->eng.device));
   return g->eng.solve(x_dev);
}

int pips_hip_ldl_solve_batch(void* const* handles, int n, double* const* rhs_inout_host) {
   std::shared_ptr<LdlGroup> g;
   int rc = ldl_group_of(handles, n, g);
   if (rc) return rc;
   if (!rhs_inout_host) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_ldl_solve_batch: null array");
   Engine& e = g->eng;
   if ((rc = ldl_group_is_current(*g, "pips_hip_ldl_solve_batch"))) return rc;
   HIP_TRY(hipSetDevice(e.device));
   if (!g->d_x) PIPS_TRY(g->d_x.alloc((size_t)std::max<long long>(e.n_total, 1)));
   // a leaf without a right-hand side this time (NULL) is solved with zeros: the batch runs every block in every launch
   HIP_TRY(hipMemsetAsync(g->d_x, 0, (size_t)e.n_total * sizeof(double), e.stream));
   for (int i = 0; i < n; ++i)
      if (rhs_inout_host[i])
         HIP_TRY(hipMemcpyAsync(g->d_x + e.x_off[i], rhs_inout_host[i], (size_t)(e.x_off[i + 1] - e.x_off[i]) * sizeof(double), hipMemcpyHostToDevice, e.stream));
   if ((rc = e.solve(g->d_x))) return rc;
   for (int i = 0; i < n; ++i)
      if (rhs_inout_host[i])
         HIP_TRY(hipMemcpyAsync(rhs_inout_host[i], g->d_x + e.x_off[i], (size_t)(e.x_off[i + 1] - e.x_off[i]) * sizeof(double), hipMemcpyDeviceToHost, e.stream));
   HIP_TRY(hipStreamSynchronize(e.stream));
   return e.sweep.take_error("pips_hip_ldl_solve_batch");
}

int pips_hip_ldl_inertia_batch(void* const* handles, int n, int* pos, int* neg, int* zero) {
   std::shared_ptr<LdlGroup> g;
   int rc = ldl_group_of(handles, n, g);
   if (rc) return rc;
   if ((rc = ldl_group_is_current(*g, "pips_hip_ldl_inertia_batch"))) return rc;
   for (int i = 0; i < n; ++i) {
      int p = 0, q = 0, z = 0;
      if ((rc = pips_hip_batch_inertia(&g->eng, i, &p, &q, &z))) return rc;
      if (pos) pos[i] = p;
      if (neg) neg[i] = q;
      if (zero) zero[i] = z;
   }
   return PIPS_OK;
}

int pips_hip_ldl_inertia(void* handle, int* pos, int* neg, int* zero) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   if (ldl_uses_group(h))   // the newest factorisation of this leaf was the batch's (pips_hip_ldl_factor_schur_batch)
      return pips_hip_batch_inertia(&h->group->eng, h->group_index, pos, neg, zero);
   return pips_hip_batch_inertia(&h->eng, 0, pos, neg, zero);
}

int pips_hip_ldl_info(void* handle, int64_t* what, int n_what) {
   LdlHandle* h = (LdlHandle*)handle;
   const bool grp = h && ldl_uses_group(h);
   if (!h || (h->eng.sym.empty() && !grp)) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_info: analyze first");
   // (a handle that was only ever factorised through its batch has its analysis there)
   const BlockSym& s = h->eng.sym.empty() ? h->group->eng.sym[h->group_index] : h->eng.sym[0];
   // [8], [9]: of the engine that holds this leaf's newest factors - the Schur mode its analysis took and the doubles of its compact
   // sparse Schur target (0: none, the target is dense)
   const Engine& cur = grp ? h->group->eng : h->eng;
   const SparseSchurBind& sb = grp ? h->group->sparse_sc : h->sparse_sc;
   int64_t v[10] = {s.nnzL, s.n_head, s.m, (int64_t)s.sn.size(), s.n_levels, (int64_t)s.flops_factor, (int64_t)h->eng.last_refine_steps, (int64_t)h->eng.last_multi_path,
                    (int64_t)cur.schur_mode_eff, sb.bound ? (int64_t)sb.pos.size() : 0};
   for (int i = 0; i < n_what && i < 10; ++i) what[i] = v[i];
   return PIPS_OK;
}

int pips_hip_ldl_get_perm(void* handle, int* perm) {
   LdlHandle* h = (LdlHandle*)handle;
   if (!h || h->eng.sym.empty() || !perm) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_ldl_get_perm: analyze first");
   std::copy(h->eng.sym[0].perm.begin(), h->eng.sym[0].perm.end(), perm);
   return PIPS_OK;
}

void pips_hip_ldl_destroy(void* handle) { delete (LdlHandle*)handle; }
