// Dense root solver (DeSymIndefSolver replacement) on the same tile kernels: DenseLdl and the pips_hip_dense_ldl_* entry points.
// Included once by engine.hip, inside namespace pips, after Engine and before kkt.hip.h (KktSystem holds a DenseLdl).
#pragma once

extern "C" int pips_hip_allreduce_sum(void* comm, double* buf_dev, size_t n, void* stream);
extern "C" int pips_hip_all_gather(void* comm, double* buf_dev, size_t chunk, int n_parts, void* stream);
extern "C" int pips_hip_broadcast(void* comm, double* buf_dev, size_t n, int root, void* stream);
extern "C" int pips_hip_comm_has_broadcast(void* comm);

__global__ void k_inertia_to_double(const int* __restrict__ in, double* __restrict__ out, int back, int* __restrict__ in_out) {
   if (threadIdx.x < 3) { if (!back) out[threadIdx.x] = (double)in[threadIdx.x]; else in_out[threadIdx.x] = (int)(out[threadIdx.x] + 0.5); }
}

// Several right-hand sides (DenseLdl::solve_multi_dev): the transposing copy between the caller's nr vectors at distance ld and the interleaved
// panels of MQ (kernels.hip.h "multi-vector solves": entry k of right-hand side q of panel p at xm[p * panel_stride + k * MQ + q]).  k_mpermute
// is the leaf's version; its consecutive threads walk q, ld doubles apart on the caller's side - which for a dense root is the whole of the
// data.  Here a workgroup moves 32 rows x 32 right-hand sides through an LDS tile padded to 33 columns, so that both sides are read and
// written along their contiguous direction (with a Bunch-Kaufman order, perm != nullptr, the caller's side is a gather / scatter: position k
// is x[perm[k]]).  grid (npad / 32, panels), 256 threads.  In (out = 0): all npad rows and MQ columns of every panel are written, zeros for
// k >= n and q >= nr; out = 1: only k < n, q < nr go back.  Nothing of x outside the nr x n entries is touched.
__global__ __launch_bounds__(256) void k_root_interleave(double* __restrict__ x, long long ld, int nr, int n, const int* __restrict__ perm,
                                                         double* __restrict__ xm, long long panel_stride, int out) {
   __shared__ double t[MQ][MQ + 1];   // t[q][k]
   const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, k0 = 32 * blockIdx.x, q0 = MQ * blockIdx.y;
   double* w = xm + panel_stride * blockIdx.y + (long long)k0 * MQ;
   const int k = k0 + tx;
   const long long col = k < n ? (perm ? perm[k] : k) : 0;
   if (!out) {
      for (int q = ty; q < MQ; q += 8) t[q][tx] = (k < n && q0 + q < nr) ? x[(long long)(q0 + q) * ld + col] : 0.0;
      __syncthreads();
      for (int r = ty; r < 32; r += 8) w[r * MQ + tx] = t[tx][r];
   } else {
      for (int r = ty; r < 32; r += 8) t[tx][r] = w[r * MQ + tx];
      __syncthreads();
      for (int q = ty; q < MQ; q += 8)
         if (k < n && q0 + q < nr) x[(long long)(q0 + q) * ld + col] = t[q][tx];
   }
}

struct DenseLdl {
   int device = 0, n = 0, npad = 0, n_primal = -1;
   // 0: static pivot order with the expected signs of the inertia hint (right for the quasi-definite Schur complement the fused
   //    path builds itself: no search on the critical path of the 128 dependent pivots of a tile);
   // 1: Bunch-Kaufman 1 x 1 / 2 x 2 pivoting bounded to the diagonal tile (k_tile_diag_bk): what a drop-in for DeSymIndefSolver
   //    needs - dsytrf takes any symmetric matrix (DeSymIndefSolver.C:78)
   int pivoting = 0;
   hipStream_t stream = nullptr;
   double thr_rel = 1e-13, repl_rel = 1e-8;
   bool factored = false;
   std::vector<BlkDesc> h_blks;
   TailPlan plan;
   DevBuf<BlkDesc> d_blks;
   DevBuf<double> d_R, d_winv, d_dtail, d_xw, d_in, d_pref;
   DevBuf<double> d_U;   // U = L D (npad x npad), B operand of the updates
   DevBuf<signed char> d_psign;
   DevBuf<long long> d_psign_off, d_kptr;
   DevBuf<int> d_inertia;
   int h_inertia[3] = {0, 0, 0};
   hipStream_t side = nullptr;
   hipEvent_t ev_panel = nullptr, ev_rest = nullptr;
   // staging copy of a host matrix: only the host-pointer entry points need it (the fused KKT path hands over d_SC)
   int ensure_input_buffer() {
      if (!d_in) PIPS_TRY(d_in.alloc((size_t)std::max(n, 1) * std::max(n, 1)));
      return PIPS_OK;
   }

   ~DenseLdl() {
      if (side) (void)hipStreamDestroy(side);
      if (ev_panel) (void)hipEventDestroy(ev_panel);
      if (ev_rest) (void)hipEventDestroy(ev_rest);
   }
   SweepRt sweep;
   // ---- the factorisation as ONE dependency-driven launch (rootkernel.hip.h, rootplan.cpp): static pivot order on one rank.  Bunch-Kaufman
   // (a 454-register diagonal kernel) and the root distributed over ranks keep the launch-per-step driver (tail_factor / factor_distributed);
   // PIPS_HIP_ROOT_LAUNCHES (set to any value) keeps it everywhere (the tests run both).
   bool single_launch = !knob_set<K_ROOT_LAUNCHES>();
   bool last_single = false;       // which driver the last factorisation took (pips_hip_dense_ldl_info)
   DevBuf<double> d_C;             // the accumulating tiles (scratch): L goes to d_R, U to d_U, each written once per launch
   DevBuf<TileTask> d_rtasks;
   int n_rtasks = 0, n_rbulk = 0;
   DevBuf<int> d_rflags;           // ctl[8] | prog[ntc * ntc] | rowdone[ntc] | dready[ntc]
   double plan_makespan_us = 0.0;
   long long root_poll_limit = 0;   // PIPS_HIP_ROOT_POLL_LIMIT (ensure_single_launch): polls before a wait inside the launch gives up (some 0.1 s: a factorisation takes 2 - 40 ms)
   bool root_error_pending = false;
   int ensure_single_launch() {
      if (d_rtasks) return PIPS_OK;
      const int ntc = npad / TILE;
      RootPlanParams pp;
      if (const int cu = knob_tri<K_ROOT_CHAIN_CU>(); cu >= 0) pp.chain_slots = cu ? 2 : 0;
      if (pp.chain_slots == 0) pp.workers = 512;
      std::vector<int> t, tc;
      int rc = build_root_plan(ntc, pp, t, tc, &plan_makespan_us);
      if (rc) return rc;
      n_rbulk = (int)(t.size() / 4);
      t.insert(t.end(), tc.begin(), tc.end());
      n_rtasks = (int)(t.size() / 4);
      PIPS_TRY(d_rtasks.alloc(std::max<size_t>(t.size() / 4, 1)));
      HIP_TRY(hipMemcpy(d_rtasks, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
      PIPS_TRY(d_rflags.alloc(((size_t)8 + (size_t)ntc * ntc + 2 * (size_t)ntc)));
      PIPS_TRY(d_C.alloc((size_t)npad * npad));
      root_poll_limit = knob_int<K_ROOT_POLL_LIMIT>();
      return PIPS_OK;
   }
   int factor_single_launch() {
      const int ntc = npad / TILE;
      HIP_TRY(hipMemsetAsync(d_rflags, 0, ((size_t)8 + (size_t)ntc * ntc + 2 * (size_t)ntc) * sizeof(int), stream));
      RootArgs a{};
      a.tasks = d_rtasks; a.n_tasks = n_rtasks; a.n_bulk = n_rbulk; a.ntc = ntc; a.ld = npad;
      a.C = d_C; a.R = d_R; a.U = d_U; a.winv = d_winv; a.dtail = d_dtail; a.pref = d_pref; a.psign = d_psign; a.inertia = d_inertia;
      a.ctl = d_rflags; a.prog = d_rflags + 8; a.rowdone = a.prog + (size_t)ntc * ntc; a.dready = a.rowdone + ntc;
      a.blk = d_blks; a.poll_limit = root_poll_limit;
      a.diag_blocked = knob_int<K_ROOT_DIAG_BARRIERS>() ? 0 : 1;
      const char* trace_file = knob_text<K_ROOT_TRACE>();
      DevBuf<long long> d_trace;
      if (trace_file) {
         PIPS_TRY(d_trace.alloc(((size_t)3 * n_rtasks + 32 * (size_t)ntc)));
         HIP_TRY(hipMemsetAsync(d_trace, 0, ((size_t)3 * n_rtasks + 32 * (size_t)ntc) * sizeof(long long), stream));
         a.trace = d_trace;
      }
      hipLaunchKernelGGL(k_root_ldl, dim3(n_rtasks), dim3(512), 0, stream, a);
      HIP_TRY(hipGetLastError());
      root_error_pending = true;
      if (trace_file) {
         std::vector<long long> h((size_t)3 * n_rtasks + 32 * (size_t)ntc);
         std::vector<int> ht((size_t)4 * n_rtasks);
         HIP_TRY(hipStreamSynchronize(stream));
         HIP_TRY(hipMemcpy(h.data(), d_trace, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
         HIP_TRY(hipMemcpy(ht.data(), d_rtasks, ht.size() * sizeof(int), hipMemcpyDeviceToHost));
         d_trace.reset();
         if (FILE* f = fopen(trace_file, "w")) {
            for (int t = 0; t < n_rtasks; ++t)
               fprintf(f, "%d %d %d %d %d %lld %lld %lld\n", t, ht[4 * t], ht[4 * t + 1], ht[4 * t + 2], ht[4 * t + 3], h[3 * (size_t)t], h[3 * (size_t)t + 1], h[3 * (size_t)t + 2]);
            fclose(f);
         }
         if (FILE* f = fopen((std::string(trace_file) + ".diag").c_str(), "w")) {   // phase clocks of the diagonal tiles (blocked variant)
            for (int jj = 0; jj < ntc; ++jj) {
               for (int q = 0; q < 26; ++q) fprintf(f, "%lld ", h[(size_t)3 * n_rtasks + 32 * (size_t)jj + q]);
               fprintf(f, "\n");
            }
            fclose(f);
         }
      }
      return PIPS_OK;
   }
   // a wait inside the launch that gave up raised the error word; read at the host's next synchronisation point with this handle
   int take_root_error(const char* who) {
      if (!root_error_pending || !d_rflags) return PIPS_OK;
      root_error_pending = false;
      int w = 0;
      HIP_TRY(hipMemcpyAsync(&w, d_rflags + 1, sizeof(int), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      if (w) PIPS_FAIL(PIPS_ERR_HIP, "%s: the single-launch root factorisation gave up waiting for a tile after %lld polls (its factors are invalid); "
                                     "PIPS_HIP_ROOT_LAUNCHES (set to any value) selects the launch-per-step factorisation", who, root_poll_limit);
      return PIPS_OK;
   }
   int init() {
      HIP_TRY(hipSetDevice(device));
      int rc = PIPS_OK;
      npad = (n + TILE - 1) / TILE * TILE;
      BlkDesc d{};
      d.n = n; d.n_head = 0; d.m = n; d.m_pad = npad; d.nb = 0; d.nb_pad = 0; d.ldT = npad;
      d.ntc = d.ntr = npad / TILE;
      d.thr_rel = 0; d.repl_rel = 1e-8; d.repl_abs = 1;
      h_blks.assign(1, d);
      if ((rc = d_blks.upload(h_blks))) return rc;
      // one block only: right-looking (measured on MI355X, tools/root_probe.py: S=2000 4.3 -> 2.3 ms, S=16000 183 -> 45 ms;
      // panels of 1 tile column are best up to S = 8000, 2-3 beyond)
      const int panel = d.ntc <= 64 ? 1 : 2;
      // lookahead (second stream) pays once the trailing update of a panel outlasts a diagonal tile: S >= 6000 measured
      const bool lookahead = d.ntc >= 48;
      if ((rc = plan.build_root(h_blks, panel, lookahead))) return rc;
      if ((rc = sweep.build(h_blks, nullptr))) return rc;
      if (lookahead) {
         int prio_lo = 0, prio_hi = 0;
         HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
         HIP_TRY(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, prio_lo));   // the bulk update: behind the diagonal chain
         HIP_TRY(hipEventCreateWithFlags(&ev_panel, hipEventDisableTiming));
         HIP_TRY(hipEventCreateWithFlags(&ev_rest, hipEventDisableTiming));
      }
      std::vector<signed char> ps(npad, 1);
      for (int i = 0; i < n; ++i) ps[i] = n_primal < 0 ? 0 : (i < n_primal ? 1 : -1);
      if ((rc = d_psign.upload(ps))) return rc;
      std::vector<long long> zero(1, 0), kp = {0, (long long)npad};   // fallback magnitude from the diagonal only
      if ((rc = d_psign_off.upload(zero))) return rc;
      if ((rc = d_kptr.upload(kp))) return rc;
      PIPS_TRY(d_R.alloc((size_t)npad * npad));
      PIPS_TRY(d_U.alloc((size_t)npad * npad));
      PIPS_TRY(d_winv.alloc((size_t)npad * TILE));
      PIPS_TRY(d_dtail.alloc((size_t)npad));
      PIPS_TRY(d_xw.alloc((size_t)npad));
      PIPS_TRY(d_pref.alloc((size_t)npad));
      PIPS_TRY(d_inertia.alloc(3));
      return PIPS_OK;
   }
   TailCtx ctx() {
      TailCtx c;
      c.d_blks = d_blks; c.plan = &plan; c.d_arena = d_R; c.d_uarena = d_U; c.d_dtail = d_dtail; c.d_winv = d_winv;
      c.d_psign = d_psign; c.d_psign_off = d_psign_off; c.d_inertia = d_inertia; c.d_pref = d_pref;
      c.stream = stream; c.side = side; c.ev_panel = ev_panel; c.ev_rest = ev_rest;
      c.is_root = true; c.sweep = &sweep; c.bunch_kaufman = pivoting == 1;
      if (pivoting == 1) {
         c.d_pert_cnt = d_pert_cnt; c.d_pert_list = d_pert_list;
         c.bk_orig = last_A; c.bk_orig_ld = last_lda; c.bk_orig_rowmajor = last_rowmajor; c.d_bk_perm = perm.empty() ? nullptr : d_perm;
         c.bk_isolate = bk_isolate;
      }
      return c;
   }
   // ---- Bunch-Kaufman beyond the tile.  k_tile_diag_bk searches its 128 x 128 tile; dsytrf searches the whole column
   // (DeSymIndefSolver.C:78).  Where a tile finds no pivot for an index (a zero leading block coupled only to later rows: [[0 A^T]; [A 0]])
   // the kernel records the row of the column's largest entry in the panel below.  check_pivots() - at the next host synchronisation
   // point: the end of the host-pointer factor call, or the join with the root's stream before the first Dsolve - then moves every such
   // row next to its column (a symmetric permutation P kept for the following factorisations: the structure that needed it comes back
   // every iteration), factorises P A P^T again and goes on until no index is left without a pivot (at most BK_RETRIES times).  The
   // pair then sits inside one tile, where the 2 x 2 pivot is found.  Solves permute their right-hand side in and out.
   static constexpr int BK_RETRIES = 8;
   static constexpr int BK_MAX_COLUMNS = 2048;   // columns per round whose original entries travel to the host for the partner choice
   std::vector<int> perm;              // perm[i] = original index at position i (empty: identity)
   DevBuf<int> d_perm;
   DevBuf<int> d_pert_cnt, d_pert_list;
   const double* last_A = nullptr;     // the matrix of the last factor_dev (the caller keeps it until the next factorisation)
   int last_lda = 0, last_rowmajor = 0;
   bool check_pending = false;
   int bk_isolate = 1;                 // factorisations check_pivots will look at take an index without a pivot OUT of the matrix (k_tile_diag_bk)
   int bk_refactorizations = 0;        // how often check_pivots had to factorise again (diagnostics / tests)
   // indices (positions in the current order) the last factorisation found no pivot for: one rank - what its tile kernels recorded, in
   // their order; a root distributed over several ranks - every rank recorded those of its own tile columns, the union (ascending) reaches
   // every rank through an all-reduce of a 0 / 1 vector, so that all ranks go on to build the SAME pivot order
   DevBuf<double> d_flagvec;
   int flagged_positions(std::vector<int>& pos) {
      pos.clear();
      int cnt = 0;
      HIP_TRY(hipMemcpyAsync(&cnt, d_pert_cnt, sizeof(int), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      cnt = std::min(cnt, npad);   // (an index flagged by the tile kernel AND the growth check counts twice: the kernels stop writing at npad records)
      std::vector<int> rec((size_t)2 * std::max(cnt, 0));
      if (cnt > 0) HIP_TRY(hipMemcpy(rec.data(), d_pert_list, rec.size() * sizeof(int), hipMemcpyDeviceToHost));
      if (dist_P <= 1) {
         for (int q = 0; q < cnt; ++q) pos.push_back(rec[2 * q]);
         return PIPS_OK;
      }
      std::vector<double> flag((size_t)npad, 0.0);
      for (int q = 0; q < cnt; ++q) if (rec[2 * q] >= 0 && rec[2 * q] < npad) flag[rec[2 * q]] = 1.0;
      if (!d_flagvec) PIPS_TRY(d_flagvec.alloc((size_t)npad));
      HIP_TRY(hipMemcpy(d_flagvec, flag.data(), flag.size() * sizeof(double), hipMemcpyHostToDevice));
      int rc = pips_hip_allreduce_sum(dist_comm, d_flagvec, (size_t)npad, stream);
      if (rc) return rc;
      HIP_TRY(hipStreamSynchronize(stream));
      HIP_TRY(hipMemcpy(flag.data(), d_flagvec, flag.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (int i = 0; i < n; ++i) if (flag[i] > 0.0) pos.push_back(i);
      return PIPS_OK;
   }
   int check_pivots() {
      if (!check_pending) return PIPS_OK;
      check_pending = false;
      if (pivoting != 1 || !d_pert_cnt) return PIPS_OK;
      HIP_TRY(hipSetDevice(device));
      std::vector<int> fpos;
      for (int attempt = 0; attempt < BK_RETRIES; ++attempt) {
         int rcf = flagged_positions(fpos);
         if (rcf) return rcf;
         const int cnt = (int)fpos.size();
         if (cnt <= 0) return PIPS_OK;
         std::vector<int> rec((size_t)2 * cnt, -1);
         for (int q = 0; q < cnt; ++q) rec[2 * q] = fpos[q];
         if (dist_P > 1) HIP_TRY(hipMemcpy(d_pert_list, rec.data(), std::min(rec.size(), (size_t)2 * npad) * sizeof(int), hipMemcpyHostToDevice));   // (k_bk_gather_columns reads the positions there)
         // positions (in the current order) -> partner positions.  For every index without a pivot the column of the ORIGINAL matrix comes
         // to the host; in the order the tiles reported them each takes the row with its largest entry that is still free (not itself
         // without a pivot, not taken by an earlier column): the row a 2 x 2 pivot with this column needs ([[0 A^T]; [A 0]]: a row of A).
         const int n_use = std::min(cnt, BK_MAX_COLUMNS);
         std::vector<double> cols((size_t)n_use * n);
         {
            DevBuf<double> d_cols;
            PIPS_TRY(d_cols.alloc(cols.size()));
            hipLaunchKernelGGL(k_bk_gather_columns, dim3(std::max(1, std::min(64, (n + 255) / 256)), n_use), dim3(256), 0, stream, last_A, last_lda, last_rowmajor,
                               perm.empty() ? (const int*)nullptr : (const int*)d_perm, n, d_pert_list, n_use, d_cols);
            const hipError_t ec = hipMemcpy(cols.data(), d_cols, cols.size() * sizeof(double), hipMemcpyDeviceToHost);
            d_cols.reset();
            if (ec != hipSuccess) PIPS_FAIL(PIPS_ERR_HIP, "dense root: %s", hipGetErrorString(ec));
         }
         std::vector<int> partner(n, -1);
         std::vector<char> taken(n, 0), flagged(n, 0);
         for (int q = 0; q < cnt; ++q) if (rec[2 * q] >= 0 && rec[2 * q] < n) flagged[rec[2 * q]] = 1;
         bool any = false;
         for (int q = 0; q < n_use; ++q) {
            const int c = rec[2 * q];
            if (c < 0 || c >= n || partner[c] >= 0) continue;
            const double* col = cols.data() + (size_t)q * n;
            int best = -1;
            for (int i = 0; i < n; ++i)
               if (!flagged[i] && !taken[i] && col[i] > 0.0 && (best < 0 || col[i] > col[best])) best = i;
            if (best < 0) continue;
            partner[c] = best; taken[best] = 1; any = true;
         }
         if (!any) break;               // nothing below to pair with
         std::vector<int> cur(n);
         for (int i = 0; i < n; ++i) cur[i] = perm.empty() ? i : perm[i];
         std::vector<int> next;
         next.reserve(n);
         std::vector<int> deferred;     // a pair must not straddle a tile boundary: an unpaired index goes in between
         for (int i = 0; i < n; ++i) {
            if (taken[i]) continue;      // emitted right behind its column (wherever it stood)
            if (partner[i] >= 0) {
               if ((int)next.size() % TILE == TILE - 1) {
                  int filler = -1;
                  for (int t = i + 1; t < n && filler < 0; ++t) if (!taken[t] && partner[t] < 0 && t != i && !flagged[t] && std::find(deferred.begin(), deferred.end(), t) == deferred.end()) filler = t;
                  if (filler >= 0) { next.push_back(cur[filler]); deferred.push_back(filler); }
               }
               next.push_back(cur[i]);
               next.push_back(cur[partner[i]]);
            } else if (std::find(deferred.begin(), deferred.end(), i) == deferred.end())
               next.push_back(cur[i]);
         }
         if ((int)next.size() != n) PIPS_FAIL(PIPS_ERR_STATE, "dense root: internal error building the pivot order (%zu of %d)", next.size(), n);
         perm.swap(next);
         if (!d_perm) PIPS_TRY(d_perm.alloc((size_t)std::max(n, 1)));
         HIP_TRY(hipMemcpy(d_perm, perm.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
         ++bk_refactorizations;
         int rc = factor_enqueue();
         if (rc) return rc;
      }
      // indices without a pivot are left: they get the usual small replacement (and are reported as perturbed pivots - what the
      // regularisation loop of the caller reacts to) instead of being taken out of the matrix
      {
         int rcf = flagged_positions(fpos);
         if (rcf) return rcf;
         if (!fpos.empty()) {
            bk_isolate = 0;
            const int rc = factor_enqueue();
            bk_isolate = 1;
            if (rc) return rc;
         }
      }
      return PIPS_OK;
   }

   // ---- distributed factorisation (several ranks, each with the whole reduced Schur complement): tile column j belongs to rank
   // j mod P (1-D column-cyclic).  The owner factorises the diagonal tile and solves the column's panel, the panel (Winv_j, d_j, L(:, j),
   // U(:, j)) goes to every rank, and every rank applies it to the tile columns it owns - 1 / P of the S^3 / 3 flops per rank instead
   // of all of them on every rank (DistributedRootLinearSystem.C:1436-1464 has every rank call dsytrf on the same matrix).  At the
   // end every rank holds the complete factor, so the solves stay local and replicated.  The panel travels by pips_hip_broadcast
   // (ncclBroadcast / the host's broadcast callback; a host communicator without one: as an all-reduce in which the other ranks
   // contribute zeros - exact, twice the bytes).  One column of lookahead (round 5): see factor_distributed.  NOT TIMED: the GPU box has one
   // device; correctness with 2 and 4 processes sharing it (tests/test_dist_root_gpu.py).
   void* dist_comm = nullptr;
   int dist_rank = 0, dist_P = 1;
   std::vector<TaskList> dist_diag, dist_trsm, dist_next, dist_upd;   // dist_next[j]: this rank's tiles of column j + 1 under panel j; dist_upd[j]: of its columns >= j + 2
   DevBuf<TileTask> d_dist_tasks;
   DevBuf<double> d_panel;
   int set_distributed(void* comm, int rank, int P) {
      if (P <= 1 || !comm) { dist_comm = nullptr; dist_P = 1; return PIPS_OK; }
      if (rank < 0 || rank >= P) PIPS_FAIL(PIPS_ERR_ARG, "distributed root: rank %d of %d", rank, P);
      HIP_TRY(hipSetDevice(device));
      dist_comm = comm; dist_rank = rank; dist_P = P;
      const int ntc = npad / TILE;
      std::vector<TileTask> all;
      dist_diag.assign(ntc, {}); dist_trsm.assign(ntc, {}); dist_next.assign(ntc, {}); dist_upd.assign(ntc, {});
      for (int j = 0; j < ntc; ++j) {
         dist_diag[j].off = (long long)all.size();
         all.push_back({0, j, j, 0});
         dist_diag[j].cnt = 1;
         dist_trsm[j].off = (long long)all.size();
         for (int ti = j + 1; ti < ntc; ++ti) all.push_back({0, ti, j, 0});
         dist_trsm[j].cnt = (int)((long long)all.size() - dist_trsm[j].off);
         dist_next[j].off = (long long)all.size();
         if (j + 1 < ntc && (j + 1) % P == rank)
            for (int ti = j + 1; ti < ntc; ++ti) all.push_back({0, ti, j + 1, j | ((j + 1) << 16)});   // C(ti, tk) -= L(ti, j) U(tk, j)^T
         dist_next[j].cnt = (int)((long long)all.size() - dist_next[j].off);
         dist_upd[j].off = (long long)all.size();
         for (int tk = j + 2; tk < ntc; ++tk)
            if (tk % P == rank)
               for (int ti = tk; ti < ntc; ++ti) all.push_back({0, ti, tk, j | ((j + 1) << 16)});
         dist_upd[j].cnt = (int)((long long)all.size() - dist_upd[j].off);
      }
      int rc = d_dist_tasks.upload(all);
      if (rc) return rc;
      if (!d_panel) PIPS_TRY(d_panel.alloc(((size_t)TILE * TILE + TILE + 8 + 2 * (size_t)npad * TILE)));
      if (!side) {   // one column of lookahead: the bulk of a panel's update runs beside the factorisation and the broadcast of the next column
         HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
         HIP_TRY(hipEventCreateWithFlags(&ev_panel, hipEventDisableTiming));
         HIP_TRY(hipEventCreateWithFlags(&ev_rest, hipEventDisableTiming));
      }
      return PIPS_OK;
   }
   int factor_distributed() {
      const TailCtx c = ctx();
      const int ntc = npad / TILE;
      const size_t ld_bytes = (size_t)npad * sizeof(double);
      bool side_busy = false;
      for (int j = 0; j < ntc; ++j) {
         const int owner = j % dist_P;
         const size_t rows = (size_t)npad - (size_t)(j + 1) * TILE;
         const size_t head = (size_t)TILE * TILE + TILE + 8, count = head + 2 * rows * TILE;
         double* Lp = d_panel + head;
         double* Up = Lp + rows * TILE;
         const size_t col0 = (size_t)(j + 1) * TILE + (size_t)j * TILE * npad;   // first entry below the diagonal tile of column j
         if (owner == dist_rank) {
            launch_tile_diag(c, d_dist_tasks, dist_diag[j], stream);   // (one tile: the list holds the diagonal tile of column j)
            if (dist_trsm[j].cnt > 0) launch_tile_gemm<1>(c, d_dist_tasks, dist_trsm[j], stream);
            // (the owner looks for multipliers a whole-column search would not allow, as on one rank: DenseLdl::check_pivots)
            if (c.bunch_kaufman && c.d_pert_cnt && dist_trsm[j].cnt > 0)
               hipLaunchKernelGGL(k_bk_growth, dim3(TILE), dim3(256), 0, stream, c.d_blks, c.d_arena, j, 1e8, c.d_pert_cnt, c.d_pert_list);
            HIP_TRY(hipMemcpyAsync(d_panel, d_winv + (size_t)j * TILE * TILE, (size_t)TILE * TILE * sizeof(double), hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(d_panel + (size_t)TILE * TILE, d_dtail + (size_t)j * TILE, TILE * sizeof(double), hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemsetAsync(d_panel + (size_t)TILE * TILE + TILE, 0, 8 * sizeof(double), stream));
            if (rows > 0) {
               HIP_TRY(hipMemcpy2DAsync(Lp, rows * sizeof(double), d_R + col0, ld_bytes, rows * sizeof(double), TILE, hipMemcpyDeviceToDevice, stream));
               HIP_TRY(hipMemcpy2DAsync(Up, rows * sizeof(double), d_U + col0, ld_bytes, rows * sizeof(double), TILE, hipMemcpyDeviceToDevice, stream));
            }
         } else if (!pips_hip_comm_has_broadcast(dist_comm))
            HIP_TRY(hipMemsetAsync(d_panel, 0, count * sizeof(double), stream));   // (no broadcast primitive: the panel travels as an all-reduce of zeros)
         int rc = pips_hip_broadcast(dist_comm, d_panel, count, owner, stream);
         if (rc) return rc;
         if (owner != dist_rank) {
            HIP_TRY(hipMemcpyAsync(d_winv + (size_t)j * TILE * TILE, d_panel, (size_t)TILE * TILE * sizeof(double), hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(d_dtail + (size_t)j * TILE, d_panel + (size_t)TILE * TILE, TILE * sizeof(double), hipMemcpyDeviceToDevice, stream));
            if (rows > 0) {
               HIP_TRY(hipMemcpy2DAsync(d_R + col0, ld_bytes, Lp, rows * sizeof(double), rows * sizeof(double), TILE, hipMemcpyDeviceToDevice, stream));
               HIP_TRY(hipMemcpy2DAsync(d_U + col0, ld_bytes, Up, rows * sizeof(double), rows * sizeof(double), TILE, hipMemcpyDeviceToDevice, stream));
            }
         }
         // One column of lookahead.  Panel j is applied in two pieces: this rank's tiles of column j + 1 on the main stream - the owner of that
         // column goes on to factorise and broadcast it - and its columns >= j + 2 (the bulk) on the side stream, beside that.  Column j + 1
         // also takes the bulk of panel j - 1: the main stream joins it first (ev_rest as recorded before this iteration's bulk).
         const bool ahead = side && !knob_set<K_DIST_NO_LOOKAHEAD>();
         hipStream_t bulk = ahead ? side : stream;
         if (ahead) {
            if (side_busy) HIP_TRY(hipStreamWaitEvent(stream, ev_rest, 0));
            HIP_TRY(hipEventRecord(ev_panel, stream));          // panel j is in d_R / d_U on this rank
            HIP_TRY(hipStreamWaitEvent(side, ev_panel, 0));
         }
         if (dist_upd[j].cnt > 0) launch_tile_gemm<3>(c, d_dist_tasks, dist_upd[j], bulk);
         if (ahead) { HIP_TRY(hipEventRecord(ev_rest, side)); side_busy = true; }
         if (dist_next[j].cnt > 0) launch_tile_gemm<3>(c, d_dist_tasks, dist_next[j], stream);
      }
      if (side_busy) HIP_TRY(hipStreamWaitEvent(stream, ev_rest, 0));
      // every rank counted the pivots of its own diagonal tiles: the sum is the inertia
      hipLaunchKernelGGL(k_inertia_to_double, dim3(1), dim3(64), 0, stream, d_inertia, d_panel, 0, d_inertia);
      HIP_TRY(hipMemsetAsync(d_panel + 3, 0, 5 * sizeof(double), stream));
      int rc = pips_hip_allreduce_sum(dist_comm, d_panel, 8, stream);
      if (rc) return rc;
      hipLaunchKernelGGL(k_inertia_to_double, dim3(1), dim3(64), 0, stream, d_inertia, d_panel, 1, d_inertia);
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }

   // A_dev: n x n, symmetric, column-major with the lower triangle authoritative (== row-major with the upper one)
   // rowmajor = 1: A_dev is row-major (the reference's DenseStorage), 0: column-major; lower triangle authoritative
   int factor_dev(const double* A_dev, int lda, int rowmajor) {
      last_A = A_dev; last_lda = lda; last_rowmajor = rowmajor;
      int rc = factor_enqueue();
      check_pending = pivoting == 1;
      return rc;
   }
   int factor_enqueue() {
      const double* A_dev = last_A;
      const int lda = last_lda, rowmajor = last_rowmajor;
      HIP_TRY(hipSetDevice(device));
      if (pivoting == 1) {
         if (!d_pert_cnt) {
            PIPS_TRY(d_pert_cnt.alloc(1));
            PIPS_TRY(d_pert_list.alloc((size_t)2 * std::max(npad, 1)));
         }
         HIP_TRY(hipMemsetAsync(d_pert_cnt, 0, sizeof(int), stream));
      }
      const bool single = single_launch && pivoting == 0 && dist_P <= 1;
      last_single = single;
      if (single) { const int rcs = ensure_single_launch(); if (rcs) return rcs; }
      double* d_work = single ? d_C : d_R;   // where the matrix is accumulated: a scratch copy (single launch) or in place
      hipLaunchKernelGGL(k_copy_lower_to_padded, dim3(grid_for((long long)npad * npad, 256)), dim3(256), 0, stream, A_dev,
                         lda, n, d_work, npad, npad, rowmajor, perm.empty() ? (const int*)nullptr : (const int*)d_perm);
      hipLaunchKernelGGL(k_pref_tail, dim3(8, 1), dim3(256), 0, stream, d_blks, d_work, d_pref, 1);
      hipLaunchKernelGGL(k_block_absmax_init, dim3(1), dim3(256), 0, stream, d_blks, 1);
      hipLaunchKernelGGL(k_block_absmax, dim3(8, 1), dim3(256), 0, stream, d_pref, d_kptr, d_blks);
      hipLaunchKernelGGL(k_block_absmax_finish, dim3(1), dim3(256), 0, stream, d_blks, 1, thr_rel, repl_rel);
      HIP_TRY(hipMemsetAsync(d_inertia, 0, 3 * sizeof(int), stream));
      int rc = single ? factor_single_launch() : (dist_P > 1 ? factor_distributed() : tail_factor(ctx(), nullptr, 0));
      if (rc) return rc;
      factored = true;
      return PIPS_OK;
   }
   int solve_dev(double* x_dev) {
      if (!factored) PIPS_FAIL(PIPS_ERR_STATE, "dense solve called before factor");
      HIP_TRY(hipSetDevice(device));
      int rc = check_pivots();     // (a factorisation whose pivots were not looked at yet: host-pointer callers come here first)
      if (rc) return rc;
      last_solve_path = 0;
      HIP_TRY(hipMemsetAsync(d_xw, 0, (size_t)npad * sizeof(double), stream));
      if (perm.empty()) HIP_TRY(hipMemcpyAsync(d_xw, x_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
      else hipLaunchKernelGGL(k_perm_gather, dim3(grid_for(n, 256)), dim3(256), 0, stream, d_perm, n, x_dev, d_xw, 0, (double*)nullptr);
      rc = tail_fwd(ctx(), d_xw);
      if (rc) return rc;
      rc = tail_bwd(ctx(), d_xw);
      if (rc) return rc;
      if (perm.empty()) HIP_TRY(hipMemcpyAsync(x_dev, d_xw, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
      else hipLaunchKernelGGL(k_perm_gather, dim3(grid_for(n, 256)), dim3(256), 0, stream, d_perm, n, (const double*)nullptr, d_xw, 1, x_dev);
      return PIPS_OK;
   }

   // ---- several right-hand sides (= DeSymIndefSolver::solve(GeneralMatrix&), one dsytrs call for all of them: DeSymIndefSolver.C:120-129).
   // From Engine::multi_knob().from right-hand sides on (8; PIPS_HIP_MULTI as for the leaves) they go through the leaf solver's interleaved
   // tail sweeps - panels of MQ = 32 on the matrix pipe, L read once per panel instead of once per right-hand side (mtail_sweep: the root is
   // one block without a head).  Chunks of at most Engine::MULTI_CHUNK_MAX right-hand sides; k_root_interleave copies in and out of d_xm.
   DevBuf<double> d_xm;             // np * MQ * npad doubles: panel p at d_xm + p * MQ * npad, entry k of right-hand side q at [k * MQ + q]
   int xm_cap = 0;                  // right-hand sides it holds
   DevBuf<double> d_stage;          // the host-pointer entry's copy of a chunk (nr x n; d_in is n x n and nrhs may exceed n)
   int stage_cap = 0;
   int last_solve_path = 0, last_solve_slices = 0, last_solve_rows = 0;   // pips_hip_dense_ldl_info what[5 .. 7]
   static int grow(DevBuf<double>& buf, int& cap, int want, size_t per_rhs, hipStream_t st) {
      if (cap >= want) return PIPS_OK;
      if (buf) HIP_TRY(hipStreamSynchronize(st));   // (work queued on the smaller one)
      buf.reset();
      cap = 0;
      PIPS_TRY(buf.alloc((size_t)want * std::max<size_t>(per_rhs, 1)));
      cap = want;
      return PIPS_OK;
   }
   static bool use_multi(int nrhs) {
      const int from = Engine::multi_knob().from;
      return from > 0 && nrhs >= from;
   }
   // X_dev: nrhs vectors of length n at distance ld >= n on the device, overwritten; asynchronous on the handle's stream.
   // part_of_more: a chunk of a larger set that took the interleaved path (the host-pointer entry): however few, it takes it too
   int solve_multi_dev(double* X_dev, int nrhs, long long ld, bool part_of_more = false) {
      if (!factored) PIPS_FAIL(PIPS_ERR_STATE, "dense solve called before factor");
      HIP_TRY(hipSetDevice(device));
      PIPS_TRY(check_pivots());
      if (!part_of_more && !use_multi(nrhs)) {
         last_solve_path = 0;
         for (int r = 0; r < nrhs; ++r) PIPS_TRY(solve_dev(X_dev + (long long)r * ld));
         return PIPS_OK;
      }
      const int chunk_max = Engine::MULTI_CHUNK_MAX;
      PIPS_TRY(grow(d_xm, xm_cap, (std::min(nrhs, chunk_max) + MQ - 1) / MQ * MQ, (size_t)npad, stream));
      const TailCtx c = ctx();
      const long long ps = (long long)MQ * npad;
      const int* pm = perm.empty() ? (const int*)nullptr : (const int*)d_perm;
      for (int r0 = 0; r0 < nrhs; r0 += chunk_max) {
         const int nr = std::min(chunk_max, nrhs - r0), np = (nr + MQ - 1) / MQ;
         double* X = X_dev + (long long)r0 * ld;
         const dim3 grid(npad / 32, np);
         const int sl = mtail_slices(c, np, Engine::multi_knob().slices);
         hipLaunchKernelGGL(k_root_interleave, grid, dim3(256), 0, stream, X, ld, nr, n, pm, (double*)d_xm, ps, 0);
         mtail_sweep(c, d_xm, ps, np, sl, 0);
         mtail_sweep(c, d_xm, ps, np, sl, 1);
         hipLaunchKernelGGL(k_root_interleave, grid, dim3(256), 0, stream, X, ld, nr, n, pm, (double*)d_xm, ps, 1);
         last_solve_path = 1; last_solve_slices = std::max(sl, 1); last_solve_rows = sl > 0 ? 1 : 0;
      }
      HIP_TRY(hipGetLastError());
      return PIPS_OK;
   }
};

// ---- C ABI of the dense root (C linkage: the names of include/pips_hip.h, whichever namespace the definitions stand in)
extern "C" {

int pips_hip_dense_ldl_create(void** handle, int n, int n_primal, int device) {
   if (!handle || n <= 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_dense_ldl_create: bad arguments");
   int dev;
   int rc = resolve_device(device, &dev);
   if (rc) return rc;
   auto d = std::make_unique<DenseLdl>();
   d->n = n;
   d->n_primal = n_primal;
   d->device = dev;
   // no inertia hint = a plain DeSymIndefSolver replacement: pivot like dsytrf; with a hint the caller vouches for the quasi-definite order
   d->pivoting = n_primal < 0 ? 1 : 0;
   rc = d->init();
   if (rc) return rc;
   *handle = d.release();
   return PIPS_OK;
}

int pips_hip_dense_ldl_set_distributed(void* handle, void* comm, int rank, int n_ranks) {
   DenseLdl* d = (DenseLdl*)handle;
   if (!d) PIPS_FAIL(PIPS_ERR_ARG, "null handle");
   d->factored = false;
   return d->set_distributed(comm, rank, n_ranks);
}

int pips_hip_dense_ldl_set_pivoting(void* handle, int mode) {
   DenseLdl* d = (DenseLdl*)handle;
   if (!d || mode < 0 || mode > 1) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_dense_ldl_set_pivoting: mode 0 (static order) or 1 (Bunch-Kaufman inside the diagonal tiles)");
   d->pivoting = mode;
   d->factored = false;
   return PIPS_OK;
}

int pips_hip_dense_ldl_factor(void* handle, const double* A_host, int lda) {
   DenseLdl* d = (DenseLdl*)handle;
   if (!d || !A_host || lda < d->n) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_dense_ldl_factor: bad arguments");
   HIP_TRY(hipSetDevice(d->device));
   // DenseStorage is row-major with the lower triangle authoritative (DeSymIndefSolver.h:41-42 hands exactly this to
   // dsytrf_('U') as a column-major matrix); upload and let the copy kernel read it transposed.
   if (int rc0 = d->ensure_input_buffer()) return rc0;
   HIP_TRY(hipMemcpy2DAsync(d->d_in, (size_t)d->n * sizeof(double), A_host, (size_t)lda * sizeof(double),
                            (size_t)d->n * sizeof(double), (size_t)d->n, hipMemcpyHostToDevice, d->stream));
   int rc = d->factor_dev(d->d_in, d->n, 1);
   if (rc) return rc;
   if ((rc = d->check_pivots())) return rc;     // (the staged copy d_in stays valid: a new pivot order factorises from it again)
   HIP_TRY(hipStreamSynchronize(d->stream));
   return d->take_root_error("pips_hip_dense_ldl_factor");
}

int pips_hip_dense_ldl_factor_dev(void* handle, const double* A_dev, int lda) {
   DenseLdl* d = (DenseLdl*)handle;
   if (!d || !A_dev || lda < d->n) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_dense_ldl_factor_dev: bad arguments");
   return d->factor_dev(A_dev, lda, 0);
}

int pips_hip_dense_ldl_solve_dev(void* handle, double* rhs_inout_dev) {
   DenseLdl* d = (DenseLdl*)handle;
   if (!d || !rhs_inout_dev) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_dense_ldl_solve_dev: bad arguments");
   return d->solve_dev(rhs_inout_dev);
}

int pips_hip_dense_ldl_solve_multi_dev(void* handle, int nrhs, double* rhs_inout_dev, long long ld) {
   DenseLdl* d = (DenseLdl*)handle;
   if (nrhs < 0 || !d || !rhs_inout_dev || ld < d->n) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_dense_ldl_solve_multi_dev: bad arguments");
   if (nrhs == 0) return PIPS_OK;
   return d->solve_multi_dev(rhs_inout_dev, nrhs, ld);
}

int pips_hip_dense_ldl_solve(void* handle, int nrhs, double* rhs, int ld) {
   DenseLdl* d = (DenseLdl*)handle;
   if (!d || !rhs || nrhs < 0 || ld < d->n) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_dense_ldl_solve: bad arguments");
   HIP_TRY(hipSetDevice(d->device));
   if (DenseLdl::use_multi(nrhs)) {
      // interleaved panels: per chunk one strided copy into a staging buffer of its own, one solve_multi_dev, one copy back, one host stop
      const int chunk_max = Engine::MULTI_CHUNK_MAX;
      const size_t row = (size_t)d->n * sizeof(double);
      PIPS_TRY(DenseLdl::grow(d->d_stage, d->stage_cap, std::min(nrhs, chunk_max), (size_t)d->n, d->stream));
      for (int r0 = 0; r0 < nrhs; r0 += chunk_max) {
         const int nr = std::min(chunk_max, nrhs - r0);
         double* x = rhs + (size_t)r0 * ld;
         HIP_TRY(hipMemcpy2DAsync(d->d_stage, row, x, (size_t)ld * sizeof(double), row, (size_t)nr, hipMemcpyHostToDevice, d->stream));
         PIPS_TRY(d->solve_multi_dev(d->d_stage, nr, d->n, true));
         HIP_TRY(hipMemcpy2DAsync(x, (size_t)ld * sizeof(double), d->d_stage, row, row, (size_t)nr, hipMemcpyDeviceToHost, d->stream));
         HIP_TRY(hipStreamSynchronize(d->stream));
      }
      return d->sweep.take_error("pips_hip_dense_ldl_solve");
   }
   d->last_solve_path = 0;
   if (int rc0 = d->ensure_input_buffer()) return rc0;
   for (int k = 0; k < nrhs; ++k) {
      double* x = rhs + (size_t)k * ld;
      HIP_TRY(hipMemcpyAsync(d->d_in, x, (size_t)d->n * sizeof(double), hipMemcpyHostToDevice, d->stream));
      int rc = d->solve_dev(d->d_in);
      if (rc) return rc;
      HIP_TRY(hipMemcpyAsync(x, d->d_in, (size_t)d->n * sizeof(double), hipMemcpyDeviceToHost, d->stream));
      HIP_TRY(hipStreamSynchronize(d->stream));
   }
   return d->sweep.take_error("pips_hip_dense_ldl_solve");
}

int pips_hip_dense_ldl_inertia(void* handle, int* pos, int* neg, int* zero) {
   DenseLdl* d = (DenseLdl*)handle;
   if (!d || !d->factored) PIPS_FAIL(PIPS_ERR_STATE, "pips_hip_dense_ldl_inertia: factor first");
   HIP_TRY(hipSetDevice(d->device));
   { const int rcp = d->check_pivots(); if (rcp) return rcp; }
   HIP_TRY(hipMemcpyAsync(d->h_inertia, d->d_inertia, 3 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
   HIP_TRY(hipStreamSynchronize(d->stream));
   { const int rce = d->sweep.take_error("pips_hip_dense_ldl_inertia"); if (rce) return rce; }
   { const int rce = d->take_root_error("pips_hip_dense_ldl_inertia"); if (rce) return rce; }
   if (pos) *pos = d->h_inertia[0];
   if (neg) *neg = d->h_inertia[1];
   if (zero) *zero = d->h_inertia[2];
   return PIPS_OK;
}

int pips_hip_dense_ldl_info(void* handle, int64_t* what, int n_what) {
   DenseLdl* d = (DenseLdl*)handle;
   if (!d || !what || n_what < 0) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_dense_ldl_info: bad arguments");
   const int64_t v[8] = {d->factored && d->last_single ? 1 : 0, d->npad / TILE, d->dist_P, d->pivoting, d->bk_refactorizations,
                         d->last_solve_path, d->last_solve_slices, d->last_solve_rows};
   for (int i = 0; i < n_what && i < 8; ++i) what[i] = v[i];
   return PIPS_OK;
}

void pips_hip_dense_ldl_destroy(void* handle) { delete (DenseLdl*)handle; }

}  // extern "C"
