/* pips_hip.h — C ABI of the MI355X-native KKT linear-system backend for PIPS-IPM++ (libpipship.so).
 *
 * Every entry point returns 0 on success and a non-zero PIPS_ERR_* code on failure; pips_hip_last_error() gives the
 * message.  The C++ adapter maps non-zero onto the reference's convention of printing and calling
 * MPI_Abort (PardisoSolver.C:201-204,222-225).  No call throws, none takes or returns a C++/torch type.
 *
 * "host" pointers are ordinary memory, "dev" pointers are HIP device memory of the device the handle was created on.
 * All matrices are CSR, row-major, 0-based, int32 indices, fp64 values (SparseStorage.h:45-50).
 */
#ifndef PIPS_HIP_H
#define PIPS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* pips_hip_last_error(void);
/* how often this process has made the host wait for the device inside the library so far (stream / event / device synchronisations and
 * blocking copies, all counted at one place: csrc/common.h) - a diagnostic: the difference around a call sequence is its number of host stops */
long long pips_hip_host_wait_count(void);
/* the same per call site, as lines "file:line count" written into buf (at most cap bytes, NUL-terminated); returns the bytes written */
int pips_hip_host_wait_sites(char* buf, int cap);
/* device and pinned host allocations the library holds right now, and their bytes (every one is made at one place: csrc/devmem.h) -
 * a diagnostic: equal values before and after a create ... destroy sequence mean that nothing leaked */
long long pips_hip_device_allocs_live(void);
long long pips_hip_device_bytes_live(void);
/* the environment switches the library reads - every one of them, from the one table they are read through (csrc/knobs.h) - as lines
 * "name kind default when effect" written into buf (at most cap bytes, NUL-terminated); returns the bytes written.  kind: set (present, any
 * value), int, tri (-1 not set, else 0 / 1), real, text; default "-": none; when: create, analyze, call, process, or two of them joined by "+" */
int pips_hip_knobs(char* buf, int cap);
/* what the library would make of the switch `name` right now: *value is the parsed number (set and text: whether the variable is there),
 * text (may be NULL; at most cap bytes) the value of a text switch, else empty.  PIPS_ERR_ARG for a name that is not in the table.
 * Neither call touches the device. */
int pips_hip_knob_value(const char* name, double* value, char* text, int cap);
/* number of visible HIP devices (0 without a GPU; never fails) */
int pips_hip_device_count(void);

/* ---------------------------------------------------------------------------------------------------------------
 * 1. Leaf solver handle: drop-in for DoubleLinearSolver behind DistributedFactory::make_leaf_solver
 *    (DoubleLinearSolver.h:24-72, DistributedFactory.cpp:66-112).  Replaces PardisoSolver / Ma27Solver / Ma57Solver.
 * ------------------------------------------------------------------------------------------------------------- */
/* pattern of the lower-triangular CSR matrix the solver will factorise (SparseSymmetricMatrix, isLower;
 * PardisoSolver.C:51-135 reads the same krowM/jcolM).  The arrays are copied.  device < 0: current device. */
int pips_hip_ldl_create(void** handle, int n, const int* krow, const int* jcol, int device, int flags);
/* optional: the leading n_primal rows are expected to yield positive pivots, the rest negative
 * (= the inertia the regularisation loop asks for: DistributedLeafLinearSystem.C:22, LinearSystem.C:296-325) */
int pips_hip_ldl_set_inertia_hint(void* handle, int n_primal);
/* relative pivot threshold / replacement (times max|K|); PARDISO's counterpart is the 1e-8 pivot perturbation */
int pips_hip_ldl_set_pivot_rule(void* handle, double thr_rel, double repl_rel);
/* iterative refinement of every solve: at most max_steps steps; tol > 0 stops as soon as ||r||inf <= tol*||rhs||inf
 * (PARDISO: iparm[7]=2, PardisoProjectSolver.C:72), tol = 0 always does max_steps steps.  Default (1, 0). */
int pips_hip_ldl_set_refinement(void* handle, int max_steps, double tol);
/* same, the stopping test being the normwise backward error ||r||inf / (max|K| ||x||inf + ||rhs||inf) <= tol - what PARDISO's adaptive
 * refinement looks at; solve(nrhs) decides per right-hand side (the measures of a chunk read back with one copy, the correction solve only for
 * the columns whose first solve was not accurate enough).  The adapters use (2, 1e-15): iparm[7] = 2, PardisoProjectSolver.C:72 */
int pips_hip_ldl_set_refinement_backward_error(void* handle, int max_steps, double tol);
/* deterministic mode of this leaf (see pips_hip_batch_set_deterministic): factor(), solve() and solve(nrhs) repeat to the bit - no FP64
 * atomics on their path; several right-hand sides go panel by panel through the slot / gather forward substitution.  Before the first
 * factorisation.  (The reference's breakdown tests compare bitwise between runs: pipsdef.h:35,108.) */
int pips_hip_ldl_set_deterministic(void* handle, int on);
/* symbolic phase (ordering, supernodes, device allocation); pattern-only, done once */
int pips_hip_ldl_analyze(void* handle);
/* = DoubleLinearSolver::matrixChanged(): numeric LDL^T of the current values (host array of length nnz, CSR order) */
int pips_hip_ldl_factor(void* handle, const double* vals_host);
/* the values alone (host array of length nnz, CSR order), the leaf handle's twin of pips_hip_batch_set_values: uploads them and keeps the
 * factors.  Later solves refine against these values with the factors they have - the sweeps read the factors only, the residual and the
 * measure of the refinement read the values.  PIPS_ERR_STATE before the first factorisation, and for a handle whose newest factors are a
 * batch's (pips_hip_ldl_factor_schur_batch). */
int pips_hip_ldl_set_values(void* handle, const double* K_val_host);
/* = DoubleLinearSolver::solve(int nrhss, double* rhss, int* colSparsity) (PardisoSolver.C:276-352): nrhs contiguous
 * right-hand sides of length ld >= n, overwritten by the solutions; all-zero right-hand sides are left out of the transfer and
 * of the solve, as the reference's packing does.  nrhs = 1 is DoubleLinearSolver::solve(Vector&). */
int pips_hip_ldl_solve(void* handle, int nrhs, double* rhs_inout_host, int ld);
/* = DoubleLinearSolver::get_inertia(): (positive, negative, zero/perturbed) pivots of the last factorisation */
int pips_hip_ldl_inertia(void* handle, int* pos, int* neg, int* zero);
/* The leaf's Schur term computed where the factor lives (INTEGRATION.md level 1.5): replaces the host's K4-K6 chunk loop
 * (addBiTLeftKiBiRightToResBlockedParallelSolvers, DistributedLinearSystem.C:766-1047; caller DistributedLeafLinearSystem.C:214-252),
 * which ships every border column dense over PCIe and back.
 *   set_border     before the analysis: pattern of Br_i^T, CSR with S rows (Schur column ids) over the n rows of K_i
 *                  (border_left_transp); empty rows are skipped as the reference skips empty border columns (:870-874)
 *   factor_schur   = matrixChanged() + addTermToSchurComplBlocked(): factorises K_i (values as in pips_hip_ldl_factor) and adds
 *                  -Br_i^T K_i^-1 Br_i to SC_host, the S x S row-major DenseSymmetricMatrix storage (lower triangle, ldSC >= S);
 *                  solves and inertia queries work afterwards as after pips_hip_ldl_factor */
int pips_hip_ldl_set_border(void* handle, int S, const int* Bt_rowptr, const int* Bt_colidx);
int pips_hip_ldl_factor_schur(void* handle, const double* K_vals_host, const double* Bt_vals_host, double* SC_host, int ldSC);
/* Variants of the solve.  solve_dev: the right-hand sides are device memory (nrhs vectors at distance ld >= n; no PCIe, asynchronous on
 * the handle's stream).  solve_sparse = DoubleLinearSolver::solve(int nrhss, double* rhss, int* colSparsity) with the third argument
 * honoured: col_sparsity[i] != 0 marks the rows that can be non-zero in any right-hand side (the border's row pattern the caller builds,
 * DistributedLinearSystem.C:903); only those rows of the non-zero right-hand sides travel to the device.  NULL: same as pips_hip_ldl_solve. */
int pips_hip_ldl_solve_dev(void* handle, int nrhs, double* rhs_inout_dev, long long ld);
int pips_hip_ldl_solve_sparse(void* handle, int nrhs, double* rhs_inout_host, int ld, const int* col_sparsity);
/* Array-of-handles entries (INTEGRATION.md level 1.5b): the leaf solvers of a rank run as ONE batch from the host's loop over its children
 * (sLinsysRootAug::assembleLocalKKT :210-227; Lsolve / Ltsolve :323-365).  The first call binds the handles (created, borders set, same
 * Schur dimension and device; the same array in the same order afterwards) into one batch engine analysed over all of them.
 *   factor_schur_batch  = for every leaf matrixChanged() + addTermToSchurComplBlocked(): K_vals_host[i] / Bt_vals_host[i] are leaf i's
 *                         values (CSR order); adds sum_i -Br_i^T K_i^-1 Br_i to SC_host (row-major, lower triangle, ldSC >= S) with one
 *                         S x S buffer on the device and one transfer; SC_host == NULL: factorise only
 *   solve_batch         one right-hand side per leaf (host pointers of length n_i, NULL = none for that leaf), overwritten
 *   solve_batch_dev     the flat device vector of all leaves, block after block
 *   inertia_batch       per leaf (positive, negative, zero / perturbed)
 * pips_hip_ldl_inertia / pips_hip_ldl_solve on a bound handle go through the batch (a single-leaf solve then costs a batch solve). */
int pips_hip_ldl_factor_schur_batch(void* const* handles, int n, const double* const* K_vals_host, const double* const* Bt_vals_host,
                                    double* SC_host, int ldSC);
int pips_hip_ldl_solve_batch(void* const* handles, int n, double* const* rhs_inout_host);
int pips_hip_ldl_solve_batch_dev(void* const* handles, int n, double* x_dev);
int pips_hip_ldl_inertia_batch(void* const* handles, int n, int* pos, int* neg, int* zero);
/* The same two entries for a host whose Schur complement is sparse (hasSparseKkt): the branch sparse_res = true of
 * addBiTLeftKiBiRightToResBlockedParallelSolvers (DistributedLinearSystem.C:766-770, 1050-1113, 1180-1190), which adds the term into a
 * SparseSymmetricMatrix through multMatSymUpper.  sc_rowptr / sc_colidx: the CSR pattern of one triangle of the symmetric S x S Schur
 * complement - lower = 0 the upper one (row i holds columns >= i: the reference's SparseSymmetricMatrix of the sparse KKT), lower = 1 the
 * lower one (what pips_hip_kkt_get_schur_sparse returns); sc_val_host its sc_rowptr[S] values.  The call factorises as the dense entry
 * does and ADDS the term's entries at their positions; every other value keeps its bits.  Solves, inertia and info afterwards as after
 * the dense entries.  A leaf without non-empty border columns adds nothing; sc_val_host == NULL (batch entry): factorise only.
 * Only the rows of the leaves' non-empty border columns are consulted; their columns must ascend, and they must hold the clique of
 * every leaf's non-empty border columns, the diagonal included.
 * The device never holds S x S nor sc_rowptr[S] doubles: the target is the T distinct pattern positions the leaves' cliques touch (one
 * leaf: the lower half of its own nb x nb block), addressed through the position tables of the sparse root; one copy of T doubles
 * comes back per call.  The host keeps those T positions, S, the number of entries and a 64-bit hash of the consulted rows.
 * Errors, all before any value of sc_val_host changes:
 *   PIPS_ERR_ARG    S differs from the border's; a consulted row does not ascend or holds an index out of range; a later call passes
 *                   another pattern (S, entries, triangle or the hash differ)
 *   PIPS_ERR_STATE  the pattern lacks an entry of a leaf's clique - the message names it as (row, column); the handle or the bound
 *                   group has had a dense Schur target (pips_hip_ldl_factor_schur / _batch), or the dense entries are called after
 *                   these: one kind per handle for its life
 * Deterministic mode: pips_hip_ldl_set_deterministic on the handle (batch entry: on the first handle), or PIPS_HIP_DETERMINISTIC=1 in the
 * environment at the first call. */
int pips_hip_ldl_factor_schur_sparse(void* handle, const double* K_vals_host, const double* Bt_vals_host, int S, const int* sc_rowptr,
                                     const int* sc_colidx, double* sc_val_host, int lower);
int pips_hip_ldl_factor_schur_sparse_batch(void* const* handles, int n, const double* const* K_vals_host, const double* const* Bt_vals_host,
                                           int S, const int* sc_rowptr, const int* sc_colidx, double* sc_val_host, int lower);
/* diagnostics of the symbolic phase: what[0]=nnz(L) what[1]=n_head what[2]=tail m what[3]=#head supernodes
 * what[4]=#levels what[5]=factor flops (rounded); and what[6]=refinement steps the last solve took (solve(nrhs) goes chunk by chunk: the
 * steps of the last chunk that took any, not their sum), what[7]=how the last solve(nrhs) went
 * (0 one sweep per right-hand side, 1 interleaved panels on the matrix pipe, 2 the same with the deterministic forward substitution);
 * of the engine that holds the leaf's newest factors (its own, or the batch it is bound into): what[8]=the Schur mode its analysis took
 * (1 augmented partial factorisation, 2 blocked solves), what[9]=doubles of its compact sparse Schur target (0: none) */
int pips_hip_ldl_info(void* handle, int64_t* what, int n_what);
/* copies the fill-reducing permutation (perm[k] = original index eliminated k-th) */
int pips_hip_ldl_get_perm(void* handle, int* perm);
void pips_hip_ldl_destroy(void* handle);

/* ---------------------------------------------------------------------------------------------------------------
 * 2. Dense root solver: drop-in for DeSymIndefSolver (DeSymIndefSolver.C:56-168; dsytrf_/dsytrs_).
 * ------------------------------------------------------------------------------------------------------------- */
/* n_primal >= 0: inertia hint (rows [0, n_primal) are expected to give positive pivots, the rest negative ones) - the caller vouches
 * for a quasi-definite order and the factorisation keeps it (static pivots); n_primal < 0: no hint, the matrix is pivoted like
 * dsytrf does: Bunch-Kaufman 1 x 1 / 2 x 2 pivots, the search bounded to the 128 x 128 diagonal tiles.
 * pips_hip_dense_ldl_set_pivoting overrides: 0 static order, 1 Bunch-Kaufman. */
int pips_hip_dense_ldl_create(void** handle, int n, int n_primal, int device);
int pips_hip_dense_ldl_set_pivoting(void* handle, int mode);
/* With the static order on one rank the factorisation is ONE launch of tile tasks that wait for each other through flags
 * (csrc/rootkernel.hip.h), in the order of a list schedule the host builds once per dimension (csrc/rootplan.cpp).  This entry returns
 * that schedule for ntc tile columns of 128 (no device involved; tests): (kind 0 update / 1 trsm / 2 diagonal tile, tile row, tile column,
 * k0 | k1 << 16) quadruples - the bulk list, then the chain's list, each in ticket order.  workers, qmin <= 0, urgent, chain_slots < 0:
 * the defaults.  out may be NULL (counts only). */
int pips_root_plan_build(int ntc, int workers, int qmin, int urgent, int chain_slots, int* out, long long cap, long long* n_tasks,
                         long long* n_chain_tasks, double* makespan_us);
/* Several ranks hold the same matrix (the reduced Schur complement): factorise it column-cyclically over the ranks instead of
 * redundantly on each (DistributedRootLinearSystem.C:1436-1464 does the latter).  Tile column j belongs to rank j mod n_ranks; the
 * owner's panel reaches every rank through the communicator (pips_hip_comm_create / _create_external), every rank ends with the
 * complete factor and solves locally.  Collective: every rank must call factor with the same matrix.  comm == NULL or n_ranks <= 1
 * switches it off.  Fused path: PIPS_HIP_ROOT_DISTRIBUTED=1. */
int pips_hip_dense_ldl_set_distributed(void* handle, void* comm, int rank, int n_ranks);
/* = DeSymIndefSolver::matrixChanged(): A is the n x n row-major DenseSymmetricMatrix storage (DenseStorage.C:64-83,
 * lower triangle authoritative, lda = n); it is copied to the device and factorised */
int pips_hip_dense_ldl_factor(void* handle, const double* A_host, int lda);
/* factorise a matrix that already lives on the device in column-major-lower form (fused path, see section 3) */
int pips_hip_dense_ldl_factor_dev(void* handle, const double* A_dev, int lda);
/* = DeSymIndefSolver::solve: nrhs vectors of length n at distance ld >= n in host memory, overwritten with the solutions.  Fewer than 8
 * right-hand sides (PIPS_HIP_MULTI as for the leaf solver: set non-zero 2, set to 0 never) are solved one at a time; from there on in
 * chunks of at most 256 through interleaved panels of 32 on the matrix pipe, the factor read once per panel (= the one dsytrs call of
 * DeSymIndefSolver::solve(GeneralMatrix&), DeSymIndefSolver.C:120-129), with one host stop per chunk. */
int pips_hip_dense_ldl_solve(void* handle, int nrhs, double* rhs_inout_host, int ld);
int pips_hip_dense_ldl_solve_dev(void* handle, double* rhs_inout_dev);
/* ... the same for nrhs vectors at distance ld >= n in device memory, overwritten; asynchronous on the handle's stream.  nrhs == 0 is a
 * no-op.  PIPS_ERR_ARG for a null pointer, nrhs < 0, ld < n; PIPS_ERR_STATE before a factorisation. */
int pips_hip_dense_ldl_solve_multi_dev(void* handle, int nrhs, double* rhs_inout_dev, long long ld);
int pips_hip_dense_ldl_inertia(void* handle, int* pos, int* neg, int* zero);
/* diagnostics (read-only; tests assert which path ran): what[0]=1 if the last factorisation was the single launch, what[1]=tile columns
 * of 128, what[2]=ranks the factorisation is distributed over, what[3]=pivoting mode, what[4]=how often Bunch-Kaufman pivoting had to
 * factorise again under a new order since the handle was created, what[5]=how the last solve call went (0 one sweep pair per
 * right-hand side, 1 interleaved panels), what[6]=slices per panel of the last interleaved solve (1, 2, 4; 0: none yet), what[7]=1 if
 * its tail sweeps were the single launches, 0 the launches per tile column */
int pips_hip_dense_ldl_info(void* handle, int64_t* what, int n_what);
void pips_hip_dense_ldl_destroy(void* handle);

/* ---------------------------------------------------------------------------------------------------------------
 * 3. Batched, device-resident fast path for all leaves owned by one GPU.  Replaces the host loops of
 *    DistributedRootLinearSystem::factor2 (:206-243), sLinsysRootAug::assembleLocalKKT (:210-227),
 *    DistributedLeafLinearSystem::addTermToSchurComplBlocked (:214-252) with
 *    addBiTLeftKiBiRightToResBlockedParallelSolvers / addLeftBorderTimesDenseColsToResTranspDense
 *    (DistributedLinearSystem.C:766-1047,1115-1175), and the leaf parts of Lsolve/Ltsolve
 *    (addLniziLinkCons DistributedLeafLinearSystem.C:171-212, LniTransMult DistributedLinearSystem.C:430-483).
 * ------------------------------------------------------------------------------------------------------------- */
/* S = dimension of the root Schur complement (n0 + my0 + myl + mzl); stream: hipStream_t or NULL (default stream) */
int pips_hip_batch_create(void** handle, int n_blocks, int S, int device, void* stream);
/* block b: lower CSR pattern of K_b (n x n), leading primal rows, and Br_b^T as CSR with S rows over n columns
 * (build it with pips_border_assemble); Bt_* may be NULL for a block without border.  Arrays are copied. */
int pips_hip_batch_set_block(void* handle, int b, int n, int n_primal, const int* K_rowptr, const int* K_colidx,
                             const int* Bt_rowptr, const int* Bt_colidx, const double* Bt_val);
int pips_hip_batch_set_options(void* handle, int force_n_head, int refine_steps, double thr_rel, double repl_rel);
/* How the Schur contribution SC -= Br^T K^-1 Br is formed.  1: augmented partial factorisation (border columns ride as rows
 * of every panel; dense MFMA work - the PardisoSchurSolver idea, PardisoSchurSolver.C:83-389).  2: blocked solves with the
 * plain factor, 32 border columns at a time over all blocks (addTermToSchurComplBlocked, DistributedLeafLinearSystem.C:
 * 214-252 + DistributedLinearSystem.C:766-1175: densify, multi-RHS solve, sparse border times dense columns).  0 (default):
 * chosen at analyze time from the symbolic flop / byte counts - dense factors take 1, sparse structured ones 2.
 * Call before analyze; get_schur_mode reports the choice. */
int pips_hip_batch_set_schur_mode(void* handle, int mode);
int pips_hip_batch_get_schur_mode(void* handle, int* mode);
/* Deterministic mode (call before analyze): bit-identical factors, Schur complement, inertia and solutions from run to run, at a
 * cost in time and memory ("deterministic mode").  By default the head scatter, the Schur accumulation over the
 * blocks and the head substitution use hardware FP64 atomics, whose order of arrival decides the last bits - the reference's
 * breakdown tests (PIPSisZero, pipsdef.h:35,108) and any bitwise comparison between runs see that. */
int pips_hip_batch_set_deterministic(void* handle, int on);
/* add_regularization_local_kkt (DistributedLeafLinearSystem.C:108-143): K diagonal += primal on the leading n_primal rows
 * of every block, -= dual on the remaining rows; used by the inertia-correcting loop (LinearSystem.C:296-325) */
int pips_hip_batch_add_regularization(void* handle, double primal, double dual);
/* iterative refinement policy of pips_hip_batch_solve* (see pips_hip_ldl_set_refinement); default (1, 0) */
int pips_hip_batch_set_refinement(void* handle, int max_steps, double tol);
/* same, but the stopping test is the normwise backward error  ||r_b||inf / (max|K_b| ||x_b||inf + ||rhs_b||inf) <= tol
 * for every block b — the criterion PARDISO's iparm[7] refinement uses ("stops if a satisfactory level of accuracy of the
 * solution in terms of backward error is achieved") */
int pips_hip_batch_set_refinement_backward_error(void* handle, int max_steps, double tol);
/* error measure the last adaptive solve saw at its final check */
double pips_hip_batch_last_refinement_measure(void* handle);
/* refinement steps the last solve actually took */
int pips_hip_batch_last_refinement_steps(void* handle);
/* symbolic phase for all blocks (n_threads host threads) + device setup */
int pips_hip_batch_analyze(void* handle, int n_threads);
/* upload all values of K_b (CSR order, host) — needed once; afterwards only diagonals change (a2).  It only copies: factors that exist
 * stay as they are and stay in use (it has always behaved this way), so solves between this call and the next pips_hip_batch_factor sweep
 * with the old factors and refine against the new values */
int pips_hip_batch_set_values(void* handle, int b, const double* K_val_host);
/* K diagonals of all blocks from one flat device vector (block after block, rows in [x|y|z] order):
 * put_primal_diagonal / clear_dual_equality_diagonal / put_dual_inequalites_diagonal / add_regularization_local_kkt
 * (DistributedLeafLinearSystem.C:88-143) collapsed into one scatter */
int pips_hip_batch_set_diagonals_dev(void* handle, const double* diag_dev);
int pips_hip_batch_set_diagonals(void* handle, const double* diag_host);
/* factor every K_b and accumulate  SC -= sum_b Br_b^T K_b^-1 Br_b  into SC_dev: S x S, column-major with leading
 * dimension ldSC, lower triangle written (== the upper triangle of the reference's row-major layout's transpose; the
 * matrix is symmetric).  SC_dev may be NULL to factor only.  Asynchronous on the handle's stream. */
int pips_hip_batch_factor(void* handle, double* SC_dev, int ldSC);
/* x_b := K_b^-1 x_b for every block; x_dev is the flat vector of all blocks (sum of n).  Asynchronous. */
int pips_hip_batch_solve_dev(void* handle, double* x_dev);
int pips_hip_batch_solve(void* handle, double* x_host);
/* b0 += alpha * sum_b Br_b^T z_b   (addLniziLinkCons uses alpha = -1) */
int pips_hip_batch_border_tmult_dev(void* handle, const double* z_dev, double* b0_dev, double alpha);
/* t_b += alpha * Br_b x0 for every block   (LniTransMult) */
int pips_hip_batch_border_mult_dev(void* handle, const double* x0_dev, double* t_dev, double alpha);
/* The same two products on nrhs vectors, the border read once for all of them (the kernels pips_hip_kkt_solve_compressed_multi runs
 * between its panel solves; not in deterministic mode, whose form of the first product is reached through that call alone - PIPS_ERR_STATE):
 *   tmult_panel:  T(s, q) += alpha * sum_b (Br_b^T z_b(q))_s;  vector q of Z at Z_dev + q * ldz (ldz >= sum of n), T(s, q) at
 *                 T_dev[s * ldt + q] (S rows of ldt >= nrhs doubles: the layout the kernel's atomic adds are contiguous in);
 *   mult_panel:   W(:, q) = alpha * Br X0(:, q) for every block - a store, rows without border entries get zeros;  vector q of X0 at
 *                 X0_dev + q * ldx (ldx >= S), of W at W_dev + q * ldw (ldw >= sum of n).
 * Asynchronous on the batch's stream; nrhs == 0 does nothing. */
int pips_hip_batch_border_tmult_panel_dev(void* handle, int nrhs, const double* Z_dev, long long ldz, double* T_dev, long long ldt, double alpha);
int pips_hip_batch_border_mult_panel_dev(void* handle, int nrhs, const double* X0_dev, long long ldx, double* W_dev, long long ldw, double alpha);
int pips_hip_batch_inertia(void* handle, int b, int* pos, int* neg, int* zero);
/* the factorised dense tail of block b as it lies in device memory (tests compare two kernels' factors entry for entry): which = 0 the tail
 * panel, column-major ldT x m_pad (m_pad tail rows - D on the diagonal, L below it - then the border rows), 1 its scaled copy U = L D,
 * m_pad x m_pad (tiles strictly below the tile diagonal only), 2 the pivots d (m_pad).  dims[0..3] = m, m_pad, nb, ldT; out may be NULL
 * (dimensions only), n_out = the doubles it holds.  Waits for the handle's stream. */
int pips_hip_batch_tail_to_host(void* handle, int b, int which, double* out, int64_t n_out, int* dims);
/* what[0]=sum nnz(L) what[1]=sum n what[2]=sum n_head what[3]=sum tail m what[4]=#head supernodes what[5]=max levels
 * what[6]=factor flops what[7]=border (TRSM+SYRK) flops what[8]=arena bytes what[9]=max tail tile columns
 * what[10]=bytes of the head-to-head update position tables what[11]=sum of non-empty border columns what[12]=sum nnz(K lower)
 * what[13]=1 if solveCompressed takes its Ltsolve from the augmented factor (one backward sweep) while no pivot is perturbed
 * what[14]=1 multifrontal head ... what[24]=blocks analysed with the border split of the fronts; what[26]=right-hand sides of the packed
 * blocked solves (max over the blocks of their non-empty border columns; Schur mode 2 with the sparse root), 0 where that path is
 * not active; what[27]=1 where the tails are written once, assembled in LDS column by column (k_tail_first_touch: multifrontal head, no
 * deterministic mode, tallest tail column within the LDS budget; PIPS_HIP_TAIL_FIRST_TOUCH=0 refuses it), 0 where they are cleared and
 * added to (python/capi.py LeafBatch.info names all) */
int pips_hip_batch_info(void* handle, int64_t* what, int n_what);
int pips_hip_batch_sync(void* handle);
/* per-phase device time in ms (HIP events on the handle's stream) of the last pips_hip_batch_factor
 *   ms[0]=scatter ms[1]=head ms[2]=tail update GEMM ms[3]=tail diag ms[4]=tail trsm ms[5]=Schur SYRK ms[6]=total
 * and, summed over the solves since that factorisation,
 *   ms[7]=permute in/out ms[8]=head forward ms[9]=tail sweeps + D ms[10]=head backward ms[11]=refinement residual + norms
 * cnt[i] = number of records of phase i (n <= 16).  Enable with pips_hip_batch_set_timing(handle, 1). */
int pips_hip_batch_set_timing(void* handle, int on);
int pips_hip_batch_get_timing(void* handle, double* ms, int64_t* cnt, int n);
void pips_hip_batch_destroy(void* handle);

/* ---------------------------------------------------------------------------------------------------------------
 * 3b. Fused two-level system of one rank: leaves + replicated dense root + Schur reduction.
 *     factorize      = DistributedRootLinearSystem::factor2 (:206-243): initializeKKT, children factor2, assembleLocalKKT,
 *                      reduceKKT, finalizeKKT (sLinsysRootAug::finalizeKKTdense :1769-1796), factorizeKKT
 *     solve_compressed = DistributedLinearSystem::solveCompressed (:409-420): Lsolve / Dsolve / Ltsolve
 *                      (sLinsysRootAug.C:323-365); root vector layout [x0 | y0 | ylink | zlink] (mz0 = 0)
 * ------------------------------------------------------------------------------------------------------------- */
/* batch: analyzed leaf batch (created with the same S).  A0 (my0 x n0), F0 (myl x n0), G0 (mzl x n0) are the root's own
 * constraint blocks (CSR, may be NULL).  comm: handle from pips_hip_comm_create or NULL when n_ranks == 1. */
int pips_hip_kkt_create(void** handle, void* batch, int n0, int my0, int myl, int mzl, const int* A0_rowptr,
                        const int* A0_colidx, const double* A0_val, const int* F0_rowptr, const int* F0_colidx,
                        const double* F0_val, const int* G0_rowptr, const int* G0_colidx, const double* G0_val, void* comm,
                        int rank, int n_ranks);
/* leaf_diag_dev: flat K diagonals of this rank's blocks (NULL: keep); xdiag0_dev: n0 primal diagonal of the root
 * (xDiag); zdiag_link_dev: mzl entries or NULL.  Asynchronous on the batch's stream. */
/* Sparse-root variant of pips_hip_kkt_create (createSchurCompSymbSparseUpper DistributedProblem.cpp:2235+,
 * finalizeKKTsparse sLinsysRootAug.C:1629-1739, PardisoIndefSolver as root solver): the Schur complement is kept as the value
 * array of a lower-triangular CSR pattern - dense x0 block, per block the clique on its non-empty border columns, the root
 * rows A0 / F0 / G0, full diagonal - and factorised / solved by the same sparse LDL^T machinery as the leaves.  Meant for
 * 2-link structure (a linking row touches two blocks), where SC is sparse and S may be far beyond what S x S storage allows.
 * blk_cols_ptr / blk_cols: border column sets (ascending Schur column ids) of ALL n_blocks_global blocks of the problem -
 * required with n_ranks > 1 so that every rank reduces the same value array; NULL = the blocks of this batch.
 * The batch must be analyzed; either Schur mode works.  Mode 1 accumulates into the value array from the augmented factorisation;
 * mode 2 forms it by blocked solves packed by block-local column (right-hand side q carries every block's q-th non-empty border
 * column: max_b nb_b right-hand sides, pips_hip_batch_info what[26]) and, as with the dense root, leaves solveCompressed on path 0. */
int pips_hip_kkt_create_sparse(void** handle, void* batch, int n0, int my0, int myl, int mzl, const int* A0_rowptr,
                               const int* A0_colidx, const double* A0_val, const int* F0_rowptr, const int* F0_colidx,
                               const double* F0_val, const int* G0_rowptr, const int* G0_colidx, const double* G0_val,
                               int n_blocks_global, const int* blk_cols_ptr, const int* blk_cols, void* comm, int rank,
                               int n_ranks);
/* pattern and values (host copies) of the sparse Schur complement; any output may be NULL; *nnz = number of entries */
int pips_hip_kkt_get_schur_sparse(void* handle, int* nnz, int* rowptr, int* colidx, double* val_host);
/* what[0] = elimination order of the sparse root: 0 minimum degree, 1 linking rows then x0 as a band of dense tiles, 2 linking rows
 * dissected around x0 / the root equality rows (a chain-like Schur complement becomes a tree of small fronts: default where the tile
 * envelope is thin; PIPS_HIP_SPARSE_ROOT_BAND=0|1|2 forces one); what[1 + i] = pips_hip_batch_info entry i of the root's engine */
int pips_hip_kkt_sparse_root_info(void* handle, int64_t* what, int n_what);
int pips_hip_kkt_factorize(void* handle, const double* leaf_diag_dev, const double* xdiag0_dev, const double* zdiag_link_dev);
/* sLinsysRootAug::add_regularization_local_kkt (sLinsysRootAug.C:1545-1600) as a setting of the following factorizations: the
 * x0 diagonal of the Schur complement gets + primal, the diagonal of its dual rows (y0, y_link, z_link) - dual; (0, 0) = off */
int pips_hip_kkt_set_root_regularization(void* handle, double primal, double dual);
/* root inequality rows C0 (mz0 x n0, CSR): adds -C0^T diag(zdiag0)^-1 C0 to SC at every factorize (sLinsysRootAug.C:
 * 1276-1338) and the z0 elimination to solve_compressed (:384-466); zdiag0 (< 0, = nOmegaInv of the root, caller-owned
 * device vector of mz0 entries) must be set before pips_hip_kkt_factorize */
int pips_hip_kkt_set_root_inequalities(void* handle, int mz0, const int* C0_rowptr, const int* C0_colidx, const double* C0_val);
int pips_hip_kkt_set_zdiag0_dev(void* handle, const double* zdiag0_dev);
/* Q0, the Hessian of the first-stage variables (n0 x n0, lower-triangular CSR, diagonal included): constant lower-triangular entries
 * added to the x0 block of the Schur complement at every factorize (sLinsysRootAug.C:234-261), after the reduction over the ranks and on
 * every rank, like xdiag0.  Dense and sparse root alike (the sparse root's pattern holds the dense x0 block).  Entries given twice are added up.  A second call
 * replaces the entries, Q0_rowptr == NULL removes them.  PIPS_ERR_ARG for an entry outside the lower triangle, PIPS_ERR_STATE if the sparse
 * root's pattern has no place for one. */
int pips_hip_kkt_set_root_hessian(void* handle, const int* Q0_rowptr, const int* Q0_colidx, const double* Q0_val);
/* in place: b0 (replicated on every rank; [x0 | y0 | ylink | zlink], or [x0 | y0 | z0 | ylink | zlink] when mz0 > 0) and
 * the flat leaf vector of this rank's blocks */
int pips_hip_kkt_solve_compressed(void* handle, double* b0_dev, double* b_leaf_dev);
/* solveCompressed for nrhs right-hand sides on one factorisation (the reference: addBlTKiInvBrToResBlockwise's LsolveHierarchyBorder /
 * DsolveHierarchyBorder / LtsolveHierarchyBorder on a buffer of SC_BLOCKSIZE_HIERARCHICAL columns, sLinsysRootAug.C:1815-1940).
 * Column q of B0_dev starts at B0_dev + q * ld0 and has the layout pips_hip_kkt_solve_compressed takes (S + mz0 entries); column q of
 * Bleaf_dev is the flat leaf vector of this rank's blocks at Bleaf_dev + q * ldl.  Both are overwritten in place, asynchronously on the
 * batch's stream except where adaptive refinement makes the host wait; entries between the columns (ld0 > S + mz0, ldl > n_total) are
 * neither read nor written.  nrhs == 0 does nothing.
 *   nrhs below the threshold of the multi-vector sweeps (8; PIPS_HIP_MULTI as for pips_hip_ldl_solve and the dense root): exactly the
 *     sequence of pips_hip_kkt_solve_compressed calls, column by column - way, checks, counters, graph replay.
 *   From the threshold on: the refined way 0 on panels - the leaves' interleaved sweeps (panels of 32 on the matrix pipe, adaptive
 *     refinement per column), the two border products with the border read once per chunk, the root's panel solve - in chunks of at
 *     most 256 columns, fewer where the leaf panel n_total x chunk would exceed 2 GiB, never fewer than 32.  Several ranks: one
 *     all-reduce of S x chunk doubles per chunk; every rank must pass the same nrhs.  This path takes no augmented sweep, captures no
 *     graph, and leaves what pips_hip_kkt_last_solve_path, _last_ltsolve_from_factor and _solve_check_counts report - and which way the
 *     next pips_hip_kkt_solve_compressed goes - as they were.  Only those: the leaf batch's own reports of its last solve
 *     (pips_hip_batch_last_refinement_steps / _measure, the multi-vector path in pips_hip_batch_info) are the panel call's afterwards.
 *     In deterministic mode the leaves solve in panels only where the slots of a panel fit (a leaf handle, a small batch), else one
 *     right-hand side at a time as pips_hip_ldl_solve does there; the border products and the root run on panels either way.
 * PIPS_ERR_ARG: nrhs < 0 and, with nrhs > 0, a NULL pointer, ld0 < S + mz0, ldl < n_total.  PIPS_ERR_STATE: before the first pips_hip_kkt_factorize. */
int pips_hip_kkt_solve_compressed_multi(void* handle, int nrhs, double* B0_dev, long long ld0, double* Bleaf_dev, long long ldl);
/* How the last pips_hip_kkt_solve_compressed_multi went: what[0] 0 = column by column through the single path, 1 = panels; what[1] its
 * chunks (column by column: one per column); what[2] the right-hand sides of a full chunk (of the first one); what[3] / what[4] the
 * refinement steps of the last chunk's Lsolve / Ltsolve leaf solves (panels); what[5] panel chunks solved since the handle was created.
 * Entries beyond these are 0. */
int pips_hip_kkt_solve_multi_info(void* handle, int64_t* what, int n_what);
int pips_hip_kkt_get_schur(void* handle, double** SC_dev, int* ld);
int pips_hip_kkt_root_inertia(void* handle, int* pos, int* neg, int* zero);
/* dense root: 0 static pivot order (default: the Schur complement the leaves build is quasi-definite in the order x0, duals),
 * 1 Bunch-Kaufman inside the diagonal tiles (default once pips_hip_kkt_set_root_inequalities folds -C0^T Omega^-1 C0 into the x0 block) */
int pips_hip_kkt_set_root_pivoting(void* handle, int mode);
/* phase times (ms, HIP events on the streams the work runs on) of the last pips_hip_kkt_factorize and of the solveCompressed calls
 * since; on while the batch's timing switch is on:  ms[0]=diagonals + zero SC  ms[1]=leaf factorisation  ms[2]=Schur reduction
 * ms[3]=finalize  ms[4]=root factorisation  ms[5]=Lsolve leaf solves  ms[6]=Lsolve border product + b0 reduction  ms[7]=Dsolve
 * ms[8]=Ltsolve  ms[9]=x_i = z_i - u_i  ms[10]=panel-wise Schur reduction on its own stream, summed over the panels (ms[2] is
 * then what the main stream waited for it: the exposed part).  What bench.py's phase table is made of. */
int pips_hip_kkt_get_timing(void* handle, double* ms, int64_t* cnt, int n);
/* solveCompressed as a captured and replayed HIP graph : the launch sequence of a call is fixed between
 * factorisations, so it is captured once per (b0, b_leaf pointers, Ltsolve path) and replayed - what pays on launch-bound problems and
 * inside the outer BiCGStab, whose preconditioner this call is (LinearSystem.C:550-798).  Only with a fixed number of refinement steps
 * (pips_hip_batch_set_refinement with tol = 0: the adaptive variant reads norms on the host between steps), one rank, the dense root;
 * otherwise the call is issued launch by launch as before.  stats: captures made / replays so far. */
/* The dense root is factorised on a stream of its own so that the leaf solves of the next solveCompressed run beside it (default on;
 * PIPS_HIP_ROOT_SYNC=1 switches it off for the process).  own_stream = 0: on the main stream - for callers that ask for the root's
 * inertia right after every factorisation (the order of LinearSystem::factorize_with_correct_inertia), where nothing can overlap. */
int pips_hip_kkt_set_root_stream(void* handle, int own_stream);
int pips_hip_kkt_set_solve_graph(void* handle, int on);
int pips_hip_kkt_solve_graph_stats(void* handle, int64_t* captures, int64_t* replays);
/* 1 if the last pips_hip_kkt_solve_compressed took its Ltsolve from the augmented factor (one unrefined backward sweep: only while no
 * pivot is perturbed and the refined leaf solve of the same call needed no refinement step), 0 if by border product + refined solve */
int pips_hip_kkt_last_ltsolve_from_factor(void* handle, int* flag);
/* Which way the last pips_hip_kkt_solve_compressed went (Lsolve / Ltsolve of sLinsysRootAug.C:323-365 with addLniziLinkCons and
 * LniTransMult, DistributedLeafLinearSystem.C:171-212, DistributedLinearSystem.C:430-483):
 *   0  two leaf solves with adaptive refinement (K_i^-1 b_i, then K_i^-1 Br_i x0) and the two sparse border products;
 *   1  refined Lsolve, Ltsolve by one backward sweep of the augmented factor;
 *   2  one forward and one backward sweep of the augmented factor [L 0; L_b I]: the forward sweep leaves -Br_i^T K_i^-1 b_i in the
 *      border rows, the backward sweep started from D^-1 y with the border rows at x0 gives K_i^-1 (b_i - Br_i x0);
 *   3  the sweeps of 2 with their result checked: r_i = (b_i - Br_i x0) - K_i x_i within the refinement tolerance, else the result is
 *      discarded and the call is repeated the refined way (one rank only).
 * 1 and 2 carry no refinement; they are taken only while no pivot of the factorisation is perturbed, and 2 only after a witness on
 * the same factors: a solveCompressed that went way 3, or way 0 / 1 with its refined solves meeting the backward-error tolerance
 * without a step (the first solveCompressed after every factorisation; needs adaptive refinement, pips_hip_batch_set_refinement*). */
int pips_hip_kkt_last_solve_path(void* handle, int* path);
/* How often a solveCompressed that goes by sweeps (way 2) is measured against the leaf rows like the witness (way 3): every `every`-th
 * one; 1 (the default) = every solve is measured, as the reference's PARDISO measures and refines every leaf solve (iparm[7] = 2,
 * PardisoProjectSolver.C:72); 0 = only the first after a factorisation.  A solve whose measure exceeds the refinement tolerance is
 * repeated the refined way from the saved right-hand side and the sweeps stay off for these factors; with several ranks the ranks decide
 * together (one number all-reduced per solveCompressed).  _counts: measured solves and failed measures so far. */
int pips_hip_kkt_set_solve_check(void* handle, int every);
int pips_hip_kkt_solve_check_counts(void* handle, long long* checked, long long* failed);
void pips_hip_kkt_destroy(void* handle);

/* plain device buffers for hosts that do not bring their own allocator */
int pips_hip_malloc(void** dev_ptr, size_t bytes);
int pips_hip_free(void* dev_ptr);
int pips_hip_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
int pips_hip_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
int pips_hip_memset(void* dst_dev, int value, size_t bytes);

/* ---------------------------------------------------------------------------------------------------------------
 * 4. Reduction of the Schur complement and of b0 across the GPUs of a node (replaces MPI_Allreduce in
 *    DistributedRootLinearSystem::reduceKKTdense :860-881 / submatrixAllReduce* :1614-1707 and
 *    PIPS_MPIsumArrayInPlace in sLinsysRootAug::Lsolve :340-341).  RCCL over xGMI.
 * ------------------------------------------------------------------------------------------------------------- */
int pips_hip_comm_unique_id(void* id128);                 /* 128-byte ncclUniqueId, produced on rank 0 */
int pips_hip_comm_create(void** comm, const void* id128, int n_ranks, int rank, int device);
int pips_hip_allreduce_sum(void* comm, double* buf_dev, size_t n, void* stream);
void pips_hip_comm_destroy(void* comm);
/* Communicator backed by the host's own collective (what an MPI build of the reference would pass: a GPU-aware
 * MPI_Allreduce(MPI_IN_PLACE, buf_dev, n, MPI_DOUBLE, MPI_SUM, comm) as in PIPS_MPIsumArrayInPlace, pipsdef.h).  The
 * callback must return 0 after buf_dev (device memory, n doubles) holds the sum over all ranks and is safe to read
 * from any stream; the library synchronises its own stream before calling it. */
typedef int (*pips_hip_allreduce_cb)(void* user, double* buf_dev, size_t n);
int pips_hip_comm_create_external(void** comm, pips_hip_allreduce_cb allreduce, void* user);
/* The same sum as reduce-scatter + all-gather (ncclReduceScatter + ncclAllGather; the slice a rank owns after the first phase is
 * what a distributed root would keep): buf_dev must have room for ceil(n / n_ranks) * n_ranks doubles.  Host-supplied pair for an
 * external communicator (MPI_Reduce_scatter_block / MPI_Allgather, in place on buf_dev: reduce_scatter leaves the sum of slice
 * `rank` at buf_dev + rank * chunk, all_gather replicates every slice); without it the external all-reduce is used.
 * PIPS_HIP_SC_REDUCE=rsag makes pips_hip_kkt_factorize reduce the Schur complement this way. */
typedef int (*pips_hip_reduce_scatter_cb)(void* user, double* buf_dev, size_t chunk);
typedef int (*pips_hip_all_gather_cb)(void* user, double* buf_dev, size_t chunk);
int pips_hip_comm_set_external_rsag(void* comm, int n_ranks, int rank, pips_hip_reduce_scatter_cb reduce_scatter, pips_hip_all_gather_cb all_gather);
/* in-place all-gather of n_parts (= number of ranks) equal parts (rank r's part at buf_dev + r * chunk on entry); without an all-gather in
 * the communicator: the all-reduce, for which the other ranks' parts must be zero on entry */
int pips_hip_all_gather(void* comm, double* buf_dev, size_t chunk, int n_parts, void* stream);
/* Broadcast of n device doubles from rank `root` (the panel of the distributed root factorisation, pips_hip_dense_ldl_set_distributed;
 * the reference has every rank factorise the same matrix instead, DistributedRootLinearSystem.C:1436-1464).  The library's RCCL
 * communicator uses ncclBroadcast; a host-supplied communicator its broadcast callback (MPI_Bcast on device pointers) when one was
 * registered, else an all-reduce in which the other ranks contribute zeros - exact, twice the bytes on the wire; the caller clears the
 * buffer on those ranks first (pips_hip_comm_has_broadcast tells which way it goes). */
typedef int (*pips_hip_broadcast_cb)(void* user, double* buf_dev, size_t n, int root);
int pips_hip_comm_set_external_broadcast(void* comm, int n_ranks, int rank, pips_hip_broadcast_cb broadcast);
int pips_hip_broadcast(void* comm, double* buf_dev, size_t n, int root, void* stream);
int pips_hip_comm_has_broadcast(void* comm);
int pips_hip_allreduce_sum_rsag(void* comm, double* buf_dev, size_t n, void* stream);
int pips_hip_comm_size(void* comm);

/* ---------------------------------------------------------------------------------------------------------------
 * 4b. Flat-arena vector kernels: DistributedVector<T>/DenseVector<T> operations used around the path
 *     (DistributedVector.C:406-460,1160-1340; DenseVector.cpp:281-516).  n = arena length; skip_root = number of leading
 *     (replicated root) entries a non-special rank must not count in sums (iAmSpecial, DistributedVector.C:1293-1303).
 *     Reductions return one host scalar (the caller all-reduces it across ranks where the reference does).
 * ------------------------------------------------------------------------------------------------------------- */
int pips_hip_vec_axpy(long long n, double a, const double* x_dev, double* y_dev, void* stream);           /* add            */
int pips_hip_vec_axpby(long long n, double a, const double* x_dev, double b, double* y_dev, void* stream);
int pips_hip_vec_scale(long long n, double a, double* y_dev, void* stream);                               /* scale / negate */
int pips_hip_vec_copy(long long n, const double* x_dev, double* y_dev, void* stream);                     /* copyFrom       */
int pips_hip_vec_set(long long n, double a, double* y_dev, void* stream);                                 /* setToConstant  */
int pips_hip_vec_add_const(long long n, double a, double* y_dev, void* stream);                           /* add_constant   */
int pips_hip_vec_mul(long long n, const double* x_dev, double* y_dev, void* stream);                      /* componentMult  */
int pips_hip_vec_div(long long n, const double* x_dev, double* y_dev, void* stream);                      /* componentDiv   */
int pips_hip_vec_add_product(long long n, double a, const double* x_dev, const double* z_dev, double* y_dev, void* stream);
int pips_hip_vec_add_quotient(long long n, double a, const double* x_dev, const double* z_dev, const double* mask_dev,
                              double* y_dev, void* stream);
int pips_hip_vec_divide_some(long long n, const double* x_dev, const double* mask_dev, double* y_dev, void* stream);
int pips_hip_vec_select_nonzeros(long long n, const double* mask_dev, double* y_dev, void* stream);
int pips_hip_vec_safe_invert(long long n, double* y_dev, void* stream);
/* y_i = rmin - y_i if y_i < rmin, rmax - y_i if y_i > rmax, else 0; then y_i = max(y_i, -rmax)   (Vector::gondzioProjection,
 * DenseVector.cpp:405-420, used by Residuals::project_r3, Residuals.cpp:262-290) */
int pips_hip_vec_gondzio_projection(long long n, double rmin, double rmax, double* y_dev, void* stream);
int pips_hip_vec_dot(long long n, long long skip_root, const double* x_dev, const double* y_dev, double* result, void* stream);
int pips_hip_vec_one_norm(long long n, long long skip_root, const double* x_dev, double* result, void* stream);
int pips_hip_vec_inf_norm(long long n, const double* x_dev, double* result, void* stream);
int pips_hip_vec_min(long long n, const double* x_dev, double* result, void* stream);
/* two_norm = s*sqrt(sum (x/s)^2) with s = inf_norm (DistributedVector.C:424-437): returns sum (x*scale_inv)^2 */
int pips_hip_vec_sumsq_scaled(long long n, long long skip_root, double scale_inv, const double* x_dev, double* result, void* stream);
/* min over {dx_i < 0, mask_i != 0} of -x_i/dx_i (fraction_to_boundary / stepbound, Variables.C:191-225) */
int pips_hip_vec_stepbound(long long n, const double* x_dev, const double* dx_dev, const double* mask_dev, double* result, void* stream);
/* Variables::find_blocking (Variables.C:227-308) for one pair of complementary vectors: out5 = [min ratio -x_i/dx_i over
 * dx_i < 0 (inf if no entry blocks), then x, dx, y, dy at the blocking index (smallest index on ties)] */
/* the step bounds of nw <= 16 blended directions in one pass: out[k] = largest alpha with x + alpha (dx + w_k cx) >= 0 (inf if
 * unbounded), out[nw + k] the same for (y, dy, cy), w_k = min(1, wmin + (1 - wmin) k / (nw - 1)) - the corrector weight search
 * calculate_alpha_pd_weight_candidate (InteriorPointMethod.cpp:486-523); out2nw is a host array */
int pips_hip_vec_weighted_stepbounds(long long n, const double* x_dev, const double* dx_dev, const double* cx_dev, const double* y_dev,
                                     const double* dy_dev, const double* cy_dev, double wmin, int nw, double* out2nw, void* stream);
int pips_hip_vec_find_blocking(long long n, const double* x_dev, const double* dx_dev, const double* y_dev, const double* dy_dev,
                               double* out5, void* stream);
/* sum (x + a dx)(y + b dy)  (mustep_pd, Variables.C:109) */
int pips_hip_vec_dot_shifted(long long n, long long skip_root, const double* x_dev, double a, const double* dx_dev,
                             const double* y_dev, double b, const double* dy_dev, double* result, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * 4c. Host harness: Mehrotra predictor-corrector IPM with Gondzio correctors for the reference's full problem class
 *        min c^T x [+ 1/2 x^T Q x]   s.t.  A x = b,  clow <= C x <= cupp,  xlow <= x <= xupp      (every bound optional per row / entry)
 *     with block-angular A and C (and a convex Hessian, block-diagonal through pips_ipm_create_qp or bordered through pips_ipm_create_qp_cross), driving the fused KKT path (counterpart of PIPSIPMppSolver::solve / InteriorPointMethod /
 *     LinearSystem::computeDiagonals, solve, solveXYZS, solveCompressedBiCGStab, system_mult / Residuals::evaluate /
 *     DistributedMatrix::mult).  One or several ranks.
 *     Input = the reader's per-block layout (GMSPIPSBlockData_t, Drivers/gams/gmspips/gmspipsio.h:5-58): block 0 is the root
 *     (n0 variables; A = A0, C = C0, BL = F0, DL = G0; B, D absent), block k >= 1 has n variables, A (my x n0) and B (my x n)
 *     for its equality rows, C (mz x n0) and D (mz x n) for its inequality rows, BL (myl x n) / DL (mzl x n) its part of the
 *     linking rows.  Row pointers are block-local and start at 0.  Indicators are 0.0 / 1.0.
 *     Vector orders: x = [x0 | x_1 .. x_N]; equality rows / y = [root rows | linking rows | block 1 .. N];
 *     inequality rows / s, z, t, u, lambda, pi = [root rows | linking rows | block 1 .. N].
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
   int rows, cols;
   const int* rowptr;      /* NULL: matrix absent (all zero) */
   const int* colidx;
   const double* val;
} pips_csr_view;
typedef struct {
   int n, my, mz;                                        /* variables, own equality rows, own inequality rows */
   pips_csr_view A, B, C, D, BL, DL;
   const double *c, *xlow, *xupp, *ixlow, *ixupp;        /* n entries each */
   const double* b;                                      /* my */
   const double *clow, *cupp, *iclow, *icupp;            /* mz */
} pips_ipm_block;
/* n_blocks counts the root (block 0).  bL: right-hand side of the myl linking equalities; dlow / dupp / idlow / idupp: bounds
 * of the mzl linking inequalities.  Several ranks: blocks[1..] are this rank's blocks, the root block and
 * the linking data are identical on every rank; comm as for pips_hip_kkt_create.  Scalars are reduced over the ranks
 * (replicated parts counted on rank 0 only, DistributedVector.C:1293-1303), replicated rows of the SpMVs are summed
 * (DistributedMatrix.C:224-326); every rank returns the same result and holds the root part and its blocks' part of the
 * solution. */
int pips_ipm_create_general(void** handle, int n_blocks, const pips_ipm_block* blocks, int myl, int mzl, const double* bL,
                            const double* dlow, const double* dupp, const double* idlow, const double* idupp, double dual_reg,
                            int device, void* comm, int rank, int n_ranks);
/* the generator's class  min c^T x, A x = b, x >= 0   as a shorthand for the general entry: W/T/F rowptr
 * arrays hold N block-local row pointers back to back; x order [x_0 | x_1 .. x_N], b/y order [linking rows | block rows] */
int pips_ipm_create(void** handle, int N, int n0, int myl, const int* n_i, const int* my_i, const int* W_rowptr,
                    const int* W_colidx, const double* W_val, const int* T_rowptr, const int* T_colidx, const double* T_val,
                    const int* F_rowptr, const int* F_colidx, const double* F_val, const int* F0_rowptr, const int* F0_colidx,
                    const double* F0_val, const double* c, const double* b, double dual_reg, int device);
int pips_ipm_create_rank(void** handle, int N, int n0, int myl, const int* n_i, const int* my_i, const int* W_rowptr,
                         const int* W_colidx, const double* W_val, const int* T_rowptr, const int* T_colidx, const double* T_val,
                         const int* F_rowptr, const int* F_colidx, const double* F_val, const int* F0_rowptr, const int* F0_colidx,
                         const double* F0_val, const double* c, const double* b, double dual_reg, int device, void* comm, int rank,
                         int n_ranks);
/* result7: [0] primal objective [1] iterations [2] mu [3] residual inf-norm [4] status (0 converged, 1 max iterations, 2 numerical
 * breakdown before any usable iterate, 3 numerical troubles: the best iterate so far is returned - its mu / residual are in
 * [2] / [3], 4 probably infeasible: phi = (||r|| + |gap|) / dnorm is >= 1e-8 and 1e4 times its best value after ten iterations,
 * PIPSIPMppSolver.cpp:128-170) [5] dual objective b^T y + clow^T lambda - cupp^T pi + xlow^T gamma - xupp^T phi [6] data norm.
 * Termination as PIPSIPMppSolver.cpp:143-149: mu <= mutol and ||r||inf <= artol * dnorm. */
int pips_ipm_solve(void* handle, int max_iter, double mutol, double artol, int verbose, double* result7);
/* Gondzio multiple centrality correctors per iteration (InteriorPointMethod.cpp:236-358): 0 = plain Mehrotra predictor-
 * corrector; default 2, i.e. 4 solves per iteration like the work unit of bench.py */
int pips_ipm_set_gondzio(void* handle, int max_correctors);
/* harness settings under the reference's option identifiers (Options.C:18-73, PIPSIPMppOptions.C:170-264,303-310):
 * GONDZIO_MAX_CORRECTORS, OUTER_SOLVE (1 iterative refinement, 2 BiCGStab), OUTER_BICG_MAX_ITER,
 * OUTER_BICG_MAX_NORMR_DIVERGENCES, OUTER_BICG_MAX_STAGNATIONS, REGULARIZATION (0/1: the inertia-correcting loop); anything else
 * returns an error */
int pips_ipm_set_option(void* handle, const char* name, double value);
/* shorthand for the x >= 0 class: bounded_mask (nx host doubles) is 1 for x_j >= 0 and 0 for a free x_j (ixlow = ixupp = 0, whose
 * computeDiagonals leaves dd_j = 0: LinearSystem.C:262-294).  Free entries carry no complementarity pair; the preconditioner gets
 * a proximal term on their diagonal (1e-6, option FREE_VARIABLE_PROXIMAL_TERM), the outer solve none.  Call before
 * pips_ipm_solve; with several ranks on every rank.  (The general entry takes free variables through ixlow = ixupp = 0.) */
int pips_ipm_set_free_variables(void* handle, const double* bounded_mask_host);
int pips_ipm_get_solution(void* handle, double* x_host, double* y_host);
/* dims4 = {nx, my, mz, complementarity pairs over all ranks}; iterate: any pointer may be NULL (sizes nx: x v w gamma phi,
 * my: y, mz: s z t u lambda pi) */
int pips_ipm_get_dims(void* handle, long long* dims4);
int pips_ipm_get_iterate(void* handle, double* x, double* s, double* y, double* z, double* t, double* u, double* v, double* w,
                         double* lambda, double* pi, double* gamma, double* phi);
/* history of the last pips_ipm_solve, one row of 7 doubles per iterate: mu, ||r||inf, primal objective, dual objective, and the
 * step taken from it: sigma, alpha_primal, alpha_dual (zeros in the final row).  rows7 may be NULL to query *n_rows. */
int pips_ipm_get_trace(void* handle, double* rows7, int max_rows, int* n_rows);
/* counters of the last pips_ipm_solve: [0] KKT factorisations, [1] of which repeats with added regularisation (the inertia
 * loop, LinearSystem.C:295-325), [2] solveCompressed calls (preconditioner applications), [3] Gondzio correctors accepted;
 * stats2: [0] BiCGStab iterations, [1] host synchronisations (scalar read-backs) */
int pips_ipm_get_stats(void* handle, long long* stats4);
int pips_ipm_get_stats2(void* handle, long long* stats2);
/* how the leaves form their Schur contribution, as analyzed (pips_hip_batch_get_schur_mode: 1 augmented factorisation, 2 blocked solves).
 * pips_ipm_create reads PIPS_IPM_SCHUR_MODE (0 auto, 1, 2; unset: the batch's default) before it analyzes */
int pips_ipm_get_schur_mode(void* handle, int* mode);
/* direct entries to the rows either side of the path, for parity tests.  pips_ipm_mult: out = J in (transposed = 0; in: nx, out:
 * my + mz = [A x | C x]) or out = J^T in (transposed = 1) - DistributedMatrix::mult / transpose_mult; with several ranks the
 * replicated rows are summed.  pips_ipm_outer_solve: factorises with the diagonals of the pair vectors G = [t|u|v|w],
 * L = [lambda|pi|gamma|phi] (host, 2 mz + 2 nx entries each) and runs the outer solve (OUTER_SOLVE option) on
 * [dd J^T; J diag(0, nOmegaInv)] sol = rhs ([x | y | z] order) to tolerance tol * ||rhs||; info6 = {status (1 converged, 2 skipped,
 * 3 max iterations, 4 breakdown, 5 diverged, 6 stagnation), iterations, ||r||_2, ||rhs||_2, preconditioner applications, host
 * synchronisations} */
int pips_ipm_mult(void* handle, int transposed, const double* in_host, double* out_host);
/* The harness kernels beside a handle, for parity tests as well (tests/harness_cases.py): host arrays in, the launch code the handle
 * runs (the launch_* functions of csrc/harness.hip: kernel choice, grid sizes, the long-row pair), host arrays out.  Synchronous, on the
 * current device.  PIPS_ERR_ARG with a message for arguments a kernel would read out of bounds with, then PIPS_ERR_NO_DEVICE without a
 * GPU; every device buffer is freed before the call returns.
 * pips_ipm_probe_spmv: out = epilogue(M in) for the CSR matrix M (nrows x ncols) and mode 0 rQ = e0 [+ e3] - s - e1 + e2, 1 [rA|rC] =
 *   s - (r < split ? e0[r] : e1[r - split]), 2 e0 e1 [+ e3] + s, 3 s + e0 e1, 4 e2 - (e0 e1 [+ e3] + s), 5 e2 - (s + e0 e1), 6 s (s the row's
 *   sum; e0..e2 nrows long - mode 1: e0 split, e1 nrows - split entries - and there where the mode reads them; e3 NULL or nrows long, modes
 *   0, 2, 4).  lin, r0e, r1b, r1e: on the rows [0, r0e) and [r1b, r1e) a rank with lin != 0 produces +-s alone, and e3 +- s with lin = 2
 *   (which needs e3).  pred: -1 none, else 0 / 1 stored on the device for the kernels to test.  out: in-out, out_len >= nrows entries,
 *   all of them uploaded and read back - what no kernel writes keeps the caller's content.  *lanes: the lanes per row chosen (4 or 8; 0
 *   without rows), *n_long and long_rows (nrows ints, or NULL): the rows handed to the long-row kernels, from the builder of the layout's lists.
 * pips_ipm_probe_reduce: out[k] = term k, 1 <= n_terms <= 12, in ONE launch.  kind 0 sum [w] a b, 1 max |a| (|a w| with w, else |a / d|
 *   with d), 2 min a over c != 0, 3 min -a / b over b < 0, 4 sum [w] (a + p c)(b + q d); operands n long, the unread ones NULL.  out in-out
 *   (pred = 0 leaves it).
 * pips_ipm_probe_step: ONE entry for the nine element-wise kernels (one argument convention instead of nine prototypes; the kernel's own
 *   argument list, in its order, is `in` followed by `out`).  in[k] has in_len[k], out[k] (in-out) out_len[k] entries, at least what the
 *   kernel touches with ncp = 2 mz + 2 nx, nyz = my + mz; longer arrays travel whole (guard entries).  scalars: 5 doubles.
 *     kernel              in                                                        out                        flag      scalars
 *     0 bound_residuals   x(nx) s(mz) z(mz) G L M Bd (ncp)                          rz(mz) rG(ncp)
 *     1 diagonals         G L M (ncp)                                               dd(nx) ddp(nx) dyz(nyz)              free_reg
 *     2 leaf_diag         ddp(nx) nOmegaInv(mz) qdiag(nx or NULL); idx: n codes     leaf_diag(n)                         primal_reg dual_reg reg
 *     3 reg_operator      ddp(nx) dyz(nyz)                                          dop_r(nx) dyz_r(nyz)                 reg dual_reg
 *     4 rhs_reduce        rQ(nx) rAC(nyz) rz(mz) rG rL G L M (ncp) dyz(nyz)         rhs(nx + nyz) rs(mz)       zero_lin
 *     5 recover           sol(nx + nyz) rs(mz) rG rL G L M (ncp) dyz(nyz)           sP(nx + mz + ncp) sD(nyz + ncp)  zero_lin
 *     6 compl_rhs         G L dG dL M (n)                                           r(n)                       mode      alpha ap ad rmin rmax
 *     7 masked_const      M(n)                                                      y(n)                       add       a
 *     8 gather            in; idx: n indices                                        out                        scatter
 *   gather: out[i] = in[idx[i]] (flag 0) or out[idx[i]] = in[i] (flag 1); the indexed array's length bounds the indices. */
typedef struct {
   int kind;
   long long n;
   const double *a, *b, *c, *d, *w;
   double p, q;
} pips_ipm_red_term;
enum {
   PIPS_STEP_BOUND_RESIDUALS = 0, PIPS_STEP_DIAGONALS, PIPS_STEP_LEAF_DIAG, PIPS_STEP_REG_OPERATOR, PIPS_STEP_RHS_REDUCE,
   PIPS_STEP_RECOVER, PIPS_STEP_COMPL_RHS, PIPS_STEP_MASKED_CONST, PIPS_STEP_GATHER
};
int pips_ipm_probe_spmv(int mode, int nrows, int ncols, const int* rowptr, const int* colidx, const double* val, const double* in,
                        const double* e0, const double* e1, const double* e2, const double* e3, int split, int lin, int r0e, int r1b, int r1e,
                        int pred, double* out, long long out_len, int* lanes, int* n_long, int* long_rows);
int pips_ipm_probe_reduce(int n_terms, const pips_ipm_red_term* terms, int pred, double* out);
int pips_ipm_probe_step(int kernel, int nx, int my, int mz, long long n, int flag, const double* scalars, int n_in, const double* const* in,
                        const long long* in_len, const long long* idx, long long idx_len, int n_out, double* const* out, const long long* out_len);
/* Problem scaling (the reference's Scaler stage, ScalerType in Core/Preprocessing/PreprocessType.h; same order).  Curtis-Reid is
 * reserved and not supported. */
enum {
   PIPS_SCALER_NONE = 0,
   PIPS_SCALER_EQUILIBRIUM = 1,             /* EquilibriumScaler: one pass, max |entry| of every row and column becomes 1 */
   PIPS_SCALER_GEOMETRIC_MEAN = 2,          /* GeometricMeanScaler: up to 10 passes of 1 / sqrt(min max), kept if it gains 15 % */
   PIPS_SCALER_GEOMETRIC_MEAN_EQUILIBRIUM = 3,   /* the same followed by an equilibrium pass */
   PIPS_SCALER_CURTIS_REID = 4,             /* reserved: PIPS_ERR_ARG */
   PIPS_SCALER_RUIZ = 5                     /* not in the reference: Ruiz equilibration of [Q J^T; J 0] by diag(col, row), ten simultaneous
                                               passes of d <- d / sqrt(max |row of D K D|) with no early stop; the only scaler that sees a
                                               Hessian.  Without one: Ruiz on [0 J^T; J 0] */
};
/* pips_ipm_create_general with a scaler, chosen at creation (the leaf borders are fixed by the analysis).  J = [A; C] becomes
 * R J Cs with R = diag(row_eq, row_ineq) and Cs = diag(col); c, b, the row and variable bounds and the linking right-hand sides
 * follow (Scaler::applyScaling: c Cs, R b, R clow, R cupp, xlow / col, xupp / col); the objective is not scaled separately.
 * The extrema sweeps run on the device.  pips_ipm_solve terminates on the UNSCALED residual (Scaler::unscale_residuals) against
 * the data norm of the original problem, which result7[3] / [6] and the trace report; the start point uses the data norm of the
 * scaled problem.  pips_ipm_get_solution / pips_ipm_get_iterate return the original problem's variables
 * (Scaler::unscale_variables).  pips_ipm_mult and pips_ipm_outer_solve act on the system as the harness holds it: the scaled
 * one.  PIPS_SCALER_NONE gives exactly pips_ipm_create_general. */
int pips_ipm_create_general_scaled(void** handle, int n_blocks, const pips_ipm_block* blocks, int myl, int mzl, const double* bL,
                                   const double* dlow, const double* dupp, const double* idlow, const double* idupp, double dual_reg,
                                   int device, void* comm, int rank, int n_ranks, int scaler);
/* the factors in the harness order: col (nx) for x = [x0 | own blocks], row_eq (my) and row_ineq (mz) for [root | linking | own
 * blocks]; any pointer may be NULL.  info8 = {scaling applied (0/1), row ratio before, column ratio before, row ratio after,
 * column ratio after, geometric passes made, geometric stage kept (0/1), host waits of the scaler}.  A handle without scaling
 * returns factors of 1 and zeros in info8.  PIPS_SCALER_RUIZ reports {1, J's ratios before and after (J's on a QP too), 10 (its
 * passes), 0, 2 (the read before and the read after)}. */
int pips_ipm_get_scaling(void* handle, double* col, double* row_eq, double* row_ineq, double* info8);
int pips_ipm_outer_solve(void* handle, const double* G_host, const double* L_host, const double* rhs_host, double tol, double* sol_host,
                         double* info6);
/* Convex QPs: the reference's full problem class  min c^T x + 1/2 x^T Q x  over the same constraints, Q block-diagonal over the root
 * and the blocks (the class PIPS-IPM++ inherits from OOQP).
 * pips_ipm_create_general with Hessians: Q[i] belongs to blocks[i] (i = 0 the root), n_i x n_i, LOWER-triangular CSR as the reference's
 * SparseSymmetricMatrix (isLower); Q == NULL or Q[i].rowptr == NULL: no Hessian for that block.  Several ranks: Q[0] identical on every rank.
 * PIPS_ERR_ARG with a message for an entry above the diagonal, a column index out of range, Q[i].rows or Q[i].cols != n_i, and a
 * negative diagonal entry.  The last is a cheap necessary test only: no test of positive semidefiniteness is made, CONVEXITY IS THE
 * CALLER'S CONTRACT (an indefinite Q gives a KKT matrix of the wrong inertia, which the regularisation loop answers as it can).
 * With Q == NULL (or no Q[i] present) the handle is the one pips_ipm_create_general builds and takes the LP path unchanged.
 * With a Hessian: Q_i enters the leaf matrices and Q0 the x0 block of the Schur complement; rQ = c + Q x - A^T y - C^T z - gamma + phi;
 * the operator of the outer solve (pips_ipm_outer_solve too) is [dd + Q  J^T; J diag(0, nOmegaInv)]; the data norm includes max |Q|;
 * the primal and the dual part of the iterate take ONE step length min(alpha_p, alpha_d) (the trace reports both columns, equal).
 * result7[0] and trace column 2 hold c^T x + 1/2 x^T Q x; result7[5] and trace column 3 hold the Lagrangian dual
 * b^T y + clow^T lambda - cupp^T pi + xlow^T gamma - xupp^T phi - 1/2 x^T Q x, so that their difference is the reference's duality gap
 * (Residuals.cpp:69-165) - the reference's own dual_objective field omits the quadratic term.
 * The cross Hessian between x0 and x_i: pips_ipm_create_qp_cross below.  Not offered: Hessians through the pips_ipm_create shorthand. */
int pips_ipm_create_qp(void** handle, int n_blocks, const pips_ipm_block* blocks, const pips_csr_view* Q, int myl, int mzl,
                       const double* bL, const double* dlow, const double* dupp, const double* idlow, const double* idupp,
                       double dual_reg, int device, void* comm, int rank, int n_ranks);
/* pips_ipm_create_qp with a scaler.  With x = Cs x' the Hessian becomes Q' = Cs Q Cs beside J' = R J Cs: the stored entry (r, c) of a
 * block's lower triangle is (q col_r) col_c, scaled on the host; the flat symmetric copy on the device is built from the scaled
 * triangles and stays exactly symmetric.  The objective c'^T x' + 1/2 x'^T Q' x' is the original problem's value; the data norm of
 * the scaled problem (start point) takes max |Q'|, the original one (termination) max |Q|; the unscaled residual keeps its weights
 * (rQ' = Cs rQ).  The equilibrium and geometric-mean scalers take their factors from J alone, as the reference's Scaler does (its
 * applyScaling leaves Q untouched), and Q follows the column factors; PIPS_SCALER_RUIZ equilibrates [Q J^T; J 0] and is the one to use
 * on a badly scaled QP.  pips_ipm_get_scaling, pips_ipm_get_solution, pips_ipm_get_iterate and the trace behave as on a scaled LP
 * handle; pips_ipm_mult, pips_ipm_outer_solve and pips_ipm_hessian_mult act on the scaled system (Q' v).
 * scaler == PIPS_SCALER_NONE is pips_ipm_create_qp, Q == NULL (or no Q[i] present) pips_ipm_create_general_scaled, call for call.
 * PIPS_ERR_ARG for PIPS_SCALER_CURTIS_REID and for any value outside 0-5. */
int pips_ipm_create_qp_scaled(void** handle, int n_blocks, const pips_ipm_block* blocks, const pips_csr_view* Q, int myl, int mzl,
                              const double* bL, const double* dlow, const double* dupp, const double* idlow, const double* idupp,
                              double dual_reg, int device, void* comm, int rank, int n_ranks, int scaler);
/* pips_ipm_create_qp_scaled with the reference's bordered (arrow-shaped) Hessian
 *        [ Q0   R_1^T ... R_N^T ]
 *   Q =  [ R_1  Q_1             ]      R_i : n_i x n0, the "left bordering blocks" of DistributedSymmetricMatrix
 *        [ R_N              Q_N ]
 * R[i] (i >= 1) is block i's cross Hessian with x0: GENERAL CSR, rows == n_i, cols == n0, rows in any order, duplicates added up; R[0]
 * must be absent (rowptr NULL).  Several ranks: R[1..] belong to the rank's own blocks.  R == NULL, every R[i].rowptr == NULL or every
 * R[i] without a stored entry is pips_ipm_create_qp_scaled, call for call.  PIPS_ERR_ARG with a message for R[i].rows != n_i or
 * R[i].cols != n0, a column index out of range, R[0] present, and stored entries with n0 == 0.  Convexity of the WHOLE Q stays the
 * caller's contract; a handle with R but without any Q[i] is a QP handle like any other.
 * Where R enters: R_i is the first block of leaf i's border (the reference's BorderBiBlock {R, A, C, n_empty, F^T, G^T}), so the Schur
 * complement, both root kinds and both Schur modes see it; the flat symmetric Hessian on the device holds (x_i row, x0 column) and its
 * mirror from the one stored value, the x0 rows taking the long-row path once they pass 512 entries; rQ, the operator of the outer
 * solve, pips_ipm_hessian_mult and the objectives carry the cross terms; the data norm takes max |R|; a scaler gives
 * R'_i(r, c) = (v col[x_i row r]) col[x0 column c], the row's factor first; PIPS_SCALER_RUIZ sees R as part of Q.
 * Several ranks: (Q x)_0 = Q0 x0 + sum_i R_i^T x_i is a sum over all ranks' blocks.  Rank 0 contributes Q0 x0 and its own blocks' terms,
 * every other rank its own blocks' terms (its flat Q holds no Q0 block); the contributions ride in the replicated x0 rows of the J^T
 * product and are summed with them - no further collective.  x^T Q x is the plain sum over the ranks of x . (Q x)_partial.  Whether any
 * rank holds a cross Hessian is agreed at creation together with whether any holds a Hessian. */
int pips_ipm_create_qp_cross(void** handle, int n_blocks, const pips_ipm_block* blocks, const pips_csr_view* Q, const pips_csr_view* R,
                             int myl, int mzl, const double* bL, const double* dlow, const double* dupp, const double* idlow,
                             const double* idupp, double dual_reg, int device, void* comm, int rank, int n_ranks, int scaler);
/* out = Q in over x = [x0 | own blocks] (Problem::hessian_multiplication; parity tests), cross terms included; several ranks with a cross
 * Hessian: the x0 part is the full sum on every rank (one collective).  Zeros on a handle without Hessian. */
int pips_ipm_hessian_mult(void* handle, const double* in_host, double* out_host);
void pips_ipm_destroy(void* handle);

/* ---------------------------------------------------------------------------------------------------------------
 * 5. Host harness helpers (no GPU needed): synthetic arrowhead LP of SURVEY.md §8d, leaf KKT / border assembly.
 * ------------------------------------------------------------------------------------------------------------- */
int pips_gen_row_nnz(int n_i, double rho);
int pips_gen_block(uint64_t seed, int block, int n_i, int my_i, int n0, int myl, double rho, int* W_rowptr,
                   int* W_colidx, double* W_val, int* T_rowptr, int* T_colidx, double* T_val, int* F_rowptr,
                   int* F_colidx, double* F_val, double* c, double* xstar);
int pips_gen_root(uint64_t seed, int n0, int myl, int* F0_rowptr, int* F0_colidx, double* F0_val, double* c0,
                  double* xstar0);
int pips_gen_diagonal(uint64_t seed, int block, int n, double lo, double hi, double* d);
int pips_kkt_leaf_assemble(int nx, int my, int mz, const int* Q_rowptr, const int* Q_colidx, const double* Q_val,
                           const int* B_rowptr, const int* B_colidx, const double* B_val, const int* D_rowptr,
                           const int* D_colidx, const double* D_val, int* K_rowptr, int* K_colidx, double* K_val,
                           int* diag_pos);
int pips_border_assemble(int nx, int my, int mz, int n0, int n_empty, int myl, int mzl, const int* R_rowptr,
                         const int* R_colidx, const double* R_val, const int* A_rowptr, const int* A_colidx,
                         const double* A_val, const int* C_rowptr, const int* C_colidx, const double* C_val,
                         const int* F_rowptr, const int* F_colidx, const double* F_val, const int* G_rowptr,
                         const int* G_colidx, const double* G_val, int* Bt_rowptr, int* Bt_colidx, double* Bt_val);
/* block -> rank map (DistributedTree::assignProcesses, DistributedTree.C:35-90): contiguous, monotone, balanced */
int pips_map_children_to_ranks(int n_children, int n_ranks, int* map);
/* symbolic analysis only (CPU): fills what[] like pips_hip_ldl_info and optionally perm/colcount (may be NULL) */
int pips_symbolic_probe(int n, int n_primal, const int* krow, const int* jcol, int S, const int* Bt_rowptr,
                        const int* Bt_colidx, int force_n_head, int64_t* what, int n_what, int* perm, int* colcount);

/* the same under the order the sparse root takes for chain-like Schur complements: the hubs (x0, root equality rows) last, the rest
 * dissected by level structures, minimum degree in segments below min_size rows (order.cpp hub_dissected_order); PIPS_ERR_STATE when
 * the graph without the hubs has no separators.  CPU only. */
int pips_symbolic_probe_hubs(int n, int n_primal, const int* krow, const int* jcol, int n_hubs, const int* hubs, int min_size,
                             int64_t* what, int n_what, int* perm, int* colcount);

/* The host layout pass of a batch analysis, without a device (csrc/layout.cpp; tests): symbolic analysis of every block with the
 * switches read from the environment as pips_hip_batch_analyze reads them, then the layout the engine would upload.  K per block as
 * lower-triangular CSR (n[b] + 1 row pointers), the border as CSR with S rows over the block's n[b] rows (bt_rowptr or bt_rowptr[b]
 * NULL: no border).  free_device_bytes stands in for the free device memory that decides the single-launch tails.  The properties
 * the kernels rely on are checked (disjoint block regions; supernode order and level ranges; front launches and their LDS; border-split
 * batches; scatter targets, diagonal positions and the two-triangle row structure; the border by leaf row; the simple leaves' gather):
 * PIPS_ERR_STATE with a message that names the first one that fails.
 * what[0] arena doubles, [1] work-vector doubles, [2] U-arena doubles, [3] head supernodes, [4] levels kept for the level launches,
 * [5] levels of the spine, [6] front launches, [7] fronts in the device-memory classes, [8] border-split batches, [9] staging doubles of a
 * batch, [10] single-launch tails, [11] border-backward sweep, [12] sweeps of the augmented factor, [13] / [14] slots of the
 * factorisation / forward substitution (deterministic mode), [15] sum of n, [16] multifrontal head, [17] Schur mode taken,
 * [18] doubles of the border-row arena, [19] doubles of update matrices, [20] supernodes of the spine */
int pips_layout_probe(int nblk, const int* n, const int* n_primal, const int* const* krow, const int* const* kcol,
                      int S, const int* const* bt_rowptr, const int* const* bt_colidx,
                      int deterministic, long long free_device_bytes, int64_t* what, int n_what);

/* The task plans of a leaf batch's launch-per-step tail factorisation, without a device (inputs as pips_layout_probe; force_n_head as
 * pips_hip_batch_set_options, -1: the cost model): the column plan, and the same tasks regrouped by groups of four tile columns.
 * col_tasks: rows of 6 ints in launch order - kind (0 update, 1 trsm), block, ti, tj, k0, k1 (the K range in tile columns; 0, 0 for a trsm).
 * grp_tasks: rows of 9 ints in launch order - list (0 deep update, 1 / 2 the diagonal block's first and second deep step, 3 / 4 its updates
 * and trsm of one column, 5 a strip of the panel launch), group, index (the tile column for 3 / 4, the strip's number inside its launch for 5),
 * position inside the list or strip, block, ti, tj, k0, k1.  At most col_cap / grp_cap rows are written.
 * counts (6 entries): rows of either kind there are, tile columns, groups, launches per factorisation of the column path and of the groups. */
int pips_tail_plan_probe(int nblk, const int* n, const int* n_primal, const int* const* krow, const int* const* kcol,
                         int S, const int* const* bt_rowptr, const int* const* bt_colidx, int force_n_head,
                         int* col_tasks, long long col_cap, int* grp_tasks, long long grp_cap, int64_t* counts);

/* The first-touch plan of the tails, without a device (csrc/layout.cpp layout_first_touch; inputs as pips_layout_probe, force_n_head as
 * pips_tail_plan_probe; lds_bytes > 0 replaces the LDS budget of a column): the layout as the analysis decides it, and the layout with
 * the first touch refused, as 14 sections of integers back to back in out, at most cap of them (cap 0: sizes only):
 *   0 per block, rows of 12: n, n_head, m, m_pad, nb, ldT, mf_split, T_in (arena offset where the tail is assembled), first K value,
 *     border entries, root fronts, tile columns
 *   1 first global column of every block (blocks + 1)        2 / 4 offsets of the columns' init entries / front pieces (columns + 1 each)
 *   3 init entries, rows (row inside the tail panel, source: >= 0 index of the K value, < 0 ~index of the border value)
 *   5 front pieces, rows (front, offset of the first value among the update matrices, offset of the first row index, entries)
 *   6 the simple leaves whose products into the tail and the Schur complement are deferred
 *   7 / 8 scatter targets of the K values without / with the first touch (arena offsets, -1: not scattered)    9 / 10 the same for the border
 *   11 root fronts in k_root_assemble's order, rows (block, front, r, rb, offset of its update matrix, offset of its row indices)
 *   12 the row indices of all supernodes     13 simple leaves, rows (supernode, block, r, update segments, offset of its row indices)
 * Sections 1 - 6 are empty where the path is refused.  counts (22 entries): [0] first touch taken, [1] multifrontal head, [2] single-launch
 * tails, [3] Schur mode taken, [4] doubles of update matrices, [5] K values, [6] border values, [7] integers in all sections,
 * [8 + k] integers of section k. */
int pips_first_touch_probe(int nblk, const int* n, const int* n_primal, const int* const* krow, const int* const* kcol,
                           int S, const int* const* bt_rowptr, const int* const* bt_colidx, int force_n_head, int deterministic,
                           long long lds_bytes, long long free_device_bytes, long long* out, long long cap, int64_t* counts);

/* The host plans of deterministic mode, without a device (csrc/detplan.cpp; tests): the layout of a deterministic analysis (inputs as
 * pips_layout_probe with deterministic set), then the planners the engine runs for this rank of n_ranks that need no recording of the
 * head's scatters, and the Schur SYRK's row panels for n_panels.  out receives 16 sections of integers back to back, at most cap
 * of them (cap 0: sizes only); a gather list is written as its number of targets T, its T targets, T + 1 offsets and its slots:
 *   0 block -> group          1 per block: tile columns, nb, nb_pad, root fronts, border-split batches, entries of bmap
 *   2 rounds of the Schur SYRK, rows (round, block, ti, tj)      3 / 4 rounds of k_root_assemble / k_border_schur_add, rows (round, block)
 *   5 gather list of Br^T z per (group, Schur column)     6 / 7 gather lists of the border products: rows per Schur column, entries per leaf row
 *   8 - 12 forward sweep of the augmented factor: gather list of the border slots per (group, Schur column); entries, rows (offset of the
 *     factors, first column in the work vector, stride, width); per target: entry pointers (targets + 1), entry indices, slot
 *   13 first Schur row of every panel (panels + 1; empty: one panel)    14 the panels' tasks, rows (group, block, ti, tj)    15 bmap, block after block
 * counts (32 entries): [0] groups, [1] first group slot, [2] group slots of this rank, [3] all eight slots are added on every rank,
 * [4] the augmented sweep's lists are built, [5] / [6] sweeps of the augmented factor: the plan's answer / the layout's, [7] multifrontal
 * head, [8] border-split batches, [9] root fronts, [10] Schur mode taken, [11] panel groups, [12] / [13] targets / entries of the augmented
 * sweep, [14] border rows of all head supernodes, [15] integers in all sections, [16 + k] integers of section k. */
int pips_det_plan_probe(int nblk, const int* n, const int* n_primal, const int* const* krow, const int* const* kcol,
                        int S, const int* const* bt_rowptr, const int* const* bt_colidx, int rank, int n_ranks, int n_panels,
                        long long* out, long long cap, int64_t* counts);

/* The host layout pass of an IPM handle's creation, without a device (csrc/ipmlayout.cpp; tests): the functions pips_ipm_create_qp runs
 * before it touches the device.  Inputs as pips_ipm_create_qp without device and comm; eliminate_z0: whether the root inequality rows are
 * eliminated from the root system (what PIPS_IPM_ROOT_INEQ_ELIMINATE / PIPS_IPM_SPARSE_ROOT decide at creation); col (nx) and
 * row ([row_eq | row_ineq], my + mz): both NULL, or scaling factors the data is scaled with first, as pips_ipm_create_general_scaled
 * and pips_ipm_create_qp_scaled scale it with their scaler's (the Hessians too: Q' = Cs Q Cs).
 * dims (PIPS_IPML_DIMS): N n0 my0 mz0 myl mzl ry rzr nx my mz ncp nxyz NP ND nleaf e_mz0 e_mzl S has_q.  scalars: this rank's
 * complementarity pairs and data norm.  Arrays by size-then-fill: with out == NULL sizes[k] receives the entry count of array k; with
 * out given, sizes must hold those counts and out[k] receives array k (out[k] may be NULL where sizes[k] is 0).  The arrays
 * (i: int, l: long long, d: double; pads of "never empty" arrays are not counted):
 *   0-3   xoff yoff zoff (i, N + 2) koff (l, N + 2)
 *   4-11  J rowptr colidx (i) val (d), J^T rowptr colidx (i) val (d), long rows of J, of J^T (i)
 *   12-20 c b M Bd wG wGs wXYZ (d) pack code (l)
 *   21-26 per leaf, back to back: K rowptr colidx (i) constant values (d), border rowptr (S + 1 each) colidx (i) val (d)
 *   27-38 rowptr colidx (i) val (d) of A0, F0, C0 and of G0 (eliminate_z0 == 0: [C0; G0]); an absent matrix has size 0
 *   39-42 per block: Hessian present (i, 0/1); of the present ones, back to back: rowptr (n + 1 each) colidx (i) val (d), lower triangle, sorted
 *   43-47 the flat Hessian (both triangles over x): rowptr colidx (i) val diagonal (d) long rows (i); all empty without a Hessian */
enum { PIPS_IPML_DIMS = 20, PIPS_IPML_SLOTS = 48 };
int pips_ipm_layout_probe(int n_blocks, const pips_ipm_block* blocks, const pips_csr_view* Q, int myl, int mzl, const double* bL,
                          const double* dlow, const double* dupp, const double* idlow, const double* idupp, int rank, int n_ranks,
                          int eliminate_z0, const double* col, const double* row, long long* dims, double* scalars, long long* sizes,
                          void* const* out);

/* pips_ipm_layout_probe for an input with cross Hessians R (pips_ipm_create_qp_cross): the same dims, scalars and arrays.  R_i's entries
 * stand in leaf i's border under the x0 Schur rows (slots 24-26) and in the flat Hessian (43-47); has_q is 1 with R alone; on a rank
 * != 0 with a cross Hessian among its own blocks the flat Hessian holds no Q0 block (qdiag keeps Q0's diagonal); given factors scale R
 * as pips_ipm_create_qp_cross does.  R == NULL: pips_ipm_layout_probe. */
int pips_ipm_layout_probe_cross(int n_blocks, const pips_ipm_block* blocks, const pips_csr_view* Q, const pips_csr_view* R, int myl, int mzl,
                                const double* bL, const double* dlow, const double* dupp, const double* idlow, const double* idupp, int rank,
                                int n_ranks, int eliminate_z0, const double* col, const double* row, long long* dims, double* scalars,
                                long long* sizes, void* const* out);

/* The tables of the packed blocked solves (Schur mode 2 with the sparse root), without a device; the code the engine builds its own
 * with.  bt_rowptr[b]: the S + 1 row pointers of block b's border (NULL: no border).  nb[b] (nblk entries): the block's non-empty
 * border columns; *nb_max their maximum = the right-hand sides of the packed solves; local_of_row[b] (S entries each): the local index
 * of Schur column s in block b, ascending in s, -1 for an empty column. */
int pips_schur_pack_probe(int nblk, int S, const int* const* bt_rowptr, int* nb, int* nb_max, int* const* local_of_row);

/* The compact target of the sparse Schur entries of section 1 (pips_hip_ldl_factor_schur_sparse / _batch), without a device; the code
 * the entries build theirs with, errors included.  bt_rowptr[b]: the S + 1 row pointers of block b's border (NULL: no border);
 * sc_rowptr / sc_colidx / lower: the caller's pattern as in section 1.  nb[b] (nblk entries): the block's non-empty border columns;
 * *n_touched = T, the distinct pattern positions any block's clique touches; pos (when cap >= T): those positions, ascending;
 * tab[b] (NULL: skipped; else nb[b] x nb[b] entries): entry la * nb[b] + lb, la >= lb, is the index into pos of the pair's place - (bm[lb],
 * bm[la]) of an upper pattern, (bm[la], bm[lb]) of a lower one, bm the block's non-empty columns ascending; the other half is 0. */
int pips_schur_target_probe(int nblk, int S, const int* const* bt_rowptr, const int* sc_rowptr, const int* sc_colidx, int lower, int* nb,
                            long long* n_touched, long long* pos, long long cap, int* const* tab);

/* The chunks pips_hip_kkt_solve_compressed_multi cuts nrhs right-hand sides into, without a device; the function the call itself uses.
 * from: the fewest right-hand sides that go by panels (0 = never); chunk_max: the most a chunk may hold (256); n_total: the length of
 * the leaf vector (several ranks: the longest of any rank); budget_bytes: the bound on n_total x chunk doubles (2 GiB).  *n_chunks: how
 * many; out (when cap >= *n_chunks; 3 ints each): first column, count, path (0 = the single solveCompressed, one column per chunk;
 * 1 = panels).  A panel chunk holds whole panels of 32 within the budget, at most max(chunk_max, 32), never fewer than 32 - the last
 * chunk takes what is left. */
int pips_kkt_multi_plan_probe(int nrhs, int from, int chunk_max, long long n_total, long long budget_bytes, int* out, int cap, int* n_chunks);

/* ---- 6. input files ---------------------------------------------------------------------------------------------------
 * One block of a block-structured LP from a "jacobian" GDX file, the format gmspips_reader opens per block
 * (Drivers/gams/gmspips/gmspips_reader.cpp:30-60; extraction rules of readBlock, gmspipsio.c:1357-2033; fields of
 * GMSPIPSBlockData_t, gmspipsio.h:5-58).  Uncompressed GDX version 7 files.  offset = stage number of block 0 (the
 * reference passes 1).  Host only. */
int pips_gdx_read_block(void** block, const char* path, int num_blocks, int act_block, int offset);
/* counts14 = {n0, ni, mA, mC, mBL, mDL, nnzA, nnzB, nnzC, nnzD, nnzBL, nnzDL, numBlocks, blockID} */
int pips_gdx_block_counts(void* block, long long* counts14);
/* which: 0 c, 1 xlow, 2 xupp, 3 ixlow, 4 ixupp, 5 b, 6 clow, 7 cupp, 8 iclow, 9 icupp, 10 bL, 11 dlow, 12 dupp, 13 idlow,
 * 14 idupp (indicators as 0.0 / 1.0); out may be NULL to query *length */
int pips_gdx_block_vector(void* block, int which, double* out, int capacity, int* length);
/* which: 0 A, 1 B, 2 C, 3 D, 4 BL, 5 DL; *present = 0 where the reference leaves the matrix pointers NULL; the arrays (any may
 * be NULL) must hold rows + 1 / nnz / nnz entries (sizes from pips_gdx_block_counts) */
int pips_gdx_block_matrix(void* block, int which, int* present, int* rows, int* cols, int* rowptr, int* colidx, double* val);
void pips_gdx_block_destroy(void* block);

#ifdef __cplusplus
}
#endif
#endif /* PIPS_HIP_H */
