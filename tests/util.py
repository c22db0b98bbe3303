"""Shared helpers for the tests: synthetic arrowhead problems in both the product's and the oracle's
representation.  The generator is the product's host harness (pips_gen_*); the oracle consumes the same matrices."""
import numpy as np
import scipy.sparse as sp

import pips_ipmpp_amd as pa
from oracle import oracle as orc


class Problem:
    """N blocks, each n_i vars / my_i equalities, n0 first-stage vars, myl linking equalities."""

    def __init__(self, seed, N, n_i, my_i, n0, myl, rho, dual_reg=1e-8, diag_lo=-4.0, diag_hi=4.0):
        self.N, self.n_i, self.my_i, self.n0, self.myl = N, n_i, my_i, n0, myl
        self.S = n0 + myl
        self.blocks = []
        for b in range(1, N + 1):
            W, T, F, c, xs = pa.gen_block(seed, b, n_i, my_i, n0, myl, rho)
            K, dpos = pa.kkt_leaf_assemble(n_i, W)
            Bt = pa.border_assemble(n_i, my_i, 0, n0, 0, A=T if n0 else None, F=F if myl else None)
            d = pa.gen_diagonal(seed, b, n_i, diag_lo, diag_hi)
            diag = np.concatenate([d, -dual_reg * np.ones(my_i)])
            K.val[dpos] = diag
            self.blocks.append(dict(W=W, T=T, F=F, K=K, dpos=dpos, Bt=Bt, diag=diag, c=c, xs=xs))
        self.F0, self.c0, self.x0s = pa.gen_root(seed, n0, myl)
        self.x_diag0 = pa.gen_diagonal(seed, 0, n0, diag_lo, diag_hi)

    @property
    def n_leaf(self):
        return self.n_i + self.my_i

    def K_scipy(self, b):
        K = self.blocks[b]["K"]
        return sp.csr_matrix((K.val.copy(), K.colidx, K.rowptr), shape=(K.nrows, K.ncols))

    def K_full(self, b):
        K = self.K_scipy(b)
        return (K + sp.tril(K, -1).T).tocsc()

    def Bt_scipy(self, b):
        return self.blocks[b]["Bt"].to_scipy()

    def oracle_leaf(self, b, **kw):
        s = orc.OracleLdl(self.K_scipy(b), n_primal=self.n_i, **kw)
        s.matrixChanged()
        return s

    def oracle_schur(self, blocks=None):
        """SC after assembleLocalKKT over the given blocks (row-major, lower authoritative)."""
        SC = np.zeros((self.S, self.S))
        for b in (range(self.N) if blocks is None else blocks):
            orc.add_term_to_schur_compl_blocked(SC, self.oracle_leaf(b), self.Bt_scipy(b))
        return SC

    def oracle_finalize(self, SC):
        return orc.finalize_kkt_dense(SC, self.n0, 0, self.myl, 0, self.x_diag0, F0=self.F0.to_scipy())


class TimeCoupledProblem(Problem):
    """Same as Problem but W_i is banded (time-coupled constraints): chain-like elimination trees, hundreds of levels,
    wide amalgamated supernodes, head-to-head update segments."""

    def __init__(self, seed, N, n_i, my_i, n0, myl, bw):
        super().__init__(seed, N, n_i, my_i, n0, myl, 0.02)
        rng = np.random.default_rng(seed)
        for b, blk in enumerate(self.blocks):
            rows, cols = [], []
            for r in range(my_i):
                center = int(r * n_i / my_i)
                cs = np.union1d(np.clip(center + rng.integers(-bw, bw + 1, 5), 0, n_i - 1), [center])
                rows += [r] * len(cs)
                cols += list(cs)
            W = sp.csr_matrix((rng.uniform(-1, 1, len(rows)), (rows, cols)), shape=(my_i, n_i))
            W.sum_duplicates()
            W.sort_indices()
            Wp = pa.Csr(my_i, n_i, W.indptr, W.indices, W.data)
            K, dpos = pa.kkt_leaf_assemble(n_i, Wp)
            K.val[dpos] = blk["diag"]
            blk.update(W=Wp, K=K, dpos=dpos)


def hip_lower_as_rowmajor(buf, S):
    """The HIP path writes SC column-major with the lower triangle valid; return the row-major lower triangle."""
    A = np.asarray(buf).reshape(S, S)   # A[c][r] = SC(r, c)
    return np.tril(A.T)


# ----------------------------------------------------------------------------------------------------------------------
# the sweeps judged without iterative refinement (tests/test_unrefined_reference_cpu.py, tests/test_unrefined_sweeps_gpu.py)
# ----------------------------------------------------------------------------------------------------------------------
UNIT_ROUNDOFF = 2.0 ** -53
UNREFINED_M_CAP = 64      # the largest margin the predicate may ever be given


class UnrefinedReference:
    """One K (a block of a Problem) and a set of right-hand sides (one per row of B): the oracle's unrefined solutions X0, its twice
    refined ones XS, and the oracle's own measures.  Everything is computed once and read-only, tests share it."""

    def __init__(self, prob, b, B):
        self.prob, self.b = prob, b
        Kf = prob.K_full(b).tocsr()
        Kf.sort_indices()
        assert np.all(np.diff(Kf.indptr) > 0)              # (every row has its diagonal: reduceat below needs no empty segment)
        self._indptr, self._indices = Kf.indptr[:-1].copy(), Kf.indices.copy()
        self._data = Kf.data.astype(np.longdouble)
        self.norm_K = float(np.abs(Kf).sum(axis=1).max())
        self.B = np.ascontiguousarray(np.atleast_2d(B), dtype=np.float64)
        o0 = prob.oracle_leaf(b, refine_steps=0)
        self.inertia = o0.get_inertia()
        self.X0 = o0.solve(self.B.copy())
        self.XS = prob.oracle_leaf(b, refine_steps=2).solve(self.B.copy())
        self.eta_ref = self.backward_errors(self.X0)
        self.fwd_ref = np.abs(self.X0 - self.XS).max(axis=1)
        self.xs_norm = np.abs(self.XS).max(axis=1)
        for a in (self.B, self.X0, self.XS, self.eta_ref, self.fwd_ref, self.xs_norm):
            a.setflags(write=False)

    def backward_errors(self, X):
        """eta(x) = ||b - K x||inf / (||K||inf ||x||inf + ||b||inf) per right-hand side, the residual formed in long double from the
        full symmetric K.  A zero right-hand side with a zero solution has eta = 0 (0 / 0 otherwise), anything non-finite has eta = inf."""
        X = np.atleast_2d(X)
        R = self.B.astype(np.longdouble) - np.add.reduceat(self._data[None, :] * X.astype(np.longdouble)[:, self._indices], self._indptr, axis=1)
        num = np.abs(R).max(axis=1).astype(np.float64)
        den = self.norm_K * np.abs(X).max(axis=1) + np.abs(self.B).max(axis=1)
        eta = np.where(num == 0.0, 0.0, num / np.where(den > 0.0, den, 1.0))
        return np.where(np.isfinite(eta), eta, np.inf)

    def backward_ratios(self, X):
        """eta(x) / max(eta_ref, 2^-53) per right-hand side: what the margin M bounds"""
        return self.backward_errors(X) / np.maximum(self.eta_ref, UNIT_ROUNDOFF)

    def forward_ratios(self, X):
        """||x - x*||inf / max(||x_ref0 - x*||inf, 2^-53 ||x*||inf) per right-hand side (0 where x = x* = 0)"""
        err = np.abs(np.atleast_2d(X) - self.XS).max(axis=1)
        den = np.maximum(self.fwd_ref, UNIT_ROUNDOFF * self.xs_norm)
        q = np.where(err == 0.0, 0.0, err / np.where(den > 0.0, den, 1.0))
        return np.where(np.isfinite(q), q, np.inf)

    def accepts(self, X, M):
        """the predicate, per right-hand side: backward and forward"""
        assert M <= UNREFINED_M_CAP
        return (self.backward_ratios(X) <= M) & (self.forward_ratios(X) <= M)


# the cases: which K, which right-hand sides.  Shapes are the smallest that still select each kernel (see the GPU module's docstring).
UNREFINED_SINGLE_SHAPES = {
    # id: (kind, n_i, my_i) - the time-coupled blocks of test_leaf_gpu.py's chain_and_spine / dissected cases (banded W, half width 6)
    "chain_and_spine": ("time_coupled", 600, 300),
    "dissected": ("time_coupled", 3000, 1500),
    # leaf dimensions 127, 128, 129, 257 for the all-tail cut: the last 128-row tile empty / full / one row / one row past two tiles
    "tail127": ("random", 85, 42),
    "tail128": ("random", 86, 42),
    "tail129": ("random", 86, 43),
    "tail257": ("random", 171, 86),
}
UNREFINED_MULTI_NRHS = (2, 7, 8, 31, 32, 33, 64, 65, 256, 257)
UNREFINED_BATCH_SHAPES = {"three_large": (3, 2600, 1300, 20, 10, 0.004), "seventy_small": (70, 400, 200, 10, 10, 0.03)}
UNREFINED_BATCH_NRHS = 33


def unrefined_single_problem(shape):
    kind, n_i, my_i = UNREFINED_SINGLE_SHAPES[shape]
    return TimeCoupledProblem(5, 1, n_i, my_i, 0, 0, 6) if kind == "time_coupled" else Problem(17, 1, n_i, my_i, 0, 0, 0.1)


def unrefined_multi_problem():
    n_i = 1500       # the block of test_leaf_many_rhs_on_the_matrix_pipe: a dense tail of several tiles under a sparse head
    return Problem(5, 1, n_i, n_i // 2, 4, 4, 6.0 / n_i)


def unrefined_batch_problem(shape):
    # the primal diagonal spans 1e-2 .. 1e2 instead of the default 1e-4 .. 1e4: in 70 random blocks there are primal variables without
    # a constraint entry and a diagonal near 1e-4 - x_j = b_j / d_j then carries ||x||inf while its rounding error leaves a residual
    # of d_j * error, and ||K||inf ||x||inf hides it: the float32-rounded solution passed the predicate (ratio 39 at block 61)
    return Problem(77, *UNREFINED_BATCH_SHAPES[shape], diag_lo=-2.0, diag_hi=2.0)


def unrefined_rhs_rows(prob, b, nrhs, seed, units=True):
    """nrhs right-hand sides, one per row, and which row is what: Gaussian rows, of which the last is scaled by 1e6; from 7 rows on row 1
    is all zero and rows 2 and 3 are unit vectors whose index lies in the head and in the tail of the device's elimination order (2 rows:
    the scaled one and the zero one; units=False: no unit vectors)."""
    n = prob.n_leaf
    R = np.random.default_rng(seed).standard_normal((nrhs, n))
    what = {}
    if nrhs >= 2:
        what["scaled"] = nrhs - 1 if nrhs > 2 else 0
        R[what["scaled"]] *= 1e6
        what["zero"] = 1
        R[1] = 0.0
    if nrhs >= 7 and units:
        probe = pa.symbolic_probe(prob.blocks[b]["K"], prob.n_i, want_perm=True)
        n_head, m, perm = probe["n_head"], probe["m"], probe["perm"]
        assert n_head > 0 and m > 0 and n_head + m == n, probe
        what["unit_head"], what["unit_tail"] = 2, 3
        R[2:4] = 0.0
        R[2, perm[n_head // 2]] = 1.0             # perm[k] = the row of K that the device eliminates k-th; the tail is the last m of them
        R[3, perm[n_head + m // 2]] = 1.0
    return R, what


_unrefined_cache = {}


def unrefined_reference(kind, key):
    """The shared references: ("single", shape) one Gaussian right-hand side; ("multi", nrhs) the rows of unrefined_rhs_rows;
    ("batch", (shape, block, rep)) one Gaussian right-hand side per block and repetition; ("batch_multi", shape) block 0, 33 rows (Gaussian, one scaled, one zero)."""
    k = (kind, key)
    if k not in _unrefined_cache:
        if kind == "single":
            prob = _unrefined_cached_problem(kind, key)
            ref = UnrefinedReference(prob, 0, np.random.default_rng(1).standard_normal((1, prob.n_leaf)))
        elif kind == "multi":
            prob = _unrefined_cached_problem(kind, None)
            R, what = unrefined_rhs_rows(prob, 0, key, key)
            ref = UnrefinedReference(prob, 0, R)
            ref.what = what
        elif kind == "batch":
            shape, b = key
            prob = _unrefined_cached_problem(kind, shape)
            ref = UnrefinedReference(prob, b, np.random.default_rng(1000 + b).standard_normal((3, prob.n_leaf)))   # row = repetition
        else:
            prob = _unrefined_cached_problem("batch", key)
            R, what = unrefined_rhs_rows(prob, 0, UNREFINED_BATCH_NRHS, 7, units=False)
            ref = UnrefinedReference(prob, 0, R)
            ref.what = what
        _unrefined_cache[k] = ref
    return _unrefined_cache[k]


def _unrefined_cached_problem(kind, key):
    k = ("problem", kind, key)
    if k not in _unrefined_cache:
        _unrefined_cache[k] = (unrefined_single_problem(key) if kind == "single" else unrefined_multi_problem() if kind == "multi"
                               else unrefined_batch_problem(key))
    return _unrefined_cache[k]


# ----------------------------------------------------------------------------------------------------------------------
# the Schur contribution judged against a long-double reference (tests/test_schur_reference_cpu.py, tests/test_schur_judged_gpu.py)
# ----------------------------------------------------------------------------------------------------------------------
class SchurReference:
    """SC = - sum_b Br_b^T K_b^-1 Br_b of a Problem, twice: SC_star from the oracle's twice refined solves of the densified border columns,
    Br^T X and the sum over the blocks accumulated in long double and rounded to float64 once; SC_ref0 by the oracle's plain FP64 algorithm
    (add_term_to_schur_compl_blocked over unrefined solves, the sign convention of Problem.oracle_schur).  Row-major, only the lower triangle
    counts.  finalized: with the constant root entries and diagonals of finalizeKKTdense in both (what a KktSystem hands out).  The same pair
    is kept per block (block_star, block_ref0: the term of that block alone, non-zero on bmaps[b] x bmaps[b] only).  Computed once, read-only."""

    def __init__(self, prob, finalized=False):
        self.prob, S = prob, prob.S
        total = np.zeros((S, S), np.longdouble)
        self.SC_ref0 = np.zeros((S, S))
        self.inertia, self.bmaps, self.block_star, self.block_ref0 = [], [], [], []
        for b in range(prob.N):
            Bt = prob.Bt_scipy(b)
            Bt.sort_indices()
            cols = np.nonzero(np.diff(Bt.indptr) > 0)[0]          # the block's non-empty border columns: its bmap
            o0 = prob.oracle_leaf(b, refine_steps=0)
            self.inertia.append(o0.get_inertia())
            t0 = orc.add_term_to_schur_compl_blocked(np.zeros((S, S)), o0, Bt)
            X = prob.oracle_leaf(b, refine_steps=2).solve(np.ascontiguousarray(Bt[cols].toarray()))      # (len(cols), n_leaf): K^-1 Br e_col per row
            term = np.zeros((S, S), np.longdouble)
            if len(cols):
                # (Br^T x)[r] = sum of Bt's row r against x, in long double: the rows between two non-empty ones hold no entry, so the segments
                # that start at the non-empty rows are exactly their entries
                term[np.ix_(cols, cols)] = -np.add.reduceat(Bt.data.astype(np.longdouble)[None, :] * X.astype(np.longdouble)[:, Bt.indices], Bt.indptr[cols], axis=1)
            total += term
            self.SC_ref0 += t0
            self.bmaps.append(cols)
            self.block_star.append(np.tril(term.astype(np.float64)))
            self.block_ref0.append(np.tril(t0))
        if finalized:
            total += prob.oracle_finalize(np.zeros((S, S))).astype(np.longdouble)     # (constants put into zeros: exact)
            prob.oracle_finalize(self.SC_ref0)
        self.SC_star = np.tril(total.astype(np.float64))
        self.SC_ref0 = np.tril(self.SC_ref0)
        self.scale = float(np.abs(self.SC_star).max())
        self.err_ref0 = float(np.abs(self.SC_ref0 - self.SC_star).max())
        self.block_scale = [float(np.abs(t).max()) for t in self.block_star]
        self.block_err_ref0 = [float(np.abs(r - t).max()) for r, t in zip(self.block_ref0, self.block_star)]
        for a in [self.SC_star, self.SC_ref0] + self.bmaps + self.block_star + self.block_ref0:
            a.setflags(write=False)

    @staticmethod
    def _quotient(err, den):
        q = 0.0 if err == 0.0 else err / (den if den > 0.0 else 1.0)
        return float(q) if np.isfinite(q) else float("inf")

    def ratio(self, SC, times=1):
        """max|SC - SC*| / max(err_ref0, 2^-53 scale) over the lower triangle.  times = 2: a contribution accumulated twice, judged against
        2 SC* - the reference doubles exactly and its own error with it, so the denominator doubles too."""
        return self._quotient(float(np.abs(np.tril(SC) - times * self.SC_star).max()), times * max(self.err_ref0, UNIT_ROUNDOFF * self.scale))

    def accepts(self, SC, M, times=1):
        assert M <= UNREFINED_M_CAP
        return self.ratio(SC, times) <= M

    def block_ratio(self, b, SC):
        """the same quotient for block b factored alone, over the rows and columns of its bmap (inf if anything outside them is touched)"""
        idx = np.ix_(self.bmaps[b], self.bmaps[b])
        L = np.tril(SC)
        outside = L.copy()
        outside[idx] = 0.0
        if outside.any():
            return float("inf")
        return self._quotient(float(np.abs(L[idx] - self.block_star[b][idx]).max()) if len(self.bmaps[b]) else 0.0,
                              max(self.block_err_ref0[b], UNIT_ROUNDOFF * self.block_scale[b]))

    def block_accepts(self, b, SC, M):
        assert M <= UNREFINED_M_CAP
        return self.block_ratio(b, SC) <= M


# the cases: (n_i, S, N, borders).  my_i = n_i // 2 (leaves of dimension 255 and 600: 2 and 5 tail tiles when all of K is in the tail), S is
# split n0 = S // 2, myl = S - n0; the widths sit at the chunk of the blocked solves (32) and at the tile (128).  borders = "hetero":
# block 1 has only the n0 border columns, block 2 only the myl ones - bmaps that differ and are proper subsets.
SCHUR_N_I = (170, 400)
SCHUR_WIDTHS = (1, 31, 32, 33, 127, 128, 129, 257)
SCHUR_WIDTHS_THREE_BLOCKS = (32, 33, 129)
SCHUR_PROBLEMS = [(n_i, S, 1, "full") for n_i in SCHUR_N_I for S in SCHUR_WIDTHS] + \
                 [(n_i, S, 3, "full") for n_i in SCHUR_N_I for S in SCHUR_WIDTHS_THREE_BLOCKS] + [(n_i, 129, 3, "hetero") for n_i in SCHUR_N_I]


def schur_problem(n_i, S, N, borders):
    # primal diagonals within 1e-2 .. 1e2, as unrefined_batch_problem (and for its reason: nothing badly scaled hides an error)
    n0 = S // 2
    prob = Problem(300 + S, N, n_i, n_i // 2, n0, S - n0, 8.0 / n_i, diag_lo=-2.0, diag_hi=2.0)
    rng = np.random.default_rng(300 + S)
    for blk in prob.blocks:
        # the generator's T_i leaves some of the n0 columns without an entry; the widths under test are those of the non-empty border columns,
        # so every column gets one: two random entries per row as the generator's, and one in row j mod my_i of column j
        rows = np.concatenate([np.repeat(np.arange(prob.my_i), min(2, n0)), np.arange(n0) % prob.my_i]).astype(np.int64)
        cols = np.concatenate([rng.integers(0, max(n0, 1), prob.my_i * min(2, n0)), np.arange(n0)]).astype(np.int64)
        T = sp.csr_matrix((rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows)), (rows, cols)), shape=(prob.my_i, n0))
        T.sum_duplicates()
        T.sort_indices()
        blk["T"] = pa.Csr(prob.my_i, n0, T.indptr, T.indices, T.data)
        blk["Bt"] = pa.border_assemble(n_i, prob.my_i, 0, n0, 0, A=blk["T"] if n0 else None, F=blk["F"])
    if borders == "hetero":
        blk = prob.blocks[1]
        top = pa.border_assemble(n_i, prob.my_i, 0, n0, 0, A=blk["T"], F=None)          # n0 rows; the myl linking ones follow, empty
        blk["Bt"] = pa.Csr(S, prob.n_leaf, np.concatenate([top.rowptr, np.full(S - n0, top.rowptr[-1], np.int32)]), top.colidx, top.val)
        blk = prob.blocks[2]
        blk["Bt"] = pa.border_assemble(n_i, prob.my_i, 0, n0, 0, A=None, F=blk["F"])    # S rows, the first n0 empty
    return prob


_schur_cache = {}


def schur_reference(key, finalized=False):
    """The shared SchurReference of a case of SCHUR_PROBLEMS (and its Problem: .prob)."""
    if ("problem", key) not in _schur_cache:
        _schur_cache[("problem", key)] = schur_problem(*key)
    if (key, finalized) not in _schur_cache:
        _schur_cache[(key, finalized)] = SchurReference(_schur_cache[("problem", key)], finalized)
    return _schur_cache[(key, finalized)]


# ----------------------------------------------------------------------------------------------------------------------
# the dense root's solves judged against a long-double reference (tests/test_dense_root_reference_cpu.py, tests/test_dense_root_judged_gpu.py)
# ----------------------------------------------------------------------------------------------------------------------
DENSE_ROOT_FAMILIES = {"flat": 0.0, "spread": 2.0}      # the spread of the diagonals in decades: cond about 20, and 1e2 .. 1e3
DENSE_ROOT_TILE = 128


def dense_root_matrix(n, n_primal, seed, spread):
    """[[H, A^T], [A, -G]] with H = diag(10 ** U(-spread, spread)) + R R^T / r (R n_primal x r standard normal, r = max(1, n_primal // 8)),
    G = diag(10 ** U(-spread, spread)) and A (n - n_primal) x n_primal standard normal, kept where a uniform draw is below 0.3: quasi-definite,
    inertia (n_primal, n - n_primal, 0) in the given order."""
    rng = np.random.default_rng(seed)
    m, r = n - n_primal, max(1, n_primal // 8)
    dH = 10.0 ** rng.uniform(-spread, spread, n_primal)
    R = rng.standard_normal((n_primal, r))
    H = np.diag(dH) + R @ R.T / r
    G = np.diag(10.0 ** rng.uniform(-spread, spread, m))
    A = rng.standard_normal((m, n_primal))
    A = A * (rng.random((m, n_primal)) < 0.3)
    return np.block([[H, A.T], [A, -G]])


def dense_root_zero_diagonal(n, seed):
    """N + N^T with its diagonal zeroed (tests/test_root_pivoting_gpu.py): no 1 x 1 pivot exists at the start of any tile"""
    N = np.random.default_rng(seed).standard_normal((n, n))
    M = N + N.T
    np.fill_diagonal(M, 0.0)
    return M


def dense_root_rhs(n, seed):
    """the right-hand sides, one per row: three standard-normal ones, e_0 and e_{n-1}"""
    B = np.zeros((5, n))
    B[:3] = np.random.default_rng(seed).standard_normal((3, n))
    B[3, 0] = 1.0
    B[4, n - 1] = 1.0
    return B


def dense_root_with_garbage_above(M, seed):
    """M's lower triangle under a strict upper triangle of other finite numbers (standard normal, its own seed): what the device is handed,
    "lower triangle authoritative" being the contract"""
    n = M.shape[0]
    return np.tril(M) + np.triu(np.random.default_rng(seed).standard_normal((n, n)), 1)


def dense_root_symmetric_from_lower(A):
    return np.tril(A) + np.tril(A, -1).T


def dense_root_ldl_static(S, skip_update_of=None):
    """Unblocked right-looking LDL^T of the symmetric S in the given order, plain FP64: (L unit lower, d).  skip_update_of = k: the rank-one
    update of pivot k is left out (a mutant of tests/test_dense_root_reference_cpu.py)."""
    A = np.array(S, dtype=np.float64)
    n = A.shape[0]
    d = np.empty(n)
    for k in range(n):
        d[k] = A[k, k]
        u = A[k + 1:, k].copy()
        l = u / d[k]
        if k != skip_update_of:
            A[k + 1:, k + 1:] -= np.outer(l, u)
        A[k + 1:, k] = l
    L = np.tril(A, -1)
    np.fill_diagonal(L, 1.0)
    return L, d


def dense_root_ldl_solve(L, d, B):
    """L D L^T x = b for every row b of B by column substitution, plain FP64"""
    X = np.array(np.atleast_2d(B), dtype=np.float64).T.copy()        # (n, nrhs)
    n = X.shape[0]
    for k in range(n - 1):
        X[k + 1:] -= np.outer(L[k + 1:, k], X[k])
    X /= d[:, None]
    for k in range(n - 1, 0, -1):
        X[:k] -= np.outer(L[k, :k], X[k])
    return np.ascontiguousarray(X.T)


class DenseRootReference:
    """One symmetric M (its lower triangle counts) and right-hand sides (one per row of B): X_star from LAPACK dsytrf / dsytrs and refinement
    steps on a long-double x (the residual formed in long double - exactly from the third step on, see _residual_rounded_once - and the correction
    added in long double) until a correction is below 2^-58 max|x|, rounded to FP64 once; X_lapack, LAPACK's unrefined dsytrs solution - x_ref0 of
    Bunch-Kaufman pivoting (mode 1); static=True: the unblocked FP64 LDL^T in the given order (L, d) and its solution X_static - x_ref0 of the
    static order (mode 0).  The predicate is UnrefinedReference's, per right-hand side.  Computed once, read-only."""
    MAX_STEPS = 5

    def __init__(self, M, B, n_primal=None, static=True):
        import scipy.linalg as sla
        self.M = dense_root_symmetric_from_lower(np.asarray(M, dtype=np.float64))
        self.n, self.n_primal = self.M.shape[0], n_primal
        self.B = np.ascontiguousarray(np.atleast_2d(B), dtype=np.float64)
        self._M_ld = self.M.astype(np.longdouble)
        self.norm_M = float(np.abs(self.M).sum(axis=1).max())
        ldu, ipiv, info = sla.lapack.dsytrf(np.tril(self.M), lower=1)
        assert info == 0
        X0, info = sla.lapack.dsytrs(ldu, ipiv, self.B.T.copy(), lower=1)
        assert info == 0
        self.X_lapack = np.ascontiguousarray(X0.T)
        X = self.X_lapack.astype(np.longdouble)
        self.refinement_steps, self.converged = 0, False
        while self.refinement_steps < self.MAX_STEPS and not self.converged:
            # two steps with the residual accumulated in long double settle all but the worst conditioned case; what they leave takes it exact
            Rres = (self.B.astype(np.longdouble) - X @ self._M_ld).astype(np.float64) if self.refinement_steps < 2 else self._residual_rounded_once(X)
            dX, info = sla.lapack.dsytrs(ldu, ipiv, Rres.T.copy(), lower=1)
            assert info == 0
            X = X + dX.T.astype(np.longdouble)
            self.refinement_steps += 1
            self.converged = bool(np.all(np.abs(dX.T).max(axis=1) <= 2.0 ** -58 * np.abs(X).max(axis=1).astype(np.float64)))
        self.X_star = X.astype(np.float64)
        self.xs_norm = np.abs(self.X_star).max(axis=1)
        self.L = self.d = self.X_static = None
        x_ref0 = {1: self.X_lapack}
        if static:
            self.L, self.d = dense_root_ldl_static(self.M)
            self.X_static = dense_root_ldl_solve(self.L, self.d, self.B)
            x_ref0[0] = self.X_static
        self.eta_ref = {mode: self.backward_errors(x) for mode, x in x_ref0.items()}
        self.fwd_ref = {mode: np.abs(x - self.X_star).max(axis=1) for mode, x in x_ref0.items()}
        for a in [self.M, self.B, self.X_lapack, self.X_star, self.xs_norm, self.L, self.d, self.X_static] + list(self.eta_ref.values()) + list(self.fwd_ref.values()):
            if a is not None:
                a.setflags(write=False)

    def _residual_rounded_once(self, X):
        """B - X M of a long-double X, every entry the exact sum rounded to FP64 once.  A residual accumulated in plain long double carries
        an error of some 2^-64 ||M|| ||x||, and the correction solved from it stalls at cond(M) 2^-64 max|x|: 2^-56 on the all-primal case of
        the spread family, above the 2^-58 the refinement has to reach.  So the long-double x is split into two doubles, every product
        into its rounded value and its exact error (Dekker), and each row is summed with math.fsum."""
        import math
        hi = X.astype(np.float64)
        lo = (X - hi.astype(np.longdouble)).astype(np.float64)           # (exact: 64 bits fit into 53 + 53)

        def split(a):
            c = 134217729.0 * a                                           # 2^27 + 1 (Veltkamp)
            h = c - (c - a)
            return h, a - h

        Mh, Ml = split(self.M)
        out = np.empty(self.B.shape)
        for i in range(self.B.shape[0]):
            terms = [self.B[i][None, :]]
            for x in (hi[i], lo[i]):
                xh, xl = split(x)
                P = x[:, None] * self.M                                   # P[j, k] = x_j M[j, k]: column k sums to (x M)_k
                E = ((xh[:, None] * Mh - P) + xh[:, None] * Ml + xl[:, None] * Mh) + xl[:, None] * Ml
                terms += [-P, -E]
            out[i] = [math.fsum(col) for col in np.concatenate(terms, axis=0).T.tolist()]
        return out

    def backward_errors(self, X):
        """eta(x) = ||b - M x||inf / (||M||inf ||x||inf + ||b||inf) per right-hand side, the residual formed in long double; anything
        non-finite has eta = inf"""
        X = np.atleast_2d(X)
        with np.errstate(all="ignore"):
            Rres = self.B.astype(np.longdouble) - X.astype(np.longdouble) @ self._M_ld
            num = np.abs(Rres).max(axis=1).astype(np.float64)
            den = self.norm_M * np.abs(X).max(axis=1) + np.abs(self.B).max(axis=1)
            eta = np.where(num == 0.0, 0.0, num / np.where(den > 0.0, den, 1.0))
        return np.where(np.isfinite(eta), eta, np.inf)

    def ratios(self, X, mode=0):
        """(forward, backward) per right-hand side: max|x - x*| / max(max|x_ref0 - x*|, 2^-53 max|x*|) and eta(x) / max(eta(x_ref0), 2^-53)
        - what the margin M bounds.  mode: the pivoting mode, it selects x_ref0."""
        X = np.atleast_2d(X)
        with np.errstate(all="ignore"):
            err = np.abs(X - self.X_star).max(axis=1)
            den = np.maximum(self.fwd_ref[mode], UNIT_ROUNDOFF * self.xs_norm)
            fwd = np.where(err == 0.0, 0.0, err / np.where(den > 0.0, den, 1.0))
        fwd = np.where(np.isfinite(fwd), fwd, np.inf)
        return fwd, self.backward_errors(X) / np.maximum(self.eta_ref[mode], UNIT_ROUNDOFF)

    def accepts(self, X, M, mode=0):
        """the predicate, per right-hand side: forward and backward"""
        assert M <= UNREFINED_M_CAP
        fwd, bwd = self.ratios(X, mode)
        return (fwd <= M) & (bwd <= M)


# the cases (n, n_primal, family): the smallest that still select each piece - 128-wide tiles, 32-wide sub-blocks of the blocked diagonal tile,
# K ranges the plan cuts only from three or four tile columns on.  n_primal = (2 n) // 3, at n = 257 also all dual, the sign boundary on the tile
# edge, one past it, all primal.
DENSE_ROOT_SIZES = (1, 31, 32, 33, 127, 128, 129, 257, 385, 513)
DENSE_ROOT_CASES = [(n, (2 * n) // 3, "flat") for n in DENSE_ROOT_SIZES] + [(n, (2 * n) // 3, "spread") for n in DENSE_ROOT_SIZES if n >= 129] + \
                   [(257, n_primal, fam) for fam in DENSE_ROOT_FAMILIES for n_primal in (0, 128, 129, 257)]
DENSE_ROOT_ZERO_DIAGONAL_SIZES = (128, 300)


def dense_root_case_id(case):
    return f"n{case[0]}-p{case[1]}-{case[2]}"


def dense_root_case_matrix(case):
    n, n_primal, family = case
    if family == "zero_diagonal":
        return dense_root_zero_diagonal(n, 10 * n + 3), 10 * n + 3
    seed = 10 * n + {"flat": 1, "spread": 2}[family] + 7000 * (n_primal + 1 if n_primal != (2 * n) // 3 else 0)
    return dense_root_matrix(n, n_primal, seed, DENSE_ROOT_FAMILIES[family]), seed


def dense_root_case_inputs(case):
    """(M, B, seed of the strict upper triangle the device is handed) of a case"""
    M, seed = dense_root_case_matrix(case)
    return M, dense_root_rhs(case[0], seed + 500000), seed + 900000


_dense_root_cache = {}


def dense_root_reference(case):
    """The shared DenseRootReference of a case (n, n_primal, family) of DENSE_ROOT_CASES, or (n, None, "zero_diagonal"); .garbage_seed: the seed
    of the strict upper triangle the device is handed"""
    if case not in _dense_root_cache:
        M, B, garbage_seed = dense_root_case_inputs(case)
        ref = DenseRootReference(M, B, case[1], static=case[2] != "zero_diagonal")
        ref.garbage_seed = garbage_seed
        if case[2] == "zero_diagonal":
            ev = np.linalg.eigvalsh(ref.M)
            ref.inertia = (int((ev > 0).sum()), int((ev < 0).sum()), 0)
        else:
            ref.inertia = (case[1], case[0] - case[1], 0)
        _dense_root_cache[case] = ref
    return _dense_root_cache[case]
