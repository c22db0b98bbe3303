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


# ----------------------------------------------------------------------------------------------------------------------
# the static pivot rule when it rejects a pivot (tests/test_pivot_rule_reference_cpu.py, tests/test_pivot_rule_gpu.py)
# ----------------------------------------------------------------------------------------------------------------------
PIVOT_THR_REL, PIVOT_REPL_REL = 1e-13, 1e-8         # the library's defaults (engine.hip: thr_rel, repl_rel)
PIVOT_MUTANTS = ("replacement_sign_flipped", "repl_abs_where_pref_positive", "repl_rel_where_pref_zero", "magnitude_test_with_hint",
                 "perturbed_counted_negative", "tail_pref_not_refreshed", "dual_pref_without_sum", "updates_with_rejected_pivot")


class PivotRule:
    """The rule of fix_pivot (csrc/kernels.hip.h) as data: thr_rel, repl_rel and at most one mutation out of PIVOT_MUTANTS - what the CPU module
    runs through PivotRuleReference to show that the cases tell a wrong rule from the right one."""

    def __init__(self, thr_rel=PIVOT_THR_REL, repl_rel=PIVOT_REPL_REL, mutant=None):
        assert mutant is None or mutant in PIVOT_MUTANTS
        self.thr_rel, self.repl_rel, self.mutant = thr_rel, repl_rel, mutant

    def sign(self, hint, d):
        """the hint's sign, the pivot's own where there is none (fix_pivot: s)"""
        return float(hint) if hint != 0 else (-1.0 if d < 0 else 1.0)

    def decide(self, d, hint, pref, repl_abs):
        """(accepted, d'): accepted iff s d > thr_rel pref, else d' = s (pref > 0 ? repl_rel pref : repl_abs)"""
        s = self.sign(hint, d)
        sd = abs(d) if (self.mutant == "magnitude_test_with_hint" and hint != 0) else s * d
        if sd > self.thr_rel * pref:
            return True, d
        use_rel = pref > 0.0
        if self.mutant == "repl_abs_where_pref_positive":
            use_rel = False
        if self.mutant == "repl_rel_where_pref_zero":
            use_rel = True
        repl = self.repl_rel * pref if use_rel else repl_abs          # (FP64 products, as on the device)
        return False, (-s if self.mutant == "replacement_sign_flipped" else s) * repl


def pivot_leaf_pref(K, n_primal, rule=None):
    """pref per row of a leaf K (lower CSR, scipy) in the caller's order, FP64, summed in the order of k_pref_rows (csrc/kernels.hip.h): primal
    rows |a_kk|, dual rows |a_kk| + sum_j K_kj^2 / |K_jj| over the primal neighbours with a non-zero diagonal (OracleLdl._pivot_reference);
    without a hint |a_kk| for every row.  And repl_abs = repl_rel max|K| (k_block_absmax_finish: 1 in place of a maximum of 0)."""
    rule = rule or PivotRule()
    diag = np.abs(K.diagonal())
    pref = diag.copy()
    if n_primal >= 0 and rule.mutant != "dual_pref_without_sum":
        for i in range(n_primal, K.shape[0]):
            v = pref[i]
            for q in range(K.indptr[i], K.indptr[i + 1]):
                j = K.indices[q]
                if j < n_primal and diag[j] > 0.0:
                    v += K.data[q] * K.data[q] / diag[j]
            pref[i] = v
    amax = float(np.abs(K.data).max()) if K.nnz else 0.0
    return pref, rule.repl_rel * (amax if amax > 0.0 else 1.0)


class PivotRuleReference:
    """Dense right-looking LDL^T of P K P^T in long double under the device's static pivot rule, restated from csrc/kernels.hip.h (fix_pivot,
    k_pref_rows, k_pref_init, k_pref_tail, k_block_absmax_finish) and csrc/engine.hip (factor_prologue, factor_head; the dense root's
    factor_enqueue):
      leaf: pref as pivot_leaf_pref in the order perm; when the head (the first n_head positions) is eliminated the last m positions take
            pref = max(pref, |diagonal as it then stands|); repl_abs = repl_rel max|K|;
      root: perm = identity, n_head = 0, pref = |diagonal| (overwritten), repl_abs = repl_rel max|diagonal|.
    A pivot k replaced by d'_k makes the factors those of K' = K + (d'_k - d_k) e_k e_k^T exactly, d_k the pivot as it stood.
    K_lower: scipy CSR, lower triangle, the caller's numbering; hint: n_primal, or -1 for none; perm[k] = the row eliminated k-th.
    Yields per position: stood (the pivot as it stood), accepted, ratio (s d / pref, inf where pref = 0 and s d > 0, 0 where both are 0),
    dprime, pref; triple (positive, negative, perturbed); Kp_lower (K' as lower CSR of the same pattern) and Kp_dense; solve(B) with its own
    factors in its own precision (for a mutant: what a device with that defect would return).
    variant: "right" - right-looking, divisions, dtype long double (the reference) or float64; "left_reverse" - FP64, every pivot and column
    summed from the last eliminated contribution to the first and multiplied by the rounded reciprocal of the pivot (the plain restatement of
    the decision margins)."""

    def __init__(self, K_lower, hint, perm, n_head, kind="leaf", rule=None, dtype=np.longdouble, variant="right"):
        self.rule = rule = rule or PivotRule()
        K_lower = sp.csr_matrix(K_lower)
        K_lower.sort_indices()
        self.K_lower, self.hint, self.kind = K_lower, hint, kind
        n = self.n = K_lower.shape[0]
        self.perm = perm = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
        self.n_head = n_head
        Kd = K_lower.toarray()
        Kd = np.tril(Kd) + np.tril(Kd, -1).T
        hints = np.zeros(n, np.int64) if hint < 0 else np.where(perm < hint, 1, -1)
        if kind == "leaf":
            pref_rows, self.repl_abs = pivot_leaf_pref(K_lower, hint, rule)
            pref = pref_rows[perm].copy()
            refresh = None if rule.mutant == "tail_pref_not_refreshed" else "max"
        else:
            assert n_head == 0
            dmax = float(np.abs(np.diag(Kd)).max())
            self.repl_abs = rule.repl_rel * (dmax if dmax > 0.0 else 1.0)
            pref = np.zeros(n)
            refresh = "overwrite"
        A0 = Kd[np.ix_(perm, perm)]
        self.exact_entry = np.diag(A0).copy()
        run = self._left_reverse if variant == "left_reverse" else self._right
        self.L, self.stood, self.dprime, self.accepted, self.pref = run(A0, hints, pref, refresh, np.float64 if variant == "left_reverse" else dtype)
        s = np.array([rule.sign(h, d) for h, d in zip(hints, self.stood)])
        sd = (s * self.stood).astype(np.float64)
        with np.errstate(all="ignore"):
            self.ratio = np.where(self.pref > 0.0, sd / np.where(self.pref > 0.0, self.pref, 1.0), np.where(sd > 0.0, np.inf, np.where(sd < 0.0, -np.inf, 0.0)))
        acc = self.accepted
        pos, neg, pert = int((acc & (self.dprime > 0)).sum()), int((acc & ~(self.dprime > 0)).sum()), int((~acc).sum())
        self.triple = (pos, neg + pert, 0) if rule.mutant == "perturbed_counted_negative" else (pos, neg, pert)
        self.rejected_positions = np.nonzero(~acc)[0]
        self.rejected_rows = perm[self.rejected_positions]
        # K': the diagonal entries of the rejected rows move by d' - d: exactly d' where d is the entry itself, else formed in long double
        newdiag = K_lower.diagonal().astype(np.longdouble)
        for k in self.rejected_positions:
            if self.stood[k] == newdiag[perm[k]]:
                newdiag[perm[k]] = self.dprime[k]
            else:
                newdiag[perm[k]] += np.longdouble(self.dprime[k]) - np.longdouble(self.stood[k])
        Kp = K_lower.copy().tolil()
        Kp.setdiag(newdiag.astype(np.float64))
        self.Kp_lower = Kp.tocsr()
        self.Kp_lower.sort_indices()
        self.Kp_dense = np.tril(self.Kp_lower.toarray()) + np.tril(self.Kp_lower.toarray(), -1).T

    def _decide_all(self, k, d, hints, pref):
        return self.rule.decide(float(d), int(hints[k]), float(pref[k]), self.repl_abs)

    def _right(self, A0, hints, pref, refresh, dtype):
        n, mutant = self.n, self.rule.mutant
        A = A0.astype(dtype)
        stood, dprime, accepted = np.zeros(n, dtype), np.zeros(n), np.zeros(n, bool)
        with np.errstate(all="ignore"):
            for k in range(n):
                if k == self.n_head and refresh is not None:
                    dg = np.abs(np.diag(A)[k:]).astype(np.float64)
                    pref[k:] = dg if refresh == "overwrite" else np.maximum(pref[k:], dg)
                stood[k] = A[k, k]
                accepted[k], dprime[k] = self._decide_all(k, stood[k], hints, pref)
                dp = stood[k] if accepted[k] else dtype(dprime[k])
                u = A[k + 1:, k].copy()
                idx = np.nonzero(u)[0]
                if idx.size:
                    ui = u[idx]
                    l = ui / dp
                    lu = ui / stood[k] if mutant == "updates_with_rejected_pivot" else l
                    ii = k + 1 + idx
                    A[np.ix_(ii, ii)] -= np.outer(lu, ui)
                    A[ii, k] = l
        L = np.tril(A, -1)
        return L, stood, dprime, accepted, pref

    def _left_reverse(self, A0, hints, pref, refresh, dtype):
        n = self.n
        A0 = A0.astype(np.float64)
        L = np.zeros((n, n))
        dfin, rd = np.zeros(n), np.zeros(n)
        stood, dprime, accepted = np.zeros(n), np.zeros(n), np.zeros(n, bool)

        def column(k, upto):
            """A0[k:, k] minus the contributions of the columns upto-1 .. 0 that reach row k, the last one first"""
            c = A0[k:, k].copy()
            for j in np.nonzero(L[k, :upto])[0][::-1]:
                c -= L[k:, j] * (L[k, j] * dfin[j])
            return c

        for k in range(n):
            if k == self.n_head and refresh is not None:
                dg = np.abs(np.array([column(i, k)[0] for i in range(k, n)]))
                pref[k:] = dg if refresh == "overwrite" else np.maximum(pref[k:], dg)
            c = column(k, k)
            stood[k] = c[0]
            accepted[k], dprime[k] = self._decide_all(k, stood[k], hints, pref)
            dfin[k] = stood[k] if accepted[k] else dprime[k]
            with np.errstate(all="ignore"):
                rd[k] = 1.0 / dfin[k]
            L[k + 1:, k] = c[1:] * rd[k]
        return L, stood, dprime, accepted, pref

    def solve(self, B):
        """L D' L^T (P x) = P b per row b of B by column substitution with this factorisation's own L and stored pivots, in its own precision,
        rounded to FP64 at the end"""
        dt = self.L.dtype
        X = np.atleast_2d(B).astype(dt)[:, self.perm].T.copy()
        dfin = np.where(self.accepted, self.stood, self.dprime.astype(dt))
        with np.errstate(all="ignore"):
            for k in range(self.n - 1):
                idx = np.nonzero(self.L[k + 1:, k])[0] + k + 1
                if idx.size:
                    X[idx] -= np.outer(self.L[idx, k], X[k])
            X /= dfin[:, None]
            for k in range(self.n - 1, 0, -1):
                idx = np.nonzero(self.L[k, :k])[0]
                if idx.size:
                    X[idx] -= np.outer(self.L[k, idx], X[k])
        out = np.empty((X.shape[1], self.n))
        out[:, self.perm] = X.T.astype(np.float64)
        return out


class _OneLeafMatrix:
    """what UnrefinedReference asks of a Problem, for one lower-CSR matrix (K' of a PivotRuleReference)"""

    def __init__(self, K_lower, n_primal):
        self.K_lower, self.n_i, self.my_i = K_lower, max(n_primal, 0), K_lower.shape[0] - max(n_primal, 0)
        self.hint = n_primal

    @property
    def n_leaf(self):
        return self.K_lower.shape[0]

    def K_full(self, b):
        return (self.K_lower + sp.tril(self.K_lower, -1).T).tocsc()

    def oracle_leaf(self, b, **kw):
        s = orc.OracleLdl(self.K_lower.copy(), n_primal=self.hint, **kw)
        s.matrixChanged()
        return s


PIVOT_CUTS = {"model": -1, "all_head": None, "all_tail": 0}      # force_n_head (None: the leaf's dimension)
PIVOT_LEAF_SHAPE = (400, 200)
PIVOT_SMALL_SHAPE = (170, 85)
PIVOT_WANTED_TILE_COLUMNS = (0, 31, 32, 127)
_ALL_CUTS = ("model", "all_head", "all_tail")
# (case, (n_i, my_i), kind of W, block of the generator, cuts).  400 / 200 random W: the model cuts head 344 (singletons: k_head_factor_simple) + tail 256;
# 400 / 200 time-coupled (banded W): fronts; 170 / 85: no tail from the model.  The last three rows are the blocks of the three-block batch two_blocks.
PIVOT_LEAF_TABLE = [(name, PIVOT_LEAF_SHAPE, kind, 0, _ALL_CUTS) for kind in ("random", "time_coupled")
                    for name in ("dead_primal", "dead_dual", "free_primal", "wrong_sign_primal", "wrong_sign_primal_unhinted")] + \
                   [("duplicate_rows", PIVOT_LEAF_SHAPE, "random", 0, _ALL_CUTS), ("duplicate_rows_wrong_sign", PIVOT_LEAF_SHAPE, "random", 0, ("model",)),
                    ("dead_primal", PIVOT_SMALL_SHAPE, "random", 0, ("model",)), ("clean", PIVOT_SMALL_SHAPE, "random", 1, ("model",)),
                    ("duplicate_rows", PIVOT_SMALL_SHAPE, "random", 2, ("model",))]
PIVOT_TWO_BLOCKS = PIVOT_LEAF_TABLE[-3:]


class PivotLeafCase:
    """One leaf block of the case table: K (pa.Csr, lower), its diagonal positions, n_i, my_i, the hint it is factorised with (n_i or -1),
    whether its solves are judged, and the rows (caller's numbering) the construction means to have rejected."""

    def __init__(self, name, K, dpos, n_i, my_i, hint, solve_judged, meant_rows, decoupled=False):
        self.name, self.K, self.dpos, self.n_i, self.my_i, self.hint = name, K, dpos, n_i, my_i, hint
        self.solve_judged, self.meant_rows, self.decoupled = solve_judged, np.sort(np.asarray(meant_rows, dtype=np.int64)), decoupled
        self.n = n_i + my_i
        K.val.setflags(write=False)

    def K_scipy(self):
        return sp.csr_matrix((self.K.val.copy(), self.K.colidx, self.K.rowptr), shape=(self.n, self.n))

    def probe(self, cut):
        f = PIVOT_CUTS[cut]
        return pa.symbolic_probe(self.K, self.hint, force_n_head=self.n if f is None else f, want_perm=True)


def _pivot_base_block(shape, kind, block=0):
    n_i, my_i = shape
    prob = TimeCoupledProblem(5, 3, n_i, my_i, 0, 0, 6) if kind == "time_coupled" else Problem(41, 3, n_i, my_i, 0, 0, 8.0 / n_i, diag_lo=-2.0, diag_hi=2.0)
    blk = prob.blocks[block]
    return blk["W"].to_scipy().tocsr(), blk["diag"].copy()


def _pivot_assemble(W, diag, n_i):
    W = sp.csr_matrix(W)
    W.sort_indices()
    Wp = pa.Csr(W.shape[0], n_i, W.indptr, W.indices, W.data)
    K, dpos = pa.kkt_leaf_assemble(n_i, Wp)
    K.val[dpos] = diag
    return K, dpos


def _pivot_positions(K, hint, n):
    """position in the elimination order of every row, at each of the three cuts"""
    out = {}
    for cut, f in PIVOT_CUTS.items():
        pr = pa.symbolic_probe(K, hint, force_n_head=n if f is None else f, want_perm=True)
        pos = np.empty(n, np.int64)
        pos[pr["perm"]] = np.arange(n)
        out[cut] = (pos, pr["n_head"], pr["m"])
    return out


def pivot_primals_before_their_duals(W, K, n_i, count):
    """primal variables with entries in W whose dual neighbours are all eliminated later at every cut; spread over head and tail of the model's cut
    (the first two of the head, then the tail's, then the head's)"""
    n = n_i + W.shape[0]
    Wc = sp.csc_matrix(W)
    posn = _pivot_positions(K, n_i, n)
    good = [j for j in range(n_i) if Wc.indptr[j + 1] > Wc.indptr[j] and
            all(pos[n_i + r] > pos[j] for pos, _, _ in posn.values() for r in Wc.indices[Wc.indptr[j]:Wc.indptr[j + 1]])]
    pos, n_head, _ = posn["model"]
    head = [j for j in good if pos[j] < n_head]
    tail = [j for j in good if pos[j] >= n_head]
    picked = (head[:2] + tail[:1] + head[2:] + tail[1:])[:count]
    assert len(picked) == count
    return picked


def pivot_leaf_case(name, shape=PIVOT_LEAF_SHAPE, kind="random", cut="model", block=0):
    """The leaf cases of the table (see tests/test_pivot_rule_gpu.py).  duplicate_rows depends on the cut: the pairs that are given equal values are
    those whose later row lands on the wanted positions of that cut's elimination order."""
    key = ("leaf_case", name, shape, kind, cut if name.startswith("duplicate_rows") else None, block)
    if key in _pivot_cache:
        return _pivot_cache[key]
    n_i, my_i = shape
    W, diag = _pivot_base_block(shape, kind, block)
    n = n_i + my_i
    if name in ("dead_primal", "dead_dual", "free_primal", "wrong_sign_primal", "wrong_sign_primal_unhinted", "clean"):
        K, dpos = _pivot_assemble(W, diag, n_i)
        rows = pivot_primals_before_their_duals(W, K, n_i, 3)
        if name == "dead_dual":             # zero diagonal and a row of W of stored zeros: the primal neighbours eliminated earlier contribute exact zeros,
            duals = [0, my_i // 2, my_i - 1]     # the pivot stands as the entry; expected negative, so d' = -repl_abs
            Wc = sp.csr_matrix(W)
            for r in duals:
                Wc.data[Wc.indptr[r]:Wc.indptr[r + 1]] = 0.0
            W = Wc
            rows = [n_i + r for r in duals]
            diag[rows] = 0.0
        elif name == "dead_primal":           # zero diagonal, and every entry of W in these columns a stored zero: decoupled
            Wc = sp.csr_matrix(W)
            Wc.data = np.where(np.isin(Wc.indices, rows), 0.0, Wc.data)        # (the pattern stays: the probe's order is the case's)
            W = Wc
            diag[rows] = 0.0
        elif name == "free_primal":
            diag[rows] = 0.0
        elif name.startswith("wrong_sign_primal"):
            rows = rows[:1]
            diag[rows] = -2.0 ** -3
        else:
            rows = []
        hint = -1 if name.endswith("unhinted") else n_i
        K, dpos = _pivot_assemble(W, diag, n_i)
        case = PivotLeafCase(name, K, dpos, n_i, my_i, hint, name not in ("wrong_sign_primal_unhinted",), [] if name.endswith("unhinted") else rows,
                             decoupled=name in ("dead_primal", "dead_dual"))
    else:
        assert name in ("duplicate_rows", "duplicate_rows_wrong_sign")
        hint = n_i
        W = sp.csr_matrix(W)
        W.sort_indices()
        assert np.all(np.diff(W.indptr) == np.diff(W.indptr)[0])           # (the generator gives every row the same number of entries)
        per = int(np.diff(W.indptr)[0])
        # groups of up to five consecutive rows share the pattern of their first row, values stay different (five and this offset: the later
        # rows of the groups then reach every wanted in-tile column at the model's cut and with all of K in the tail - asserted by the CPU module)
        G, shift = 5, 4
        first = np.array([max(0, (r + shift) - (r + shift) % G - shift) for r in range(my_i)])
        idx = W.indices.reshape(my_i, per)[first].copy()
        W = sp.csr_matrix((W.data.copy(), idx.ravel(), W.indptr.copy()), shape=W.shape)
        diag[n_i:] = 0.0
        K, dpos = _pivot_assemble(W, diag, n_i)
        f = PIVOT_CUTS[cut]
        pr = pa.symbolic_probe(K, hint, force_n_head=n if f is None else f, want_perm=True)
        perm, n_head, m = pr["perm"], pr["n_head"], pr["m"]
        pos = np.empty(n, np.int64)
        pos[perm] = np.arange(n)

        def earlier_mate(r):
            mates = [q for q in np.nonzero(first == first[r])[0] if q != r and pos[n_i + q] < pos[n_i + r]]
            return min(mates, key=lambda q: pos[n_i + q]) if mates else None

        wanted = []          # positions in the elimination order
        dual_head = [k for k in range(n_head) if perm[k] >= n_i and earlier_mate(perm[k] - n_i) is not None]
        if dual_head:        # inside the head: three, spread
            wanted += [dual_head[len(dual_head) // 4], dual_head[len(dual_head) // 2], dual_head[-1]]
        for col in PIVOT_WANTED_TILE_COLUMNS:      # in the tail: the first position at each wanted in-tile column that a later row of a pair can take
            ts = [t for t in range(col, m, DENSE_ROOT_TILE) if perm[n_head + t] >= n_i and earlier_mate(perm[n_head + t] - n_i) is not None]
            if ts:
                wanted.append(n_head + ts[0])
        if m > 128 and perm[n_head + 128] >= n_i and earlier_mate(perm[n_head + 128] - n_i) is not None:
            wanted.append(n_head + 128)            # column 128: the second tile's first
        wanted = sorted(set(wanted))
        data = W.data.reshape(my_i, per).copy()
        rng = np.random.default_rng(7)
        for k in wanted:
            r = perm[k] - n_i
            q = earlier_mate(r)
            if not np.array_equal(data[q], data[r]):
                vals = rng.choice([1.0, -1.0, 0.5, -0.5], per)
                for t in np.nonzero(first == first[r])[0]:
                    if np.array_equal(data[t], data[q]) and t != q:       # (a row already equal to q stays equal)
                        data[t] = vals
                data[q] = vals
                data[r] = vals
            diag[idx[r]] = 2.0 ** rng.integers(-2, 3, per)
        meant = list(perm[wanted])
        if name == "duplicate_rows_wrong_sign":
            # a primal neighbour of the last wanted tail row that lies in the head gets the diagonal -2^-3: replaced by +repl_rel 2^-3, its update
            # of some -1e8 makes the diagonal after the head, not the sum of k_pref_rows, the reference magnitude of that row's pivot
            assert cut == "model" and wanted and wanted[-1] >= n_head > 0
            j = [c for c in idx[perm[wanted[-1]] - n_i] if pos[c] < n_head][0]
            diag[j] = -2.0 ** -3
            meant.append(j)
        W = sp.csr_matrix((data.ravel(), idx.ravel(), W.indptr.copy()), shape=W.shape)
        K2, dpos = _pivot_assemble(W, diag, n_i)
        assert np.array_equal(K2.colidx, K.colidx)
        case = PivotLeafCase(name, K2, dpos, n_i, my_i, hint, False, meant)
        case.wanted_positions, case.cut = np.asarray(wanted), cut
    _pivot_cache[key] = case
    return case


_pivot_cache = {}


def pivot_leaf_reference(case, cut, rule=None, variant="right"):
    """The shared PivotRuleReference of a leaf case at a cut (the right rule: cached)"""
    key = ("leaf_ref", case.name, (case.n_i, case.my_i), id(case), cut, variant)
    if rule is None and key in _pivot_cache:
        return _pivot_cache[key]
    pr = case.probe(cut)
    ref = PivotRuleReference(case.K_scipy(), case.hint, pr["perm"], pr["n_head"], "leaf", rule, variant=variant)
    ref.probe = pr
    if rule is None:
        _pivot_cache[key] = ref
    return ref


def pivot_rhs(n, rejected_rows, seed=3):
    """one Gaussian right-hand side and one unit vector on a rejected row (the first), one per row"""
    B = np.zeros((2, n))
    B[0] = np.random.default_rng(seed).standard_normal(n)
    B[1, rejected_rows[0] if len(rejected_rows) else 0] = 1.0
    return B


def pivot_leaf_judge(case, cut):
    """UnrefinedReference on K' of the case at the cut, right-hand sides of pivot_rhs: the existing predicate with K' in place of K"""
    key = ("leaf_judge", id(case), cut)
    if key not in _pivot_cache:
        ref = pivot_leaf_reference(case, cut)
        j = UnrefinedReference(_OneLeafMatrix(ref.Kp_lower, case.hint), 0, pivot_rhs(case.n, ref.rejected_rows))
        j.rule_ref = ref
        _pivot_cache[key] = j
    return _pivot_cache[key]


# ---- dense root
PIVOT_ROOT_SIZES = (129, 300, 513)
PIVOT_ROOT_DEAD = (0, 31, 32, 96, 127, 128)
PIVOT_ROOT_WRONG_SIGN = ((129, 32), (300, 0), (300, 32), (300, 128), (513, 128))      # (n, p): p a primal row (n_primal = 2 n // 3)


def pivot_root_quasi_definite(n, n_primal, seed):
    """[H A^T; A -G], H and G diagonally dominant with diagonals near 2 n (tests/test_root_single_launch_gpu.py: quasi_definite, no spread)"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n)) * 0.5
    M = M + M.T
    d = np.full(n, float(n))
    d[n_primal:] *= -1
    M[np.arange(n), np.arange(n)] = d
    M[:n_primal, :n_primal] += np.diag(np.abs(M[:n_primal, :n_primal]).sum(axis=1))
    M[n_primal:, n_primal:] -= np.diag(np.abs(M[n_primal:, n_primal:]).sum(axis=1))
    return M


def pivot_root_case(kind, n, p=None):
    """("dead", n): rows and columns PIVOT_ROOT_DEAD (those below n) zeroed; ("wrong_sign", n, p): M_pp = -2^-3, M[p, :p] = 0 and
    M[p+1:n_primal, p] = 0 - row p couples to dual rows only and its pivot stands as the entry.  Returns (M, n_primal, rows meant to be rejected)."""
    n_primal = (2 * n) // 3
    M = pivot_root_quasi_definite(n, n_primal, 50 + n)
    if kind == "dead":
        rows = [i for i in PIVOT_ROOT_DEAD if i < n]
        for i in rows:
            M[i, :] = 0.0
            M[:, i] = 0.0
    else:
        assert p < n_primal
        M[p, :p] = 0.0
        M[:p, p] = 0.0
        M[p + 1:n_primal, p] = 0.0
        M[p, p + 1:n_primal] = 0.0
        M[p, p] = -2.0 ** -3
        rows = [p]
    M.setflags(write=False)
    return M, n_primal, np.asarray(rows)


PIVOT_ROOT_CASES = [("dead", n, None) for n in PIVOT_ROOT_SIZES] + [("wrong_sign", n, p) for n, p in PIVOT_ROOT_WRONG_SIGN]


def pivot_root_reference(case, rule=None, variant="right"):
    """(PivotRuleReference of the case, DenseRootReference of its K' with the right-hand sides of pivot_rhs) - the latter for the right rule only"""
    key = ("root_ref", case, variant)
    if rule is None and key in _pivot_cache:
        return _pivot_cache[key]
    M, n_primal, rows = pivot_root_case(*case)
    ref = PivotRuleReference(sp.csr_matrix(np.tril(M)), n_primal, None, 0, "root", rule, variant=variant)
    ref.M, ref.n_primal, ref.meant_rows = M, n_primal, rows
    judge = None
    if rule is None and variant == "right":
        judge = DenseRootReference(ref.Kp_dense, pivot_rhs(M.shape[0], rows), n_primal, static=True)
    if rule is None:
        _pivot_cache[key] = (ref, judge)
    return ref, judge


# ----------------------------------------------------------------------------------------------------------------------
# solveCompressed judged against a long-double arrowhead reference (tests/test_solve_compressed_reference_cpu.py,
# tests/test_solve_compressed_judged_gpu.py)
# ----------------------------------------------------------------------------------------------------------------------
SOLVE_COMPRESSED_MUTANTS = ("float32_leaves", "block_term_left_out", "border_row_dropped", "root_rhs_entry_off", "x0_entries_swapped", "z0_without_C0_x0")


class ArrowheadSystem:
    """What ArrowheadReference asks of a Problem, TimeCoupledProblem, TwoLinkProblem or GeneralProblem (told apart by its dims): the dimensions, the
    leaf matrices (lower CSR; diag_scale: with their diagonals times that factor, rounded once, as KktSystem.factorize is handed them), the borders
    Br_i^T (S x n_leaf, rows in the reduced order [x0 | y0 | ylink | zlink]) and the constant root parts.  The caller's root vector is
    [x0 | y0 | z0 | ylink | zlink] (S + mz0 entries); red maps the reduced order into it."""

    def __init__(self, prob, diag_scale=1.0):
        self.prob, self.diag_scale = prob, float(diag_scale)
        if hasattr(prob, "dims"):
            self.N, nx, my, mz, self.n0, self.my0, self.mz0, self.myl, self.mzl = prob.dims
            self.n_primal, self.n_leaf = nx, nx + my + mz
            self.root_parts = dict(A0=prob.A0.to_scipy(), F0=prob.F0.to_scipy(), G0=prob.G0.to_scipy(), z_diag_link=prob.z_diag_link)
            self.C0, self.z_diag0 = sp.csr_matrix(prob.C0.to_scipy()), np.asarray(prob.z_diag0, dtype=np.float64)
        else:
            self.N, self.n0, self.my0, self.mz0, self.myl, self.mzl = prob.N, prob.n0, 0, 0, prob.myl, 0
            self.n_primal, self.n_leaf = prob.n_i, prob.n_leaf
            self.root_parts = dict(F0=prob.F0.to_scipy())
            self.C0, self.z_diag0 = sp.csr_matrix((0, self.n0)), np.zeros(0)
        self.S = self.n0 + self.my0 + self.myl + self.mzl
        self.S_full = self.S + self.mz0
        head = self.n0 + self.my0
        self.red = np.concatenate([np.arange(head), np.arange(head + self.mz0, self.S_full)])
        self.z0_rows = np.arange(head, head + self.mz0)
        self.x_diag0 = np.asarray(prob.x_diag0, dtype=np.float64)

    def K_lower(self, b):
        K = self.prob.blocks[b]["K"]
        Kl = sp.csr_matrix((K.val.copy(), K.colidx, K.rowptr), shape=(K.nrows, K.ncols))
        if self.diag_scale != 1.0:
            Kl = sp.csr_matrix(sp.tril(Kl, -1) + sp.diags(self.diag_scale * Kl.diagonal()))
        Kl.sort_indices()
        return Kl

    def Bt(self, b):
        Bt = sp.csr_matrix(self.prob.blocks[b]["Bt"].to_scipy())
        Bt.sort_indices()
        return Bt

    def oracle_leaf(self, b, **kw):
        s = orc.OracleLdl(self.K_lower(b), n_primal=self.n_primal, **kw)
        s.matrixChanged()
        return s

    def finalize(self, SC, with_C0):
        """finalizeKKTdense on SC (S x S, row-major, lower); with_C0 = False: without the eliminated z0 rows' - C0^T diag(z_diag0)^-1 C0"""
        kw = dict(self.root_parts)
        if with_C0 and self.mz0:
            kw.update(C0=self.C0, z_diag=self.z_diag0)
        return orc.finalize_kkt_dense(SC, self.n0, self.my0, self.myl, self.mzl, self.x_diag0, **kw)

    def root_matrix(self):
        """K_0 on the caller's root vector (S + mz0, dense, symmetric): finalizeKKTdense of zeros, and with mz0 > 0 the z0 rows [C0 0 diag(z_diag0) 0 0]
        (z_diag0 = -Omega^-1 is negative as it is handed over: C0 x0 + diag(z_diag0) z0 = b_z0 is the row solveReducedLinkCons eliminates)"""
        K0 = np.tril(self.finalize(np.zeros((self.S, self.S)), with_C0=False))
        K0 = K0 + np.tril(K0, -1).T
        R = np.zeros((self.S_full, self.S_full))
        R[np.ix_(self.red, self.red)] = K0
        if self.mz0:
            C0 = self.C0.toarray()
            R[np.ix_(self.z0_rows, np.arange(self.n0))] = C0
            R[np.ix_(np.arange(self.n0), self.z0_rows)] = C0.T
            R[self.z0_rows, self.z0_rows] = self.z_diag0
        return R


def solve_compressed_fp64(sysm, leaves, Bts, root, b0, bl, mutant=None, block=None):
    """oracle.solve_compressed restated on copies of one right-hand side (b0: S + mz0, bl: N n_leaf), plain FP64, the same operations in the same
    order - mutant = None gives its bits - with one defect out of SOLVE_COMPRESSED_MUTANTS, in block `block` (default N // 2) where it has one:
      float32_leaves       every leaf solution rounded to float32 at the end
      block_term_left_out  the root right-hand side without that block's Br^T z
      border_row_dropped   the same term without the block's last non-empty border row
      root_rhs_entry_off   the largest entry of the root right-hand side (as the root solver is handed it) times 1 + 1e-11
      x0_entries_swapped   the Ltsolve reads x0 with its first and last entry swapped
      z0_without_C0_x0     z0 = b_z0 / z_diag0, the C0 x0 term left out (mz0 > 0)"""
    assert mutant is None or mutant in SOLVE_COMPRESSED_MUTANTS
    n0, my0, mz0, red = sysm.n0, sysm.my0, sysm.mz0, sysm.red
    block = sysm.N // 2 if block is None else block
    b0 = np.array(b0, dtype=np.float64)
    bs = [np.array(v, dtype=np.float64) for v in np.asarray(bl).reshape(sysm.N, -1)]
    for i, (bi, sol, Bt) in enumerate(zip(bs, leaves, Bts)):
        sol.solve(bi)
        if mutant == "block_term_left_out" and i == block:
            continue
        t = Bt @ bi
        if mutant == "border_row_dropped" and i == block:
            t[np.nonzero(np.diff(Bt.indptr) > 0)[0][-1]] = 0.0
        b0[red] -= t
    rhs = b0[red].copy()
    if mz0:
        b3 = b0[n0 + my0:n0 + my0 + mz0] / sysm.z_diag0
        rhs[:n0] -= sysm.C0.T @ b3
    if mutant == "root_rhs_entry_off":
        rhs[np.argmax(np.abs(rhs))] *= 1.0 + 1e-11
    root.solve(rhs)
    b0[red] = rhs
    if mz0:
        x3 = b0[n0 + my0:n0 + my0 + mz0] - (0.0 if mutant == "z0_without_C0_x0" else sysm.C0 @ rhs[:n0])
        b0[n0 + my0:n0 + my0 + mz0] = x3 / sysm.z_diag0
    x0 = b0[red]
    if mutant == "x0_entries_swapped":
        x0[[0, -1]] = x0[[-1, 0]]
    for bi, sol, Bt in zip(bs, leaves, Bts):
        t = Bt.T @ x0
        sol.solve(t)
        bi -= t
    xl = np.concatenate(bs)
    return b0, (xl.astype(np.float32).astype(np.float64) if mutant == "float32_leaves" else xl)


class ArrowheadReference:
    """The whole system solveCompressed solves, A = [[diag(K_i), Br_i], [Br_i^T, K_0]] as one CSR on [x_1 .. x_N | x0 y0 z0 ylink zlink], and a set of
    right-hand sides (row k of B0 and BL):
      X_star  scipy's splu on A, then refinement steps on a long-double x (residual in long double, correction added in long double) until a
              correction is below 2^-58 max|x|, rounded to FP64 once;
      X_ref0  the plain FP64 algorithm of the same kind: oracle.solve_compressed over unrefined oracle leaves and LAPACK's dsytrf / dsytrs on the
              oracle's own FP64 Schur complement (unrefined solves of the border columns, finalizeKKTdense);
    and per right-hand side the ratios of three measures of a solution to the same measure of X_ref0, at least 2^-53 of its scale:
      backward      eta = ||b - A x||inf / (||A||inf ||x||inf + ||b||inf) over the whole system
      root_rows     the same quotient over the root rows alone: ||r_0||inf / (||A_0||inf ||x||inf + ||b_0||inf), A_0 the root rows of A
      forward_root  max|x - x*| over the root part, scale max|x*| there;  forward_leaf: the same over the leaf part.
    A solution of the all-zero right-hand side that is not exactly zero, and anything non-finite, has every ratio inf.  Computed once, read-only."""
    MAX_STEPS = 8

    def __init__(self, sysm, B0, BL):
        import scipy.sparse.linalg as spl
        self.sys = sysm
        N, nl, Sf = sysm.N, sysm.n_leaf, sysm.S_full
        self.n_leaves = N * nl
        self.B0 = np.ascontiguousarray(np.atleast_2d(B0), dtype=np.float64)
        self.BL = np.ascontiguousarray(np.atleast_2d(BL), dtype=np.float64)
        assert self.B0.shape[1] == Sf and self.BL.shape[1] == self.n_leaves and self.B0.shape[0] == self.BL.shape[0]
        self.Bts = [sysm.Bt(b) for b in range(N)]
        E = sp.csr_matrix((np.ones(sysm.S), (sysm.red, np.arange(sysm.S))), shape=(Sf, sysm.S))
        Btf = [sp.csr_matrix(E @ Bt) for Bt in self.Bts]
        Kl = [sysm.K_lower(b) for b in range(N)]
        A = sp.bmat([[sp.block_diag([K + sp.tril(K, -1).T for K in Kl]), sp.vstack([B.T for B in Btf])],
                     [sp.hstack(Btf), sp.csr_matrix(sysm.root_matrix())]], format="csr")
        A.sum_duplicates()
        A.sort_indices()
        assert A.shape == (self.n_leaves + Sf,) * 2 and np.all(np.diff(A.indptr) > 0) and abs(A - A.T).max() == 0.0
        self.A = A
        self._indptr, self._indices, self._data = A.indptr[:-1].copy(), A.indices.copy(), A.data.astype(np.longdouble)
        rowsum = np.asarray(abs(A).sum(axis=1)).ravel()
        self.norm_A, self.norm_A_root = float(rowsum.max()), float(rowsum[self.n_leaves:].max())
        self.B = np.hstack([self.BL, self.B0])
        # x*
        lu = spl.splu(A.tocsc())
        X = lu.solve(self.B.T.copy()).T.astype(np.longdouble)
        self.refinement_steps, self.converged = 0, False
        while self.refinement_steps < self.MAX_STEPS and not self.converged:
            dX = lu.solve(self._residual(X).astype(np.float64).T.copy()).T
            X = X + dX.astype(np.longdouble)
            self.refinement_steps += 1
            self.converged = bool(np.all(np.abs(dX).max(axis=1) <= 2.0 ** -58 * np.abs(X).max(axis=1).astype(np.float64)))
        self.X_star = X.astype(np.float64)
        # x_ref0
        self.leaves0 = [sysm.oracle_leaf(b, refine_steps=0) for b in range(N)]
        self.leaf_inertia = [s.get_inertia() for s in self.leaves0]
        SC = np.zeros((sysm.S, sysm.S))
        for s, Bt in zip(self.leaves0, self.Bts):
            orc.add_term_to_schur_compl_blocked(SC, s, Bt)
        self.SC_ref0 = np.tril(sysm.finalize(SC, with_C0=True))
        self.root0 = orc.DenseRootSolver(sysm.S)
        self.root0.matrixChanged(self.SC_ref0)
        self.root_inertia = self.root0.get_inertia()
        self.X_ref0 = np.empty_like(self.B)
        for k in range(self.B.shape[0]):
            b0, bs = self.B0[k].copy(), [v.copy() for v in self.BL[k].reshape(N, -1)]
            orc.solve_compressed(b0, bs, self.leaves0, self.Bts, self.root0, sysm.n0, sysm.my0, sysm.mz0, sysm.myl, sysm.mzl, C0=sysm.C0, z_diag_reg=sysm.z_diag0)
            self.X_ref0[k] = np.concatenate(bs + [b0])
        self.is_zero_rhs = ~self.B.any(axis=1)
        self.measures_ref0 = self.measures(self.X_ref0[:, self.n_leaves:], self.X_ref0[:, :self.n_leaves])
        nl_ = self.n_leaves
        self.scales = dict(backward=np.ones(len(self.B)), root_rows=np.ones(len(self.B)), forward_root=np.abs(self.X_star[:, nl_:]).max(axis=1),
                           forward_leaf=np.abs(self.X_star[:, :nl_]).max(axis=1))
        for a in [self.B0, self.BL, self.B, self.X_star, self.X_ref0, self.SC_ref0] + list(self.measures_ref0.values()) + list(self.scales.values()):
            a.setflags(write=False)

    def mutant(self, k, which, block=None):
        """(x0, xl) of right-hand side k by X_ref0's algorithm with one defect (solve_compressed_fp64)"""
        return solve_compressed_fp64(self.sys, self.leaves0, self.Bts, self.root0, self.B0[k], self.BL[k], which, block)

    def _residual(self, X, rows=None):
        """B - A X per right-hand side (X: one solution per row, [leaves | root]), formed in long double from the CSR of A"""
        B = self.B if rows is None else self.B[rows]
        return B.astype(np.longdouble) - np.add.reduceat(self._data[None, :] * np.asarray(X, dtype=np.longdouble)[:, self._indices], self._indptr, axis=1)

    def measures(self, X0, XL, k=None):
        """backward, root_rows, forward_root, forward_leaf (see above) of the solutions (X0: root part, XL: leaf part; one per row) of all the
        right-hand sides, or of right-hand side k alone"""
        rows = np.arange(len(self.B)) if k is None else np.array([k])
        X = np.hstack([np.atleast_2d(XL), np.atleast_2d(X0)]).astype(np.float64)
        assert X.shape == (len(rows), self.A.shape[0])
        nl = self.n_leaves
        with np.errstate(all="ignore"):
            R = np.abs(self._residual(X, rows)).astype(np.float64)
            xn = np.abs(X).max(axis=1)
            out = {}
            for name, num, den in (("backward", R.max(axis=1), self.norm_A * xn + np.abs(self.B[rows]).max(axis=1)),
                                   ("root_rows", R[:, nl:].max(axis=1), self.norm_A_root * xn + np.abs(self.B0[rows]).max(axis=1))):
                q = np.where(num == 0.0, 0.0, num / np.where(den > 0.0, den, 1.0))
                out[name] = np.where(np.isfinite(q), q, np.inf)
            for name, sl in (("forward_root", slice(nl, None)), ("forward_leaf", slice(0, nl))):
                q = np.abs(X[:, sl] - self.X_star[rows][:, sl]).max(axis=1)
                out[name] = np.where(np.isfinite(q), q, np.inf)
        bad = ~np.isfinite(X).all(axis=1) | (self.is_zero_rhs[rows] & X.any(axis=1))
        return {name: np.where(bad, np.inf, q) for name, q in out.items()}

    def ratios(self, X0, XL, k=None):
        """the four measures, each over max(the same measure of X_ref0, 2^-53 x its scale): what the margin M bounds"""
        rows = np.arange(len(self.B)) if k is None else np.array([k])
        out = {}
        for name, q in self.measures(X0, XL, k).items():
            den = np.maximum(self.measures_ref0[name][rows], UNIT_ROUNDOFF * self.scales[name][rows])
            with np.errstate(all="ignore"):
                r = np.where(q == 0.0, 0.0, q / np.where(den > 0.0, den, 1.0))
            out[name] = np.where(np.isfinite(r), r, np.inf)
        return out

    def accepts(self, X0, XL, M, k=None):
        """the predicate, per right-hand side: all four ratios within M"""
        assert M <= UNREFINED_M_CAP
        return np.all([r <= M for r in self.ratios(X0, XL, k).values()], axis=0)


# the cases: name -> how the problem is built.  Shapes are the smallest that still select each kernel (see the GPU module's docstring).
ARROWHEAD_RHS = ("gaussian", "gaussian2", "b0_zero", "b_leaf_zero", "unit_b0_last", "zero")
ARROWHEAD_SCHUR_WIDTHS = (1, 127, 128, 129, 257)
ARROWHEAD_CASES = ("small", "dense_tail", "time_coupled") + tuple(f"width{S}" for S in ARROWHEAD_SCHUR_WIDTHS) + \
                  ("hetero129", "general", "general_mz0", "two_link_6", "two_link_30", "small_scaled", "time_coupled_scaled")
ARROWHEAD_WAY2_CASES = ("small", "time_coupled")          # the cases whose followers go way 2 on trust: no mutant may be skipped there
# (case, mutant) that the predicate cannot be asked to reject on every Gaussian right-hand side - at most one per case, none on a way-2 case:
#   width1: one Schur row, x0 has no two entries to swap;
#   two_link_30: 580 linking rows - x_ref0's own forward error is 1e-12 of max|x|, and a root right-hand side off by a relative 1e-11 measures
#   73 and 58 units of x_ref0's backward error on the two Gaussian right-hand sides: rejected on one of them (asserted), not on both
ARROWHEAD_NOT_DISTINGUISHABLE = {"width1": "x0_entries_swapped", "two_link_30": "root_rhs_entry_off"}
ARROWHEAD_GENERAL_DIMS = (3, 400, 160, 80, 20, 6, 0, 9, 5)
ARROWHEAD_SECOND_DIAG_SCALE = 1.3


def _arrowhead_narrow_diagonals(prob, seed):
    # the primal diagonals (leaves and x0) span 1e-2 .. 1e2 instead of the generator's 1e-4 .. 1e4, as in unrefined_batch_problem and schur_problem:
    # over eight decades, with the dual regularisation of 1e-8, the plain FP64 algorithm itself loses five digits of x0 (forward error 1e-12 .. 1e-11
    # of max|x0| on the small and the two-link shapes), and a root right-hand side wrong at a relative 1e-11 passed the predicate at M = 64
    for b, blk in enumerate(prob.blocks, 1):
        blk["diag"][:prob.n_i] = pa.gen_diagonal(seed, b, prob.n_i, -2.0, 2.0)
        blk["K"].val[blk["dpos"]] = blk["diag"]
    prob.x_diag0 = pa.gen_diagonal(seed, 0, prob.n0, -2.0, 2.0)
    return prob


def arrowhead_problem(case):
    """(problem, diag_scale) of a case of ARROWHEAD_CASES; problems are built once and shared"""
    scale = ARROWHEAD_SECOND_DIAG_SCALE if case.endswith("_scaled") else 1.0
    name = case[:-len("_scaled")] if case.endswith("_scaled") else case
    key = ("problem", name)
    if key not in _arrowhead_cache:
        if name == "small":
            prob = _arrowhead_narrow_diagonals(Problem(5, 3, 200, 100, 12, 10, 0.05), 5)
        elif name == "dense_tail":
            prob = _arrowhead_narrow_diagonals(Problem(3, 4, 1000, 500, 100, 100, 0.01), 3)
        elif name == "time_coupled":
            prob = _arrowhead_narrow_diagonals(TimeCoupledProblem(5, 3, 3000, 1500, 10, 8, 6), 5)
        elif name.startswith("width"):
            prob = schur_problem(170, int(name[5:]), 1, "full")
        elif name == "hetero129":
            prob = schur_problem(400, 129, 3, "hetero")
        elif name.startswith("general"):
            from tests.test_general_gpu import GeneralProblem
            dims = list(ARROWHEAD_GENERAL_DIMS)
            dims[6] = 4 if name == "general_mz0" else 0
            prob = GeneralProblem(21, *dims, 0.02)
        else:
            from tests.test_sparse_root_gpu import TwoLinkProblem
            N, n_i, my_i, n0, L = {"two_link_6": (6, 120, 60, 4, 3), "two_link_30": (30, 60, 30, 5, 20)}[name]
            prob = _arrowhead_narrow_diagonals(TwoLinkProblem(77, N, n_i, my_i, n0, L, 5.0 / n_i), 77)
        _arrowhead_cache[key] = prob
    return _arrowhead_cache[key], scale


def arrowhead_rhs(sysm, seed):
    """(B0, BL), one right-hand side per row, in the order of ARROWHEAD_RHS: two Gaussian ones, one with b0 = 0, one with b_leaf = 0 (only the
    border path carries anything in the forward half), e of the last Schur index in b0 alone, and the all-zero one"""
    rng = np.random.default_rng(seed)
    B0, BL = rng.standard_normal((6, sysm.S_full)), rng.standard_normal((6, sysm.N * sysm.n_leaf))
    B0[2] = 0.0
    BL[3] = 0.0
    B0[4], BL[4] = 0.0, 0.0
    B0[4, sysm.S_full - 1] = 1.0
    B0[5], BL[5] = 0.0, 0.0
    return B0, BL


_arrowhead_cache = {}


def arrowhead_reference(case):
    """The shared ArrowheadReference of a case of ARROWHEAD_CASES (.sys.prob: its problem)"""
    if case not in _arrowhead_cache:
        prob, scale = arrowhead_problem(case)
        sysm = ArrowheadSystem(prob, scale)
        _arrowhead_cache[case] = ArrowheadReference(sysm, *arrowhead_rhs(sysm, 4000 + ARROWHEAD_CASES.index(case)))
    return _arrowhead_cache[case]


# ----------------------------------------------------------------------------------------------------------------------
# refinement residual, measure and column choice judged row by row (tests/test_refinement_reference_cpu.py, tests/test_refinement_judged_gpu.py)
# ----------------------------------------------------------------------------------------------------------------------
# The lever: set_values only copies into the device's CSR values and the solve sweeps never read them.  factor() with K1, then values K2 =
# K1 + E: x0 = K1^-1 b, the refinement residual is b - K2 x0 = -E x0 + rounding - a signal of any size in any row - and one correction
# leaves K1 x1 = b - E x0 row by row.
REFINE_FULL_LONG_ROW = 512            # csrc/records.h FULL_LONG_ROW: longer full rows go to k_full_spmv_sub_long (the CPU module reads the header)
REFINE_SIGNAL = 2.0 ** 14             # every row's |(E x*)_i| over noise_b: 256 x UNREFINED_M_CAP
REFINE_COLUMN_GAP = 2.0 ** 20         # eta* of the dirty columns over eta* of the others
REFINE_EPS_WORST, REFINE_EPS_OTHER = 2.0 ** -10, 2.0 ** -13
REFINE_FAINT = 2.0 ** -24             # the part on J of a faint column's xs, relative to a dirty one's


def refine_perturbed_values(K, eps, seed, rows=None, coherent=False):
    """K2's values (CSR order of the lower K): K_ij (1 + s_ij eps), s_ij = +-1 at random, on every stored entry - or on those with row and
    column in `rows` (E confined to J x J) - but the block's largest entries (max|K1_b| is taken at factor() and kept).  coherent: s_ij =
    sign(K_ij), E = eps |K1|: against a positive x no row of E x cancels."""
    val = np.asarray(K.val, dtype=np.float64)
    rng = np.random.default_rng(seed)
    s = np.sign(val) if coherent else rng.choice([-1.0, 1.0], len(val))
    touch = np.abs(val) < np.abs(val).max()
    if rows is not None:
        inJ = np.zeros(K.nrows, bool)
        inJ[rows] = True
        row_of = np.repeat(np.arange(K.nrows), np.diff(K.rowptr))
        touch &= inJ[row_of] & inJ[K.colidx]
    return np.where(touch, val * (1.0 + s * eps), val)


class RefinementReference:
    """One block: K1 (lower CSR, the values that are factorised), K2's values (the ones the refinement sees), right-hand sides (one per row
    of B).  Holds the full symmetric K1, K2 and E = K2 - K1 (exact) in long double; XS = x*, the oracle's twice refined solution of K1 x = b;
    X1S = x1* = x* - K1^-1 E x*; X0_ref, X1_ref, X2_ref: the oracle's unrefined FP64 solve and one / two FP64 corrections against K2
    (refine_fp64).  Everything residual-like is summed in long double, per right-hand side, over every row.  Computed once, read-only."""

    def __init__(self, K, n_primal, val2, B):
        self.K, self.n_primal, self.n = K, n_primal, K.nrows
        self.val1, self.val2 = np.asarray(K.val, dtype=np.float64).copy(), np.asarray(val2, dtype=np.float64).copy()
        nnz = len(self.val1)
        src = sp.csr_matrix((np.arange(1, nnz + 1, dtype=np.float64), K.colidx, K.rowptr), shape=(self.n, self.n))
        full = (src + sp.tril(src, -1).T).tocsr()
        full.sort_indices()
        assert np.all(np.diff(full.indptr) > 0)
        self.indptr, self.indices = full.indptr.copy(), full.indices.copy()
        self.src = full.data.astype(np.int64) - 1                          # the stored entry a full entry reads (the device's fsrc)
        self.row_of = np.repeat(np.arange(self.n), np.diff(self.indptr))
        self.upper = self.indices > self.row_of                            # the copies above the diagonal
        self.row_len = np.diff(self.indptr)
        self.K1 = self.val1[self.src].astype(np.longdouble)
        self.K2 = self.val2[self.src].astype(np.longdouble)
        self.E = self.K2 - self.K1                                         # (exact: neighbours in FP64)
        self.norm_K1 = float(np.add.reduceat(np.abs(self.val1[self.src]), self.indptr[:-1]).max())
        self.amax1 = float(np.abs(self.val1).max())
        assert float(np.abs(self.val2).max()) == self.amax1                # E leaves the largest entry alone
        self.B = np.ascontiguousarray(np.atleast_2d(B), dtype=np.float64)
        Ksp = sp.csr_matrix((self.val1.copy(), K.colidx, K.rowptr), shape=(self.n, self.n))
        self._o0 = orc.OracleLdl(Ksp, n_primal=n_primal, refine_steps=0)
        self._o0.matrixChanged()
        o2 = orc.OracleLdl(Ksp, n_primal=n_primal, refine_steps=2)
        o2.matrixChanged()
        self.inertia = self._o0.get_inertia()
        self.XS = o2.solve(self.B.copy())
        self.EXS = self.matvec(self.E, self.XS)
        self.X1S = self.XS - o2.solve(np.ascontiguousarray(self.EXS.astype(np.float64)))
        self.EX1S = self.matvec(self.E, self.X1S)
        self.X0_ref = self.solve0(self.B)
        self.X1_ref = refine_fp64(self, self.X0_ref, 1)
        self.X2_ref = refine_fp64(self, self.X1_ref, 1)
        for a in (self.B, self.XS, self.X1S, self.X0_ref, self.X1_ref, self.X2_ref, self.val1, self.val2):
            a.setflags(write=False)

    def solve0(self, R):
        """the oracle's unrefined FP64 solve with the factors of K1, one right-hand side per row"""
        return self._o0.solve(np.ascontiguousarray(np.atleast_2d(R), dtype=np.float64).copy())

    def matvec(self, data, X):
        """(A x) per row of X, A the full symmetric matrix with the entries `data` - in the precision of data and X (long double)"""
        X = np.atleast_2d(X).astype(data.dtype)
        return np.add.reduceat(data[None, :] * X[:, self.indices], self.indptr[:-1], axis=1)

    def noise(self, X):
        """noise_b = 2^-53 (||K1_b||inf ||x_b||inf + ||b_b||inf) per right-hand side"""
        return UNIT_ROUNDOFF * (self.norm_K1 * np.abs(np.atleast_2d(X)).max(axis=1) + np.abs(self.B).max(axis=1))

    def _ratios(self, X, target):
        X = np.atleast_2d(X)
        with np.errstate(all="ignore"):
            dev = np.abs(self.matvec(self.K1, X) - target).max(axis=1).astype(np.float64)
            nz = self.noise(X)
            q = np.where(dev == 0.0, 0.0, dev / np.where(nz > 0.0, nz, 1.0))
        return np.where(np.isfinite(q), q, np.inf)

    def ratios_uncorrected(self, X):
        """max_i |K1 x - b|_i / noise_b per right-hand side"""
        return self._ratios(X, self.B.astype(np.longdouble))

    def ratios_once(self, X):
        """max_i |K1 x - (b - E x*)|_i / noise_b"""
        return self._ratios(X, self.B.astype(np.longdouble) - self.EXS)

    def ratios_twice(self, X):
        """max_i |K1 x - (b - E x1*)|_i / noise_b"""
        return self._ratios(X, self.B.astype(np.longdouble) - self.EX1S)

    def uncorrected(self, X, M):
        assert M <= UNREFINED_M_CAP
        return self.ratios_uncorrected(X) <= M

    def corrected_once(self, X, M):
        assert M <= UNREFINED_M_CAP
        return self.ratios_once(X) <= M

    def corrected_twice(self, X, M):
        assert M <= UNREFINED_M_CAP
        return self.ratios_twice(X) <= M

    def signal_over_noise(self, rows=None):
        """min over the rows (all of them, or `rows`) of |(E x*)_i| / noise_b(x*) per right-hand side"""
        sig = np.abs(self.EXS).astype(np.float64)
        if rows is not None:
            sig = sig[:, rows]
        nz = self.noise(self.XS)
        return sig.min(axis=1) / np.where(nz > 0.0, nz, 1.0)

    def target_swap_over_noise(self):
        """what replacing x0 by x* in the target costs, from x0_ref: max_i |E (x0_ref - x*)|_i / noise_b - to be far below 1"""
        cost = np.abs(self.matvec(self.E, self.X0_ref.astype(np.longdouble) - self.XS)).max(axis=1).astype(np.float64)
        nz = self.noise(self.XS)
        return cost / np.where(nz > 0.0, nz, 1.0)

    def measure_parts(self, X, mode):
        """(||r||inf, den, gamma) per right-hand side, r = b - K2 x in long double; den of mode 1: max|K1_b| ||x||inf + ||b||inf, of mode 0:
        ||b||inf; gamma = max_i (nnz_i + 2) 2^-53 (|K2| |x| + |b|)_i - what a row sum in FP64, in any order, can be off by"""
        X = np.atleast_2d(X)
        Bl = self.B.astype(np.longdouble)
        num = np.abs(Bl - self.matvec(self.K2, X)).max(axis=1).astype(np.float64)
        bn = np.abs(self.B).max(axis=1)
        den = self.amax1 * np.abs(X).max(axis=1) + bn if mode == 1 else bn
        gam = ((self.row_len + 2)[None, :] * UNIT_ROUNDOFF * (self.matvec(np.abs(self.K2), np.abs(X)) + np.abs(Bl))).max(axis=1).astype(np.float64)
        return num, den, gam

    def measures(self, X, mode):
        """eta*(x) per right-hand side (0 where the denominator is 0, as the device leaves such a block out)"""
        num, den, _ = self.measure_parts(X, mode)
        return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)


def refine_fp64(ref, X, steps, mutant=None, row=None):
    """Host emulation of the device's refinement in plain FP64 on one block: `steps` times x += solve0(b - K2 x).  mutant (tests/
    test_refinement_reference_cpu.py): "skip_row" - residual row `row` comes out 0; "stale_upper" - the copies above the diagonal still hold
    K1's values; "shift_rows" - the residual lands one row further down; "long_row_missing" - row `row` is never subtracted (r = b there)."""
    X = np.array(np.atleast_2d(X), dtype=np.float64)
    data = ref.val2[ref.src]
    if mutant == "stale_upper":
        data = np.where(ref.upper, ref.val1[ref.src], data)
    A = sp.csr_matrix((data, ref.indices, ref.indptr), shape=(ref.n, ref.n))
    for _ in range(steps):
        R = ref.B - (A @ X.T).T
        if mutant == "skip_row":
            R[:, row] = 0.0
        elif mutant == "shift_rows":
            R = np.roll(R, 1, axis=1)
        elif mutant == "long_row_missing":
            R[:, row] = ref.B[:, row]
        X += ref.solve0(R)
    return X


def refine_measure_fp64(refs, xs, mode, mutant=None):
    """Host emulation of the device's measure over the blocks of a batch (refs[b], right-hand side 0, xs[b] its iterate), plain FP64: the worst
    block of ||r_b|| / den_b.  mutant: "worst_block_dropped", "x_norm_missing" (mode 1 without max|K_b| ||x_b||), "second_largest_row"."""
    q = []
    for ref, x in zip(refs, xs):
        A = sp.csr_matrix((ref.val2[ref.src], ref.indices, ref.indptr), shape=(ref.n, ref.n))
        r = np.sort(np.abs(ref.B[0] - A @ x))
        num = r[-2] if mutant == "second_largest_row" else r[-1]
        bn = np.abs(ref.B[0]).max()
        den = ref.amax1 * np.abs(x).max() + bn if (mode == 1 and mutant != "x_norm_missing") else bn
        q.append(num / den if den > 0.0 else 0.0)
    if mutant == "worst_block_dropped":
        q.remove(max(q))
    return max(q)


def refine_batch_measure(refs, xs, mode):
    """(eta*, slack) of a batch: eta* = max_b ||r_b|| / den_b in long double from xs[b], slack = max_b gamma_b / den_b + 4 2^-53 eta* - the
    device's FP64 row sums are the only rounding source in the norms, the quotient adds a few more roundings (derived, not measured)"""
    eta, slack = 0.0, 0.0
    for ref, x in zip(refs, xs):
        num, den, gam = (float(v[0]) for v in ref.measure_parts(np.asarray(x)[None, :], mode))
        if den > 0.0:
            eta, slack = max(eta, num / den), max(slack, gam / den)
    return eta, slack + 4 * UNIT_ROUNDOFF * eta


def refine_measure_close(dev, refs, xs, mode):
    eta, slack = refine_batch_measure(refs, xs, mode)
    return abs(dev - eta) <= slack


# ---- the cases ----
REFINE_DIAG = (-1.0, 2.0)      # the primal diagonals span 1e-1 .. 1e2 (see refine_block_matrix)


def refine_long_row_leaf(seed=23):
    """(K, n_i, my_i, the long row): primal column 0 sits in 530 of the 560 equality rows, three random entries per row besides, primal
    diagonal within 1e-1 .. 1e2: the full row of column 0 holds 531 entries, above FULL_LONG_ROW"""
    n_i, my_i = 700, 560
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    hub = np.sort(rng.choice(my_i, 530, replace=False))
    for r in range(my_i):
        cs = rng.choice(np.arange(1, n_i), 3, replace=False)
        rows += [r] * 3
        cols += list(cs)
    rows += list(hub)
    cols += [0] * len(hub)
    W = sp.csr_matrix((rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows)), (rows, cols)), shape=(my_i, n_i))
    W.sort_indices()
    K, dpos = pa.kkt_leaf_assemble(n_i, pa.Csr(my_i, n_i, W.indptr, W.indices, W.data))
    K.val[dpos] = np.concatenate([pa.gen_diagonal(seed, 1, n_i, *REFINE_DIAG), -1e-8 * np.ones(my_i)])
    return K, n_i, my_i, 0


# the blocks of the one-right-hand-side batch, in the batch's order: Problem blocks of 127, 256, 257 and 2049 rows, the long-row leaf (third),
# a time-coupled block of 900 rows
REFINE_BATCH_BLOCKS = ("p127", "p256", "long_row", "p257", "tc900", "p2049")
REFINE_BATCH_WORST = (0, 3, 5, 2)        # the block with the large perturbation: first, middle, last, the long-row block
REFINE_BIG_SHAPE = (11000, 5500)         # one time-coupled block of 16 500 rows: absmax_chunks() = 2
_REFINE_RANDOM = {"p127": (85, 42, 0.1), "p256": (171, 85, 0.1), "p257": (171, 86, 0.1), "p2049": (1366, 683, 6.0 / 1366)}


def refine_block_matrix(name):
    """(K, n_primal) of a block of the table (or "big").  Every primal diagonal is gen_diagonal(.., -1, 2), 1e-1 .. 1e2: the factors grow
    like 1 / (smallest primal diagonal), and with 1e-2 the oracle's own unrefined residual stands 7 .. 15 x noise_b on the blocks of 256, 2049
    and on the long-row leaf - `uncorrected` is a statement about the residual's rounding level, and the reference has to pass it at M = 4.
    (The time-coupled blocks: with the generator's default 1e-4 .. 1e4, ||K1||inf = 1e4 lifts noise_b above the signal of 2^-13.)"""
    k = ("matrix", name)
    if k not in _refine_cache:
        if name == "long_row":
            K, n_i, _, _ = refine_long_row_leaf()
        elif name in ("tc900", "big"):
            n_i, my_i = (600, 300) if name == "tc900" else REFINE_BIG_SHAPE
            blk = TimeCoupledProblem(5, 1, n_i, my_i, 0, 0, 6).blocks[0]
            K = blk["K"]
            K.val[blk["dpos"][:n_i]] = pa.gen_diagonal(5, 1, n_i, *REFINE_DIAG)
        else:
            n_i, my_i, rho = _REFINE_RANDOM[name]
            K = Problem(17, 1, n_i, my_i, 0, 0, rho, diag_lo=REFINE_DIAG[0], diag_hi=REFINE_DIAG[1]).blocks[0]["K"]
        K.val.setflags(write=False)
        _refine_cache[k] = (K, n_i)
    return _refine_cache[k]


def refine_generic_xs(n, seed):
    """|xs_i| in [1, 2] with random signs"""
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)


def _refine_rhs(K, xs):
    """b = K1 xs per row of xs, FP64 (any b will do: x* is defined by b)"""
    Ks = sp.csr_matrix((np.asarray(K.val), K.colidx, K.rowptr), shape=(K.nrows, K.nrows))
    Kf = (Ks + sp.tril(Ks, -1).T).tocsr()
    return np.ascontiguousarray((Kf @ np.atleast_2d(xs).T).T)


_refine_cache = {}


def refine_block_reference(name, eps):
    """The shared RefinementReference of a block of the table ("big" too) under E = eps (+-1) K_ij on every stored entry, one right-hand side
    b = K1 xs"""
    k = ("block", name, eps)
    if k not in _refine_cache:
        K, n_i = refine_block_matrix(name)
        seed = 7000 + sum(map(ord, name))
        _refine_cache[k] = RefinementReference(K, n_i, refine_perturbed_values(K, eps, seed), _refine_rhs(K, refine_generic_xs(K.nrows, seed + 1)))
    return _refine_cache[k]


def refine_batch_references(worst):
    """the references of the six blocks, block `worst` perturbed by 2^-10 and the others by 2^-13"""
    return [refine_block_reference(name, REFINE_EPS_WORST if b == worst else REFINE_EPS_OTHER) for b, name in enumerate(REFINE_BATCH_BLOCKS)]


# several right-hand sides on one handle: which columns are dirty.  Column 1 is all zero (but in "all"); the others are clean (xs = 0 on J)
# and, every third of them, faint (xs on J scaled by REFINE_FAINT: below tau, yet telling "corrected" from "left alone" in its rows)
REFINE_MULTI_NRHS = (2, 8, 33, 257)
REFINE_MULTI_SETS = ("all", "none", "one", "mixed", "first_chunk", "second_chunk", "all_entries")


def refine_multi_kinds(nrhs, dirty_set):
    """per column: "dirty", "clean", "faint" or "zero" """
    if dirty_set in ("all", "all_entries"):
        return ["dirty"] * nrhs
    if dirty_set == "none":
        dirty = set()
    elif dirty_set == "one":
        dirty = {0 if nrhs == 2 else nrhs // 2}
    elif dirty_set in ("first_chunk", "second_chunk"):
        assert nrhs == 257
        dirty = {256} if dirty_set == "second_chunk" else {0, 5}
    else:   # the first and last column of a chunk of 32 (one sweep per right-hand side, deterministic panels) and of 256, and a few inside
        dirty = {c for c in (0, 5, 6, 31, 32, 40, 63, 64, 200, 255, 256) if c < nrhs}
    kinds = []
    for c in range(nrhs):
        kinds.append("zero" if c == 1 else "dirty" if c in dirty else "faint" if c % 3 == 0 else "clean")
    return kinds


def refine_multi_problem():
    """unrefined_multi_problem() - the same W, head and tail - with its primal diagonal redrawn within 1e-1 .. 1e2 (refine_block_matrix says
    why; here the default's 1e-4 .. 1e4 also leaves primal rows without a constraint entry whose signal is 40 x noise_b)"""
    k = ("problem", "multi")
    if k not in _refine_cache:
        n_i = 1500
        _refine_cache[k] = Problem(5, 1, n_i, n_i // 2, 4, 4, 6.0 / n_i, diag_lo=REFINE_DIAG[0], diag_hi=REFINE_DIAG[1])
    return _refine_cache[k]


def refine_multi_reference(nrhs, dirty_set):
    """The shared reference of a case: the block of refine_multi_problem(), E = 2^-10 (+-1) K_ij on J x J, J a random half of the rows (on
    every stored entry for "all_entries"), and .kinds, .J, .tau (the geometric mean of the smallest dirty and the largest other eta*, mode 1,
    from X0_ref; without one of the two a factor 2^10 from the other), .eta0"""
    k = ("multi", nrhs, dirty_set)
    if k not in _refine_cache:
        prob = refine_multi_problem()
        K, n = prob.blocks[0]["K"], prob.n_leaf
        rng = np.random.default_rng(900 + nrhs)
        J = np.sort(rng.choice(n, n // 2, replace=False))
        kinds = refine_multi_kinds(nrhs, dirty_set)
        XSgen = np.stack([refine_generic_xs(n, 50 * nrhs + c) for c in range(nrhs)])
        if dirty_set == "all_entries":      # E = eps |K1| against positive xs: with random signs some row of some column always cancels
            XSgen = np.abs(XSgen)           # below 2^14 noise_b (33 columns x 2250 rows: the smallest stood at 3.8e3)
        for c, kind in enumerate(kinds):
            if kind == "zero":
                XSgen[c] = 0.0
            elif kind != "dirty":
                XSgen[c, J] *= 0.0 if kind == "clean" else REFINE_FAINT
        ref = RefinementReference(K, prob.n_i, refine_perturbed_values(K, REFINE_EPS_WORST, 31, None if dirty_set == "all_entries" else J, coherent=dirty_set == "all_entries"),
                                  _refine_rhs(K, XSgen))
        ref.kinds, ref.J = kinds, J
        ref.eta0 = ref.measures(ref.X0_ref, 1)
        d = np.array([kd == "dirty" for kd in kinds])
        lo = ref.eta0[~d].max() if (~d).any() and ref.eta0[~d].max() > 0.0 else None
        hi = ref.eta0[d].min() if d.any() else None
        ref.tau = float(np.sqrt(lo * hi)) if lo and hi else float(hi * 2.0 ** -10) if hi else float(lo * 2.0 ** 10)
        _refine_cache[k] = ref
    return _refine_cache[k]


def refine_multi_fp64(ref, fix, ld, mutant=None):
    """Host emulation of solve(nrhs) with one correction for the columns `fix`, in a flat array of rows of length ld (padding 7.5): x0_ref, then
    x(:, fix[i]) += correction i.  mutant: "neighbour_column" - the corrections land one column further on; "stride_n" - they are added at
    distance n, not ld."""
    nrhs, n = ref.B.shape
    flat = np.full(nrhs * ld, 7.5)
    X = flat.reshape(nrhs, ld)
    X[:, :n] = ref.X0_ref
    A = sp.csr_matrix((ref.val2[ref.src], ref.indices, ref.indptr), shape=(n, n))
    fix = list(fix)
    if fix:
        C = ref.solve0(ref.B[fix] - (A @ ref.X0_ref[fix].T).T)
        for i, c in enumerate(fix):
            if mutant == "neighbour_column":
                c = (c + 1) % nrhs
            off = c * (n if mutant == "stride_n" else ld)
            flat[off:off + n] += C[i]
    return X


def refine_multi_judge(ref, X, M):
    """(ok, ratio) per column of X (nrhs x n): a column whose host measure eta* exceeds tau passes corrected_once at M and fails `uncorrected`
    even at the cap; a faint one the other way round; a clean one passes `uncorrected` (E x* is zero to rounding there and the two targets
    coincide: nothing can fail); the zero column is exact zeros.  ratio: the figure of the predicate that has to pass."""
    assert M <= UNREFINED_M_CAP
    X = np.atleast_2d(X)
    unc, once = ref.ratios_uncorrected(X), ref.ratios_once(X)
    ok, ratio = np.zeros(len(ref.kinds), bool), np.zeros(len(ref.kinds))
    for c, kind in enumerate(ref.kinds):
        if kind == "zero":
            ok[c] = not X[c].any()
        elif ref.eta0[c] > ref.tau:
            ok[c], ratio[c] = once[c] <= M and unc[c] > UNREFINED_M_CAP, once[c]
        else:
            ok[c], ratio[c] = unc[c] <= M and (kind == "clean" or once[c] > UNREFINED_M_CAP), unc[c]
    return ok, ratio
