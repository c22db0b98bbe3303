"""Shared cases and references of the dense root's multi-RHS tests (tests/test_dense_root_multi_reference_cpu.py,
tests/test_dense_root_multi_gpu.py): 70 right-hand sides per case - three interleaved panels of 32, the last with 6 columns.

Matrices: util.dense_root_case_matrix, and the zero_leading_tile matrix of tests/test_root_pivoting_gpu.py (the Bunch-Kaufman case whose pivot
order is not the identity).  Right-hand sides, one per row: default_rng(seed + 123456).standard_normal((70, n)) with the case's seed, then
row 5 zero, row 40 e_0 and row 69 e_{n-1}.  The references are util.DenseRootReference, computed once per case and read-only."""
import numpy as np

from tests import util as u

NRHS = 70
# (n, n_primal, family): one tile with 127 pad rows, the tile edge plus one, two to four tile columns
STATIC_CASES = [(1, 0, "flat"), (33, 22, "flat"), (129, 86, "spread"), (257, 128, "spread"), (385, 256, "spread"), (385, 256, "flat")]
BK_CASES = [(129, 86, "flat"), (385, 256, "spread"), (128, None, "zero_diagonal")]
ZERO_LEADING_TILE = (288, None, "zero_leading_tile")      # n0 = 128, m = 160


def case_id(case):
    return f"n{case[0]}-p{case[1]}-{case[2]}"


def zero_leading_tile_matrix():
    """[[0, A^T], [A, -(C C^T) - 1e-3 I]] with n0 = 128, m = 160 from default_rng(7), drawn as tests/test_root_pivoting_gpu.py draws it"""
    rng = np.random.default_rng(7)
    n0, m = 128, 160
    A = rng.standard_normal((m, n0)) * (rng.random((m, n0)) < 0.2)
    A[rng.permutation(m)[:n0], np.arange(n0)] += 3.0            # full column rank
    H = np.zeros((n0, n0))
    C = rng.standard_normal((m, m)) * 0.1
    return np.block([[H, A.T], [A, -(C @ C.T) - 1e-3 * np.eye(m)]])


def rhs(n, seed):
    B = np.random.default_rng(seed + 123456).standard_normal((NRHS, n))
    B[5] = 0.0
    B[40] = 0.0
    B[40, 0] = 1.0
    B[69] = 0.0
    B[69, n - 1] = 1.0
    return B


def case_matrix(case):
    """(M, seed)"""
    if case == ZERO_LEADING_TILE:
        return zero_leading_tile_matrix(), 7
    return u.dense_root_case_matrix(case)


_cache = {}


def reference(case, static):
    """The shared DenseRootReference of (case, static order or Bunch-Kaufman) with the 70 right-hand sides; .garbage_seed: the seed of the strict
    upper triangle the device is handed, .inertia: what the device must report"""
    key = (case, bool(static))
    if key not in _cache:
        M, seed = case_matrix(case)
        ref = u.DenseRootReference(M, rhs(M.shape[0], seed), case[1], static=static)
        ref.garbage_seed = seed + 900000
        if case[1] is None:
            ev = np.linalg.eigvalsh(ref.M)
            ref.inertia = (int((ev > 0).sum()), int((ev < 0).sum()), 0)
        else:
            ref.inertia = (case[1], case[0] - case[1], 0)
        _cache[key] = ref
    return _cache[key]


def host_matrix(ref):
    """row-major, the lower triangle M's, the strict upper one other numbers"""
    return np.ascontiguousarray(u.dense_root_with_garbage_above(ref.M, ref.garbage_seed))
