"""The column sets of the solve_compressed_multi tests (tests/test_solve_multi_reference_cpu.py, tests/test_solve_multi_judged_gpu.py,
tests/test_solve_multi_two_rank_gpu.py): any number of right-hand sides of an arrowhead case out of the six of util.arrowhead_reference.

    column j = 2^((j // 6) mod 11) x (row j mod 6 of util.arrowhead_rhs(sysm, seed)),    seed = the one util.arrowhead_reference uses

Scaling by a power of two commutes with every FP64 and long-double operation of the reference (no number here comes near the ends of the
exponent range), so x* and x_ref0 of column j are the scaled ones of its base column and every ratio of util.ArrowheadReference is the base
column's: a column is judged by scaling it back - exactly - and asking the shared reference.  The reference of 257 columns costs six solves,
the mutant proofs of tests/test_solve_compressed_reference_cpu.py carry over to every column (the CPU module shows it on twelve), neighbouring
columns differ in base and mostly in scale - columns that leak into each other show - and every sixth column is the all-zero right-hand side,
which must come back as exact zeros."""
import numpy as np

from tests import util as u

N_BASES = len(u.ARROWHEAD_RHS)
N_SCALES = 11
# twelve columns spread over 257: every base twice - two sets of six in the order of the bases - the scales 0 .. 10, both ends
SPREAD = (0, 7, 80, 21, 94, 35, 168, 43, 182, 57, 256, 131)
WIDEST = 257


def base(j):
    return j % N_BASES


def scale(j):
    return 2.0 ** ((j // N_BASES) % N_SCALES)


def seed(case):
    return 4000 + u.ARROWHEAD_CASES.index(case)


def columns(ref, nrhs, first=0):
    """(B0, BL): columns first .. first + nrhs - 1 of the set of ref's case, one per row"""
    j = np.arange(first, first + nrhs)
    s = np.array([scale(int(v)) for v in j])[:, None]
    return s * ref.B0[j % N_BASES], s * ref.BL[j % N_BASES]


def scaled(ref, X, j):
    """row base(j) of an array of the reference (X_star, X_ref0: [leaves | root]) as column j has it"""
    return scale(j) * X[base(j)]


def ratios(ref, X0, XL, first=0):
    """the four ratios of util.ArrowheadReference per column: X0 / XL hold the solutions of columns first .. (one per row)"""
    out = {}
    for i in range(len(X0)):
        j = first + i
        r = ref.ratios(X0[i] / scale(j), XL[i] / scale(j), base(j))
        for name, v in r.items():
            out.setdefault(name, []).append(float(v[0]))
    return {name: np.array(v) for name, v in out.items()}


def accepts(ref, X0, XL, M, first=0):
    """the predicate per column: all four ratios within M; the all-zero columns exact zeros (their ratios are inf otherwise)"""
    assert M <= u.UNREFINED_M_CAP
    return np.all([r <= M for r in ratios(ref, X0, XL, first).values()], axis=0)
