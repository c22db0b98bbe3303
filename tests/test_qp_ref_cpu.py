"""The numpy restatement of the harness' interior-point loop with a Hessian (tests/qp_ref.py) on the CPU: without a Hessian it walks the
path of oracle.ipm_oracle.solve_blocks, with one it reaches a point that satisfies the optimality conditions of the convex QP (which
are sufficient, so no second solver is needed).  And the C ABI of the QP entries: declared, listed, exported."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.general_lp_gen import random_block_lp
from tests.qp_ref import block_hessians, kkt_check_qp, long_row_case, solve_qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QP_SYMBOLS = ("pips_ipm_create_qp", "pips_ipm_hessian_mult", "pips_hip_kkt_set_root_hessian")


def _random_lp(seed, free_fraction):   # the family of tests/test_native_general_gpu.py
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(2, 5))
    return random_block_lp(100 + seed, nb, int(rng.integers(4, 9)), int(rng.integers(8, 20)), int(rng.integers(2, 6)), int(rng.integers(1, 5)),
                           int(rng.integers(1, 4)), int(rng.integers(1, 4)), free_fraction=free_fraction)


@pytest.mark.parametrize("seed", range(4))
def test_without_a_hessian_the_restatement_walks_the_oracles_path(seed):
    from oracle import ipm_oracle as io
    blocks = _random_lp(seed, 0.0)
    want, got = [], []
    o = io.solve_blocks(blocks, max_iter=100, mutol=1e-9, artol=1e-8, trace=want)
    r = solve_qp(io.assemble(blocks), None, max_iter=100, mutol=1e-9, artol=1e-8, trace=got)
    assert o["status"] == r["status"] == 0
    assert o["iterations"] == r["iterations"] and len(want) == len(got)
    for a, b in zip(want, got):
        assert len(a) == len(b)
        a, b = np.array(a[1:]), np.array(b[1:])
        assert (np.abs(a - b) <= 1e-10 * np.maximum(np.abs(a), 1e-300)).all(), (a, b)


@pytest.mark.parametrize("kind", ["pd", "psd"])
@pytest.mark.parametrize("seed", range(8))
def test_restatement_solves_the_qp(seed, kind):
    from oracle import ipm_oracle as io
    blocks = _random_lp(seed, 0.0)
    _, Q = block_hessians(seed, blocks, kind)
    d = io.assemble(blocks)
    trace = []
    r = solve_qp(d, Q, max_iter=100, mutol=1e-9, artol=1e-8, trace=trace)
    assert r["status"] == 0, r
    kkt_check_qp(d, Q, r, 1e-5)
    assert abs(r["objective"] - r["dual_objective"]) <= 1e-5 * max(1.0, abs(r["objective"]))
    assert all(row[6] == row[7] for row in trace if len(row) == 8)   # one step length


@pytest.mark.parametrize("s", range(2))
def test_restatement_solves_the_dense_root_shape(s):
    from oracle import ipm_oracle as io
    blocks, _, Q = long_row_case(s)
    d = io.assemble(blocks)
    r = solve_qp(d, Q, max_iter=100, mutol=1e-9, artol=1e-8)
    assert r["status"] == 0, r
    kkt_check_qp(d, Q, r, 1e-5)


def test_block_hessians_are_lower_triangular_and_match_the_global_matrix():
    blocks = _random_lp(3, 0.0)
    for kind in ("pd", "psd"):
        hs, Q = block_hessians(3, blocks, kind)
        assert len(hs) == len(blocks) and Q.shape[0] == sum(int(b["n0"] if k == 0 else b["ni"]) for k, b in enumerate(blocks))
        assert abs(Q - Q.T).max() == 0.0
        o = 0
        for k, (h, b) in enumerate(zip(hs, blocks)):
            n = int(b["n0"] if k == 0 else b["ni"])
            assert (h is None) == (kind == "psd" and k % 2 == 1)
            if h is not None:
                rows = np.repeat(np.arange(n), np.diff(h["rowptr"]))
                assert (np.asarray(h["colidx"]) <= rows).all()
                assert np.abs(np.asarray(h["val"]) - np.asarray(Q[o + rows, o + np.asarray(h["colidx"])]).ravel()).max() == 0.0
            o += n
        assert np.linalg.eigvalsh(Q.toarray()).min() > (0.05 if kind == "pd" else -1e-12)


def test_qp_symbols_are_declared_listed_and_exported():
    import pips_ipmpp_amd as pa
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pips_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pips_[a-z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(pa.capi.LIB_PATH)
    for s in QP_SYMBOLS:
        assert s in declared, s
        assert s in pa.capi.SYMBOLS, s
        assert hasattr(lib, s), s
