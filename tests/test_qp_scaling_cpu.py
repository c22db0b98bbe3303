"""Scaling of convex QPs without a GPU: the Ruiz restatement (tests/qp_scaling_ref.py) on a hand-built example and on the badly
scaled twins of the QP family, the host layout pass with factors against the layout of data scaled beforehand (Q' = Cs Q Cs), the
restatement of the interior-point loop on the Ruiz-scaled twins, and the C ABI of the new entry."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import qp_scaling_ref as qs
from tests.qp_ref import block_hessians, solve_qp
from tests.test_qp_ref_cpu import _random_lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["pd", "psd"]
SEEDS = range(8)


@functools.lru_cache(maxsize=None)
def _twin(seed, kind):
    """original blocks / Hessians, the twin's, the twin's J, my and global Q - computed once, shared, left unchanged"""
    blocks = _random_lp(seed, 0.0)
    hs, _ = block_hessians(seed, blocks, kind)
    tb, th, fac = qs.twin(blocks, hs, seed)
    J, my, _ = qs.J_of(tb)
    return blocks, hs, tb, th, J, my, qs.global_hessian(th, tb)


def test_ruiz_on_a_hand_built_example():
    """J = diag(4, 1/4, 16) without Q: one pass gives 1 / sqrt(d) on both sides exactly and |D K D| = 1, a fixed point of the later
    passes.  J = I with Q = diag(16, 0, 0): col_0 = 1/4 after the first pass (Q's entry is the maximum), row_0 follows
    r <- 2 sqrt(r) from 1 towards 4: 4 * 2^(-1/256) after ten passes; the other factors stay 1."""
    J = sp.csr_matrix(np.diag([4.0, 0.25, 16.0]))
    col, re, ri, info = qs.ruiz(J, None, my=2)
    assert np.array_equal(col, [0.5, 2.0, 0.25]) and np.array_equal(re, [0.5, 2.0]) and np.array_equal(ri, [0.25])
    assert np.array_equal(info, [1.0, 1.0, 1.0, 1.0, 1.0, 10.0, 0.0, 2.0])
    one = qs.ruiz(J, None, passes=1, my=2)
    assert np.array_equal(one[0], col) and np.array_equal(one[1], re) and np.array_equal(one[2], ri)
    Q = sp.csr_matrix(np.diag([16.0, 0.0, 0.0]))
    col, re, ri, info = qs.ruiz(sp.identity(3, format="csr"), Q, my=3)
    assert np.array_equal(col, [0.25, 1.0, 1.0]) and np.array_equal(re[1:], [1.0, 1.0]) and ri.size == 0
    assert re[0] == pytest.approx(4.0 * 2.0 ** (-1.0 / 256.0), rel=1e-14)
    # an empty row and an empty column keep their factor
    J = sp.csr_matrix(np.array([[0.0, 0.0, 9.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]]))
    col, re, ri, _ = qs.ruiz(J, None, my=3)
    assert col[0] == 1.0 and col[1] == 1.0 and re[1] == 1.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_ruiz_equilibrates_the_kkt_matrix_of_the_twins(seed, kind):
    """every row and column maximum of |D K D| within [0.9, 1.1] after ten passes (measured: [0.98, 1.00])"""
    _, _, _, _, J, my, Q = _twin(seed, kind)
    col, re, ri, info = qs.ruiz(J, Q, my=my)
    mx = qs.kkt_abs(J, Q, col, np.concatenate([re, ri])).max(axis=1).toarray().ravel()
    mx = mx[mx > 0.0]
    print(f"max |row of D K D| in [{mx.min():.4f}, {mx.max():.4f}]")
    assert mx.min() >= 0.9 and mx.max() <= 1.1
    assert info[0] == 1.0 and info[5] == 10 and info[7] == 2


def _same_layout(a, b):
    import pips_ipmpp_amd as pa
    for k in pa.capi.IPM_LAYOUT_DIMS + ("pairs", "norm"):
        assert a[k] == b[k], k
    for k, _ in pa.capi.IPM_LAYOUT_ARRAYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("eliminate", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_layout_with_factors_is_the_layout_of_the_scaled_data(kind, eliminate):
    """pips_ipm_layout_probe with a Hessian and factors: array for array and bit for bit what it returns for data scaled beforehand
    (J through transform_blocks, Q through scale_hessians) - the leaves' constant K values, the block Hessians, the flat Hessian with
    its diagonal, and a norm that takes max |Q'|."""
    import pips_ipmpp_amd as pa
    from tests import scaling_ref as sr
    _, _, tb, th, J, my, Q = _twin(2, kind)
    col, re, ri, _ = qs.ruiz(J, Q, my=my)
    got = pa.ipm_layout_probe(tb, th, eliminate_z0=eliminate, col=col, row=np.concatenate([re, ri]))
    sh = qs.scale_hessians(th, tb, col)
    want = pa.ipm_layout_probe(sr.transform_blocks(tb, col, re, ri), sh, eliminate_z0=eliminate)
    _same_layout(got, want)
    plain = pa.ipm_layout_probe(tb, th, eliminate_z0=eliminate)
    assert got["has_q"] == 1 and not np.array_equal(got["Q_v"], plain["Q_v"]) and not np.array_equal(got["hq_v"], plain["hq_v"])
    assert np.array_equal(got["Q_ci"], plain["Q_ci"]) and np.array_equal(got["Q_rp"], plain["Q_rp"])
    # the flat copy is exactly symmetric, and the norm sees Q': a Hessian blown up past every other entry decides it
    F = sp.csr_matrix((got["Q_v"], got["Q_ci"], got["Q_rp"]), shape=(got["nx"], got["nx"]))
    assert abs(F - F.T).max() == 0.0
    big = [None if h is None else dict(h, val=(1e12 * np.asarray(h["val"])).tolist()) for h in th]
    gb = pa.ipm_layout_probe(tb, big, eliminate_z0=eliminate, col=col, row=np.concatenate([re, ri]))
    assert gb["norm"] == np.abs(gb["hq_v"]).max() > got["norm"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_solves_the_ruiz_scaled_twins(seed, kind):
    """the precondition of the device solve test, on the restatement alone: status 0 and the original's objective within 1e-8 relative
    (measured: at most 6.4e-10; 9-17 iterations against 9-16 on the originals, each within two of its original's)"""
    from oracle import ipm_oracle as io
    from tests import scaling_ref as sr
    blocks, hs, tb, th, J, my, Q = _twin(seed, kind)
    ref = solve_qp(io.assemble(blocks), qs.global_hessian(hs, blocks), max_iter=100, mutol=1e-9, artol=1e-8)
    assert ref["status"] == 0
    col, re, ri, _ = qs.ruiz(J, Q, my=my)
    sb, sh = sr.transform_blocks(tb, col, re, ri), qs.scale_hessians(th, tb, col)
    r = solve_qp(io.assemble(sb), qs.global_hessian(sh, sb), max_iter=100, mutol=1e-9, artol=1e-8)
    f = ref["objective"]
    print(f"iterations {r['iterations']} (original {ref['iterations']}), objective {f:.6g}, relative error {abs(r['objective'] - f) / abs(f):.2e}")
    assert r["status"] == 0, r
    assert abs(r["objective"] - f) <= 1e-8 * abs(f)


def test_ruiz_constant_and_the_scaled_qp_entry_of_the_c_abi():
    import pips_ipmpp_amd as pa
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert pa.capi.PIPS_SCALER_RUIZ == 5 == qs.RUIZ and re.search(r"PIPS_SCALER_RUIZ\s*=\s*5\b", hdr)
    assert pa.capi.SCALERS["ruiz"] == 5
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "pips_ipm_create_qp_scaled" in set(re.findall(r"\b(pips_[a-z0-9_]+)\s*\(", txt))
    assert "pips_ipm_create_qp_scaled" in pa.capi.SYMBOLS
    assert hasattr(ctypes.CDLL(pa.capi.LIB_PATH), "pips_ipm_create_qp_scaled")
