"""Problem scaling without a GPU: the numpy restatement of the reference's scalers (tests/scaling_ref.py) on hand-built matrices,
the gmspips scaler words and the PIPS_SCALER_* constants of the C ABI."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import scaling_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand_badly_scaled(seed, m=30, n=40):
    rng = np.random.default_rng(seed)
    J = sp.random(m, n, density=0.15, random_state=np.random.RandomState(seed), format="csr")
    J.data = rng.standard_normal(J.nnz)
    return sp.csr_matrix(sp.diags(10.0 ** rng.uniform(-4, 4, m)) @ J @ sp.diags(10.0 ** rng.uniform(-4, 4, n)))


@pytest.mark.parametrize("seed", range(4))
def test_equilibrium_leaves_every_row_and_column_max_at_most_two(seed):
    """EquilibriumScaler.C:91 asserts A->inf_norm() <= 2 and C->inf_norm() <= 2 after scaling; so does geometric + equilibrium"""
    J = _rand_badly_scaled(seed)
    for kind in (sr.EQUILIBRIUM, sr.GEOMETRIC_EQUILIBRIUM):
        col, re, ri, info = sr.scale(J, 12, kind)
        S = sr.scaled_matrix(J, col, np.concatenate([re, ri]))
        assert info[0] == 1.0
        assert np.abs(S).max() <= 2.0
        assert np.abs(S).max(axis=1).toarray().max() <= 2.0 and np.abs(S).max(axis=0).toarray().max() <= 2.0
        assert info[3] < info[1] and info[4] < info[2]


def test_geometric_declines_a_matrix_whose_ratios_are_good_enough():
    """ratio <= goodEnough = 500 in both directions: no geometric scaling, factors of 1, nothing applied (GeometricMeanScaler.C:106-114)"""
    J = sp.csr_matrix(np.array([[1.0, 2.0, 0.0], [0.0, 4.0, 100.0], [3.0, 0.0, 0.5]]))
    col, re, ri, info = sr.scale(J, 1, sr.GEOMETRIC)
    assert info[0] == 0.0 and info[5] == 0 and info[6] == 0.0
    assert (col == 1.0).all() and (re == 1.0).all() and (ri == 1.0).all()
    assert info[1] <= 500 and info[2] <= 500
    # with equilibrium after it the matrix is still equilibrated
    col, re, ri, info = sr.scale(J, 1, sr.GEOMETRIC_EQUILIBRIUM)
    assert info[0] == 1.0 and info[6] == 0.0


def test_diagonal_matrix_spread_over_twelve_decades_comes_back_to_unit_ratio():
    d = 10.0 ** np.linspace(-6, 6, 9)
    J = sp.csr_matrix(sp.diags(d) @ sp.csr_matrix(np.eye(9)))
    J = sp.vstack([J, sp.csr_matrix(np.diag([1e-6, 1e6, 1.0]) @ np.eye(3, 9, 3) + np.eye(3, 9) * 0)]).tocsr()
    J.eliminate_zeros()
    for kind in (sr.GEOMETRIC, sr.GEOMETRIC_EQUILIBRIUM, sr.EQUILIBRIUM):
        col, re, ri, info = sr.scale(J, 9, kind)
        assert info[0] == 1.0
        S = sr.scaled_matrix(J, col, np.concatenate([re, ri]))
        assert info[3] == pytest.approx(1.0, rel=1e-12) and info[4] == pytest.approx(1.0, rel=1e-12), (kind, info)
        assert np.allclose(np.abs(S.data), np.abs(S.data)[0], rtol=1e-12)


def test_empty_rows_and_columns_get_a_factor_of_one():
    """safe_invert(1.0): an empty row's max is 0 (its min stays DBL_MAX, their product 0)"""
    J = sp.csr_matrix(np.array([[1e-3, 0.0, 1e4, 0.0], [0.0, 0.0, 0.0, 0.0], [2.0, 0.0, 1e-5, 0.0]]))
    for kind in (sr.EQUILIBRIUM, sr.GEOMETRIC, sr.GEOMETRIC_EQUILIBRIUM):
        col, re, ri, info = sr.scale(J, 2, kind)
        assert re[1] == 1.0 and col[1] == 1.0 and col[3] == 1.0


def test_gmspips_scaler_words():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gmspips
    finally:
        sys.path.pop(0)
    a = gmspips.parse_args(["3", "stem"])
    assert (a["nblocks"], a["stem"], a["mutol"], a["artol"], a["scaler"]) == (3, "stem", 1e-6, 1e-4, None)
    for word, name in (("scale", "equilibrium"), ("scaleEqui", "equilibrium"), ("scaleGeo", "geometric"),
                       ("scaleGeoEqui", "geometric_equilibrium"), ("scaleCurtisReid", "curtis_reid")):
        assert gmspips.parse_args(["2", "s", word])["scaler"] == name
    a = gmspips.parse_args(["4", "dir/stem", "1e-8", "scaleGeo", "1e-7", "presolve"])
    assert (a["mutol"], a["artol"], a["scaler"], a["ignored"]) == (1e-8, 1e-7, "geometric", ["presolve"])
    with pytest.raises(ValueError):
        gmspips.parse_args(["4"])


def test_scaler_constants_of_the_c_abi():
    import re
    import pips_ipmpp_amd as pa
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    for name, want in (("NONE", 0), ("EQUILIBRIUM", 1), ("GEOMETRIC_MEAN", 2), ("GEOMETRIC_MEAN_EQUILIBRIUM", 3), ("CURTIS_REID", 4)):
        assert getattr(pa.capi, "PIPS_SCALER_" + name) == want
        assert re.search(r"PIPS_SCALER_%s\s*=\s*%d\b" % (name, want), hdr)
    assert pa.capi.SCALERS["geometric"] == pa.capi.PIPS_SCALER_GEOMETRIC_MEAN
    assert "pips_ipm_create_general_scaled" in pa.capi.SYMBOLS and "pips_ipm_get_scaling" in pa.capi.SYMBOLS


def test_unknown_scaler_name_raises_before_any_device_work():
    import pips_ipmpp_amd as pa
    with pytest.raises(pa.capi.PipsHipError):
        pa.GeneralIpmSolver([dict()], scaler="powers_of_two")
