"""The compact target of the leaf handles' sparse Schur entries (pips_hip_ldl_factor_schur_sparse / _batch) on the CPU:
pips_schur_target_probe runs the host code the entries bind with (csrc/schurtarget.cpp).  The caller's Schur complement is one triangle in
CSR; the device holds the T distinct positions the blocks' cliques touch, and block b's nb_b x nb_b table maps clique pair (la >= lb) to
the index of its position among those T - (bm[lb], bm[la]) of an upper pattern, (bm[la], bm[lb]) of a lower one.  Everything is rebuilt
here in numpy from the borders' row pointers and the pattern, and the probe has to equal it exactly; the three ways a pattern is refused
are raised the way the entries raise them."""
import numpy as np
import pytest
import scipy.sparse as sp

import pips_ipmpp_amd as pa

S, N0, L = 40, 6, 8          # Schur dimension, shared x0 range, rows of one 2-link pair
ERR_ARG, ERR_STATE = 1, 2


def _borders(seed):
    """5 blocks over 12 leaf rows each: all share x0 (with holes), neighbours b, b + 1 share the L rows of pair b; block 3 has no entry at all"""
    rng = np.random.default_rng(seed)
    n = 12
    Bts = []
    for b in range(5):
        rows = np.zeros(S, bool)
        if b != 3:
            rows[:N0] = rng.random(N0) < 0.8
            for pair in (b - 1, b):
                if 0 <= pair < 4:
                    rows[N0 + pair * L:N0 + (pair + 1) * L] |= rng.random(L) < 0.6
            rows[0] = True
        cnt = np.where(rows, rng.integers(1, 4, S), 0)
        rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        colidx = np.concatenate([np.sort(rng.choice(n, c, replace=False)) for c in cnt] + [np.zeros(0, int)]).astype(np.int32)
        Bts.append(pa.Csr(S, n, rowptr, colidx, rng.standard_normal(len(colidx))))
    Bts[3] = None if seed % 2 else Bts[3]          # "no border" both ways: absent, or S empty rows
    return Bts


def _cols(Bts):
    return [np.zeros(0, int) if Bt is None else np.nonzero(np.diff(Bt.rowptr) > 0)[0] for Bt in Bts]


def _pattern(cols, lower, seed, extra=60):
    """union of the cliques plus extra entries, one triangle, as sorted CSR index arrays"""
    rng = np.random.default_rng(seed + 100)
    m = np.zeros((S, S), bool)
    for bm in cols:
        m[np.ix_(bm, bm)] = True
    m[rng.integers(0, S, extra), rng.integers(0, S, extra)] = True
    m = np.tril(m | m.T) if lower else np.triu(m | m.T)
    sc = sp.csr_matrix(m.astype(np.float64))
    sc.sort_indices()
    return sc.indptr.astype(np.int32), sc.indices.astype(np.int32)


def _expected(cols, rp, ci, lower):
    where = []
    for bm in cols:
        w = np.zeros((len(bm), len(bm)), np.int64)
        for la in range(len(bm)):
            for lb in range(la + 1):
                r, c = (bm[la], bm[lb]) if lower else (bm[lb], bm[la])
                hit = np.nonzero(ci[rp[r]:rp[r + 1]] == c)[0]
                assert len(hit) == 1
                w[la, lb] = rp[r] + hit[0]
        where.append(w)
    pos = np.unique(np.concatenate([w[np.tril_indices(len(w))] for w in where]))
    tabs = [np.tril(np.searchsorted(pos, w)) for w in where]
    return pos, tabs


@pytest.mark.parametrize("lower", [False, True], ids=["upper", "lower"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_probe_equals_the_numpy_rebuild(seed, lower):
    Bts = _borders(seed)
    cols = _cols(Bts)
    assert len(cols[3]) == 0 and min(len(c) for i, c in enumerate(cols) if i != 3) > 3
    assert len(np.intersect1d(cols[0], cols[1])) > 1 and len(np.intersect1d(cols[1][cols[1] >= N0], cols[2][cols[2] >= N0])) > 0
    rp, ci = _pattern(cols, lower, seed)
    nb, pos, tabs = pa.capi.schur_target_probe(Bts, rp, ci, S, lower=lower)
    want_pos, want_tabs = _expected(cols, rp, ci, lower)
    assert list(nb) == [len(c) for c in cols]
    assert np.array_equal(pos, want_pos) and len(pos) < rp[S]           # T: fewer than the pattern holds (the extra entries stay out)
    assert len(pos) < sum(len(c) * (len(c) + 1) // 2 for c in cols)     # shared Schur columns share positions
    for b in range(5):
        assert tabs[b].shape == (nb[b], nb[b])
        assert np.array_equal(np.tril(tabs[b]), want_tabs[b])


@pytest.mark.parametrize("lower", [False, True], ids=["upper", "lower"])
def test_missing_clique_entry_is_named(lower):
    Bts = _borders(0)
    cols = _cols(Bts)
    rp, ci = _pattern(cols, lower, 0)
    bm = cols[2]
    r, c = (bm[4], bm[1]) if lower else (bm[1], bm[4])
    k = rp[r] + int(np.nonzero(ci[rp[r]:rp[r + 1]] == c)[0][0])
    ci2 = np.delete(ci, k)
    rp2 = rp.copy()
    rp2[r + 1:] -= 1
    with pytest.raises(pa.capi.PipsHipError, match=rf"code {ERR_STATE}\).*\({r}, {c}\)"):
        pa.capi.schur_target_probe(Bts, rp2, ci2, S, lower=lower)
    # ... the diagonal counts
    d = cols[0][2]
    k = rp[d] + int(np.nonzero(ci[rp[d]:rp[d + 1]] == d)[0][0])
    rp3 = rp.copy()
    rp3[d + 1:] -= 1
    with pytest.raises(pa.capi.PipsHipError, match=rf"code {ERR_STATE}\).*\({d}, {d}\)"):
        pa.capi.schur_target_probe(Bts, rp3, np.delete(ci, k), S, lower=lower)


def test_descending_consulted_row_and_index_out_of_range():
    Bts = _borders(0)
    cols = _cols(Bts)
    rp, ci = _pattern(cols, False, 0)
    r = next(int(s) for s in cols[1] if rp[s + 1] - rp[s] >= 2)
    bad = ci.copy()
    bad[rp[r]:rp[r] + 2] = bad[rp[r]:rp[r] + 2][::-1]
    with pytest.raises(pa.capi.PipsHipError, match=rf"code {ERR_ARG}\).*row {r} .*does not ascend"):
        pa.capi.schur_target_probe(Bts, rp, bad, S)
    bad = ci.copy()
    bad[rp[r + 1] - 1] = S
    with pytest.raises(pa.capi.PipsHipError, match=rf"code {ERR_ARG}\)"):
        pa.capi.schur_target_probe(Bts, rp, bad, S)
    # a row no block's clique reads may be in any order
    used = np.unique(np.concatenate(cols))
    free = [s for s in range(S) if s not in used and rp[s + 1] - rp[s] >= 2]
    if free:
        ok = ci.copy()
        ok[rp[free[0]]:rp[free[0] + 1]] = ok[rp[free[0]]:rp[free[0] + 1]][::-1]
        nb, pos, _ = pa.capi.schur_target_probe(Bts, rp, ok, S)
        assert np.array_equal(pos, _expected(cols, rp, ci, False)[0])


def test_wrong_S():
    Bts = _borders(0)
    rp, ci = _pattern(_cols(Bts), False, 0)
    for wrong in (S - 1, S + 1):
        with pytest.raises(pa.capi.PipsHipError, match=rf"code {ERR_ARG}\)"):
            pa.capi.schur_target_probe(Bts, rp, ci, wrong)
    with pytest.raises(pa.capi.PipsHipError, match=rf"code {ERR_ARG}\)"):
        pa.capi.schur_target_probe(Bts, rp, ci, 0)
