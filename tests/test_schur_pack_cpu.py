"""The tables of the packed blocked solves (Schur mode 2 with the sparse root) on the CPU: pips_schur_pack_probe runs the host code the
engine builds them with at set_sc_tables time.  Right-hand side q of a packed chunk carries, in every block, that block's q-th non-empty border
column, so what matters is the local numbering: ascending in the Schur column id, -1 exactly on the empty columns, nb_b of them per block and
max_b nb_b right-hand sides in all - for a 2-link chain n0 plus two pairs' linking rows, however many blocks there are."""
import numpy as np

import pips_ipmpp_amd as pa
from tests import util as u
from tests.test_sparse_root_gpu import TwoLinkProblem


def _check_tables(Bts, S, nb, nb_max, local):
    """the properties every case shares; returns the column sets"""
    sets = []
    for b, Bt in enumerate(Bts):
        nonempty = np.zeros(S, bool) if Bt is None else np.diff(np.asarray(Bt.rowptr)) > 0
        assert nb[b] == nonempty.sum()
        assert np.array_equal(local[b] < 0, ~nonempty)                            # -1 exactly on the empty rows
        assert np.array_equal(local[b][nonempty], np.arange(nonempty.sum()))      # ascending in s, without gaps
        assert (local[b][~nonempty] == -1).all()
        sets.append(np.nonzero(nonempty)[0])
    assert nb_max == (max(nb) if len(nb) else 0)
    return sets


def test_chain():
    N, n_i, my_i, n0, L = 30, 60, 30, 5, 20
    prob = TwoLinkProblem(77, N, n_i, my_i, n0, L, 5.0 / n_i)
    S = prob.S
    assert S == 585
    Bts = [blk["Bt"] for blk in prob.blocks]
    nb, nb_max, local = pa.capi.schur_pack_probe(Bts, S)
    sets = _check_tables(Bts, S, nb, nb_max, local)
    assert nb_max <= n0 + 2 * L == 45 < S
    # an inner block sees x0 and the rows of its two pairs, an end block those of one pair
    for b in range(N):
        assert set(sets[b]) <= set(range(n0)) | set(range(n0 + max(b - 1, 0) * L, n0 + min(b + 1, N - 1) * L))
    assert nb[0] <= n0 + L and nb[N - 1] <= n0 + L


def test_heterogeneous():
    prob = u.schur_problem(170, 129, 3, "hetero")
    Bts = [blk["Bt"] for blk in prob.blocks]
    nb, nb_max, local = pa.capi.schur_pack_probe(Bts, prob.S)
    sets = _check_tables(Bts, prob.S, nb, nb_max, local)
    assert list(nb) == [129, 64, 65] and nb_max == 129
    # three different column sets, two of them proper subsets of the first, disjoint from each other
    assert set(sets[1]) < set(sets[0]) and set(sets[2]) < set(sets[0]) and not set(sets[1]) & set(sets[2])
    assert np.array_equal(sets[1], np.arange(64)) and np.array_equal(sets[2], np.arange(64, 129))
    assert local[2][64] == 0 and local[2][128] == 64            # the local numbering starts anew in every block


def test_block_without_border():
    prob = u.schur_problem(170, 33, 3, "full")
    S = prob.S
    empty = pa.Csr(S, prob.n_leaf, np.zeros(S + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for Bts in ([prob.blocks[0]["Bt"], None, prob.blocks[2]["Bt"]], [None, prob.blocks[1]["Bt"], empty]):
        nb, nb_max, local = pa.capi.schur_pack_probe(Bts, S)
        _check_tables(Bts, S, nb, nb_max, local)
        assert sorted(nb)[0] == 0 and nb_max == 33
    nb, nb_max, local = pa.capi.schur_pack_probe([None, empty], S)
    assert list(nb) == [0, 0] and nb_max == 0 and (local == -1).all()
