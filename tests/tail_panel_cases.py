"""The cases of tests/test_tail_panel_gpu.py and tests/test_tail_panel_plan_cpu.py and the factorisations both sides of the first run: in
the test process group by group (k_tile_panel, the default), and - `python -m tests.tail_panel_cases out.npz` - in a fresh process with
PIPS_HIP_TAIL_PANEL=0, the column launches.  The caller's environment holds PIPS_HIP_TAIL_SINGLE=0 on both sides."""
import sys

import numpy as np

from tests.trsm_cases import TILE, defined_entries   # noqa: F401  (what a factorisation defines of a block's arrays)
from tests.util import Problem, TimeCoupledProblem

# id: (problems, tail) - problems: [(class, seed, N, n_i, my_i, n0, myl, rho or band width)], their blocks form one batch (same n0, myl);
#     tail = rows of K the dense tail takes (None: all of them, no head).  Groups are four tile columns wide.
#   a: all of K in the tail, 750 rows = six tile columns (a full group and one of two columns, the last column padded); 70 border rows =
#      one padded border tile row.  All of K in the tail also gives a tile envelope: the primal tile rows couple to nothing left of their
#      diagonal tile
#   b: a sparse head under a tail of 1100 rows = nine tile columns, three groups, the last a single padded column; 200 border rows
#   c: the same without a border (nb = 0: no border tile rows, no Schur complement)
#   d: banded (time-coupled) blocks, all of K in the tail (900 rows, eight tile columns): a dual tile row starts at the tile column of
#      the primal variables its band reaches - strips start at different columns, in-group tiles without a task
#   f: blocks of different sizes in one batch: six and nine tile columns
CASES = {
    "a_all_tail_750": ([(Problem, 41, 2, 500, 250, 40, 30, 0.03)], None),
    "b_head_tail_1100": ([(Problem, 41, 2, 940, 460, 110, 90, 0.01)], 1100),
    "c_no_border": ([(Problem, 41, 2, 940, 460, 0, 0, 0.01)], 1100),
    "d_banded_envelope": ([(TimeCoupledProblem, 41, 2, 600, 300, 40, 30, 12)], None),
    "f_mixed_sizes": ([(Problem, 41, 1, 500, 250, 40, 30, 0.03), (Problem, 42, 1, 700, 350, 40, 30, 0.02)], None),
}
# (case, deterministic mode).  Two runs agree bit for bit where the order of every sum is fixed: deterministic mode, or - case a in the
# default mode - no head (nothing is added into the tail with atomics) and two blocks (an entry of SC is 0 - v1 - v2 in either order)
RUNS = [(c, True) for c in CASES] + [("a_all_tail_750", False)]

_batches = {}


def batch(case):
    """(blocks, S, force_n_head) - blocks: [(K, n_i, Bt or None)]"""
    if case not in _batches:
        probs, tail = CASES[case]
        blocks, S, n_leaf = [], None, None
        for cls, *args in probs:
            p = cls(*args)
            assert S in (None, p.S)
            S = p.S
            n_leaf = p.n_leaf
            blocks += [(b["K"], p.n_i, b["Bt"] if p.S else None) for b in p.blocks]
        _batches[case] = (blocks, S, 0 if tail is None else n_leaf - tail)
    return _batches[case]


def values(K, rep):
    """the values of factorisation `rep` on one handle: K's own last; before that every entry scaled by its own factor in [0.75, 1.25]
    (signs stay: still quasi-definite)"""
    v = np.asarray(K.val, dtype=np.float64)
    return v if rep == 1 else v * (1.0 + 0.25 * np.sin(np.arange(v.size)))


def scipy_lower(K):
    import scipy.sparse as sp
    return sp.csr_matrix((np.asarray(K.val), K.colidx, K.rowptr), shape=(K.nrows, K.ncols))


def scipy_diag(Kl):
    import scipy.sparse as sp
    return sp.diags(Kl.diagonal())


def first_panel(out, b):
    """the defined entries of block b's tail panel after the first of the two factorisations"""
    _, m_pad, _, ldT = (int(v) for v in out[f"first_dims{b}"])
    r, c = np.arange(ldT)[:, None], np.arange(m_pad)[None, :]
    return out[f"first_panel{b}"][np.broadcast_to(r >= c, (ldT, m_pad))]


def factor_case(case, deterministic):
    """Two factorisations with different values on one handle.  Of the second: SC, and per block the tail panel, U = L D, the pivots, the
    inertia, and a solution; of the first SC and the panels (keys with a leading "first_").  All on the host."""
    import torch
    import pips_ipmpp_amd as pa
    blocks, S, n_head = batch(case)
    N = len(blocks)
    bt = pa.LeafBatch(N, S)
    bt.set_deterministic(deterministic)
    for b, (K, n_i, Bt) in enumerate(blocks):
        if Bt is None:
            bt.set_block(b, K, n_i)
        else:
            bt.set_block(b, K, n_i, Bt)
    bt.set_options(force_n_head=n_head)
    bt.analyze(2)
    bt.set_timing(True)
    out = {}
    for rep in range(2):
        for b, (K, _, _) in enumerate(blocks):
            bt.set_values(b, values(K, rep))
        SC = torch.zeros(S * S, dtype=torch.float64, device="cuda")
        if S:
            bt.factor(SC, S)
        else:
            bt.factor()
        bt.sync()
        pre = "first_" if rep == 0 else ""
        out[pre + "SC"] = np.tril(SC.cpu().numpy().reshape(S, S).T)
        for b in range(N):
            panel, dims = bt.tail_to_host(b, "panel")
            out[f"{pre}panel{b}"], out[f"{pre}dims{b}"] = panel, np.array(dims)
    tm = bt.get_timing()   # which path ran: the launches the second factorisation booked as tail update, diagonal tiles, trsm
    out["tail_launches"] = np.array([tm[k][1] for k in ("tail_update", "tail_diag", "tail_trsm")])
    for b in range(N):
        out[f"U{b}"] = bt.tail_to_host(b, "U")[0]
        out[f"d{b}"] = bt.tail_to_host(b, "d")[0]
        out[f"inertia{b}"] = np.array(bt.inertia(b))
    rhs = np.random.default_rng(9).standard_normal(sum(K.nrows for K, _, _ in blocks))
    out["rhs"], out["x"] = rhs, bt.solve(rhs.copy())
    bt.close()
    return out


if __name__ == "__main__":
    res = {}
    for case, det in RUNS:
        for k, v in factor_case(case, det).items():
            res[f"{case}|{int(det)}|{k}"] = v
    np.savez(sys.argv[1], **res)
