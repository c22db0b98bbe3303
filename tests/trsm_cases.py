"""The cases of tests/test_trsm_triangular_gpu.py and the factorisation both of its sides run: in the test process with the triangular
trsm (k_tile_gemm<5>), and - `python -m tests.trsm_cases out.npz` - in a fresh process with PIPS_HIP_TRSM_DENSE=1, the dense product."""
import sys

import numpy as np

from tests.util import Problem, hip_lower_as_rowmajor

TILE = 128

# id: (N, n_i, my_i, n0, myl, rho, tail) - tail = rows of K the dense tail takes (None: all of them, no head)
#   shape A: a sparse head under a tail of 300 rows = three tile columns, the last one padded (44 of 128); about 70 border rows (one
#            tile row: its Schur tile is a diagonal pair ti == tj) and about 200 (two tile rows: the pair (1, 0) as well, both padded)
#   shape B: all of K in the tail (255 rows: two tile columns, the last one row short), no head
CASES = {
    "A_border70": (2, 400, 200, 40, 30, 0.02, 300),
    "A_border200": (2, 400, 200, 110, 90, 0.02, 300),
    "B_all_tail": (2, 170, 85, 40, 30, 0.05, None),
}
# (case, deterministic mode).  Bit-for-bit agreement of two runs needs sums whose order is fixed: deterministic mode, or - B_all_tail in the
# default mode - no head (nothing is added into the tail with atomics) and two blocks (an entry of SC is 0 - v1 - v2 in either order)
RUNS = [(c, True) for c in CASES] + [("B_all_tail", False)]

_problems = {}


def problem(case):
    if case not in _problems:
        N, n_i, my_i, n0, myl, rho, _ = CASES[case]
        _problems[case] = Problem(41, N, n_i, my_i, n0, myl, rho)
    return _problems[case]


def force_n_head(case):
    tail = CASES[case][6]
    return 0 if tail is None else problem(case).n_leaf - tail


def factor_case(case, deterministic):
    """One factorisation with the column launches (the caller's environment holds PIPS_HIP_TAIL_SINGLE=0): SC, and per block the tail
    panel, U = L D, the pivots, the inertia and a solution, all on the host."""
    import torch
    import pips_ipmpp_amd as pa
    prob = problem(case)
    S = prob.S
    bt = pa.LeafBatch(prob.N, S)
    bt.set_deterministic(deterministic)
    for b in range(prob.N):
        bt.set_block(b, prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"])
    bt.set_options(force_n_head=force_n_head(case))
    bt.analyze(2)
    for b in range(prob.N):
        bt.set_values(b, prob.blocks[b]["K"].val)
    SC = torch.zeros(S * S, dtype=torch.float64, device="cuda")
    bt.factor(SC, S)
    bt.sync()
    out = {"SC": hip_lower_as_rowmajor(SC.cpu().numpy(), S), "info_m": np.array(bt.info()["m"])}
    for b in range(prob.N):
        panel, dims = bt.tail_to_host(b, "panel")
        out[f"panel{b}"], out[f"dims{b}"] = panel, np.array(dims)
        out[f"U{b}"] = bt.tail_to_host(b, "U")[0]
        out[f"d{b}"] = bt.tail_to_host(b, "d")[0]
        out[f"inertia{b}"] = np.array(bt.inertia(b))
    rhs = np.random.default_rng(9).standard_normal(prob.N * prob.n_leaf)
    out["rhs"], out["x"] = rhs, bt.solve(rhs.copy())
    bt.close()
    return out


def defined_entries(out, b):
    """What a factorisation writes of block b's three arrays (the rest is whatever the allocation held): the panel on and below its
    diagonal, U in the tiles strictly below the tile diagonal, every pivot."""
    m, m_pad, nb, ldT = (int(v) for v in out[f"dims{b}"])
    r, c = np.arange(ldT)[:, None], np.arange(m_pad)[None, :]
    return {"panel": out[f"panel{b}"][np.broadcast_to(r >= c, (ldT, m_pad))],
            "U": out[f"U{b}"][np.broadcast_to(r[:m_pad] // TILE > c // TILE, (m_pad, m_pad))],
            "d": out[f"d{b}"]}


if __name__ == "__main__":
    res = {}
    for case, det in RUNS:
        for k, v in factor_case(case, det).items():
            res[f"{case}|{int(det)}|{k}"] = v
    np.savez(sys.argv[1], **res)
