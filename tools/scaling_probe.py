"""Problem scaling on the configs[3] share: the time-coupled chain (families.py, 256 blocks x 50 000 variables by default) through the
general entry (x >= 0), rows and columns perturbed by seeded factors 10^U(-3, 3), created with and without the geometric-mean +
equilibrium scaler.  Reports creation times, the scaler's report and host waits, nnz and the bytes the extrema sweeps read, and
the IPM time and host waits per iteration, scaled against unscaled.  Kernel times: run it under rocprofv3 --kernel-trace --stats
(k_scale_* rows) with --scaled-only.
   python tools/scaling_probe.py [blocks] [n_i] [ipm iterations] [--scaled-only]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

import families  # noqa: E402
import pips_ipmpp_amd as pa  # noqa: E402


def _d(M):
    M = sp.csr_matrix(M)
    return dict(rows=M.shape[0], cols=M.shape[1], rowptr=M.indptr.astype(np.int32), colidx=M.indices.astype(np.int32), val=M.data)


def problem(N, n_i, seed=20261004, decades=3.0):
    L, n0, bw, nnz_row = 31, 95, 12, 10
    fam, F0, my_i, myl = families.time_coupled_blocks(N, n_i, L, n0, bw, nnz_row, seed)
    rng = np.random.default_rng(seed)
    f = lambda n: 10.0 ** rng.uniform(-decades, decades, size=n)   # noqa: E731
    c0, x0s, cs0, rl = rng.uniform(0.5, 1.5, n0), rng.uniform(0.5, 1.5, n0), f(n0), f(myl)
    F0s = F0.to_scipy()
    blink = F0s @ x0s
    blocks, nnz = [], F0s.nnz
    for b in range(N):
        W, T, F = (m.to_scipy() for m in fam[b])
        c, xs, csb, rb = rng.uniform(0.5, 1.5, n_i), rng.uniform(0.5, 1.5, n_i), f(n_i), f(my_i)
        bb = T @ x0s + W @ xs
        blink = blink + F @ xs
        nnz += W.nnz + T.nnz + F.nnz
        # A' = R A Cs, b' = R b, c' = Cs c (x >= 0 stays x >= 0)
        blocks.append(dict(ni=n_i, mA=my_i, mC=0, A=_d(sp.diags(rb) @ T @ sp.diags(cs0)), B=_d(sp.diags(rb) @ W @ sp.diags(csb)), C=None, D=None,
                           BL=_d(sp.diags(rl) @ F @ sp.diags(csb)), DL=None, c=c * csb, xlow=np.zeros(n_i), xupp=np.zeros(n_i), ixlow=np.ones(n_i),
                           ixupp=np.zeros(n_i), b=rb * bb, clow=np.zeros(0), cupp=np.zeros(0), iclow=np.zeros(0), icupp=np.zeros(0)))
    root = dict(n0=n0, mA=0, mC=0, mBL=myl, mDL=0, A=None, C=None, BL=_d(sp.diags(rl) @ F0s @ sp.diags(cs0)), DL=None, c=c0 * cs0,
                xlow=np.zeros(n0), xupp=np.zeros(n0), ixlow=np.ones(n0), ixupp=np.zeros(n0), b=np.zeros(0), clow=np.zeros(0), cupp=np.zeros(0),
                iclow=np.zeros(0), icupp=np.zeros(0), bL=rl * blink, dlow=np.zeros(0), dupp=np.zeros(0), idlow=np.zeros(0), idupp=np.zeros(0))
    return [root] + blocks, nnz, n0 + N * n_i, myl + N * my_i


def run(blocks, scaler, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ipm = pa.GeneralIpmSolver(blocks, dual_reg=1e-9, scaler=scaler)
    torch.cuda.synchronize()
    t_create = time.perf_counter() - t0
    sc = ipm.scaling()
    out = dict(create_s=t_create, scaling={k: v for k, v in sc.items() if k not in ("col", "row_eq", "row_ineq")})
    if iters > 0:
        t0 = time.perf_counter()
        res = ipm.solve(max_iter=iters, mutol=1e-8, artol=1e-8)
        dt = time.perf_counter() - t0
        s2 = ipm.stats2()
        its = max(res["iterations"], 1)
        out.update(status=res["status"], iterations=res["iterations"], ms_per_iteration=1e3 * dt / its, host_syncs_per_iteration=s2["host_syncs"] / its,
                   rnorm=res["rnorm"], mu=res["mu"])
    ipm.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    N = int(args[0]) if args else 256
    n_i = int(args[1]) if len(args) > 1 else 50000
    iters = int(args[2]) if len(args) > 2 else 8
    t0 = time.perf_counter()
    blocks, nnz, nx, my = problem(N, n_i)
    print(f"shape: {N} blocks x {n_i}, nx {nx}, my {my}, nnz(J) {nnz}; generated and perturbed in {time.perf_counter() - t0:.1f} s", flush=True)
    # one sweep reads the row pointers, the column indices, the values and the gathered factors, and writes one factor per row
    sweep_bytes = nnz * (4 + 8 + 8) + 0.5 * (nx + my) * (4 + 8)
    print(f"bytes per sweep (algorithmic): {sweep_bytes / 1e6:.1f} MB", flush=True)
    runs = {}
    for scaler in ((["geometric_equilibrium"]) if "--scaled-only" in sys.argv else [None, "geometric_equilibrium"]):
        runs[scaler] = r = run(blocks, scaler, iters)
        print(f"scaler {scaler}: {r}", flush=True)
    if None in runs:
        s, u = runs["geometric_equilibrium"], runs[None]
        print(f"creation: scaled {s['create_s']:.2f} s, unscaled {u['create_s']:.2f} s, difference {s['create_s'] - u['create_s']:.2f} s")
        if iters > 0:
            print(f"IPM per iteration: scaled {s['ms_per_iteration']:.1f} ms / {s['host_syncs_per_iteration']:.1f} host syncs, "
                  f"unscaled {u['ms_per_iteration']:.1f} ms / {u['host_syncs_per_iteration']:.1f} host syncs")


if __name__ == "__main__":
    main()
