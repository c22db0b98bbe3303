#!/usr/bin/env python3
"""Cost of deterministic mode on the blocked-solve Schur path (Schur mode 2): one work unit (factorize + 4 solveCompressed, as bench.py)
timed with deterministic mode on and off, the same shape and Schur mode.

  --shape configs1   BASELINE configs[1] (64 blocks x 10k vars, S = 2000), mode 2 forced
  --shape chain      time-coupled chain (families.config3_chain) of --blocks blocks x --n vars, S = --schur-dim (few linking rows per
                     pair: the shapes for which the blocked solves are the cheaper route), Schur mode as auto picks it

Every variant: --warmup untimed units, then --repeats timings of --steps units each; the line reports the median, min and max per unit
and the spread (max / min).  One JSON line per variant, then a summary line with the ratio deterministic / default."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build(pa, blocks_data, n0, S, n_i, my_i, mode, deterministic, seed):
    bt = pa.LeafBatch(len(blocks_data), S, device=0)
    bt.set_deterministic(deterministic)
    bt.set_schur_mode(mode)
    vals, diags = [], []
    for i, (b, (W, T, F)) in enumerate(blocks_data):
        K, dpos = pa.kkt_leaf_assemble(n_i, W)
        Bt = pa.border_assemble(n_i, my_i, 0, n0, 0, A=T, F=F)
        diag = np.concatenate([pa.gen_diagonal(seed, b + 1, n_i), -1e-8 * np.ones(my_i)])
        K.val[dpos] = diag
        bt.set_block(i, K, n_i, Bt)
        vals.append(K.val)
        diags.append(diag)
    bt.analyze(16)
    bt.set_refinement_backward_error(2, 1e-15)
    for i in range(len(blocks_data)):
        bt.set_values(i, vals[i])
    return bt, np.concatenate(diags)


def measure(pa, bt, diag_h, n0, myl, F0, seed, warmup, steps, repeats):
    S = n0 + myl
    kkt = pa.KktSystem(bt, n0, 0, myl, 0, F0=F0)
    diag = torch.tensor(diag_h, device="cuda")
    xd0 = torch.tensor(pa.gen_diagonal(seed, 0, n0), device="cuda")
    g = torch.Generator(device="cpu").manual_seed(seed)
    rhs_leaf = torch.randn(diag.numel(), dtype=torch.float64, generator=g).cuda()
    rhs0 = torch.randn(S, dtype=torch.float64, generator=g).cuda()
    b_leaf, b0 = torch.empty_like(rhs_leaf), torch.empty_like(rhs0)

    def unit():
        kkt.factorize(diag, xd0)
        for _ in range(4):
            b_leaf.copy_(rhs_leaf)
            b0.copy_(rhs0)
            kkt.solve_compressed(b0, b_leaf)

    for _ in range(warmup):
        unit()
    torch.cuda.synchronize()
    per_unit = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            unit()
        torch.cuda.synchronize()
        per_unit.append((time.perf_counter() - t0) * 1e3 / steps)
    x = (b0.cpu().numpy().copy(), b_leaf.cpu().numpy().copy())
    kkt.close()
    return per_unit, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["configs1", "chain"], default="configs1")
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--schur-dim", type=int, default=None, help="chain: S = 95 first-stage variables + the linking rows (default: 95 + one row per pair)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261002)
    ap.add_argument("--mode", type=int, default=None, help="Schur mode instead of the shape's (configs1: 2, chain: 0 = auto)")
    ap.add_argument("--variants", default="default,deterministic", help="comma list of default / deterministic (the shape's Schur mode), default_mode1 / deterministic_mode1")
    a = ap.parse_args()
    import pips_ipmpp_amd as pa
    import families

    n_i, my_i = a.n, a.n // 2
    ids = list(range(a.blocks))
    if a.shape == "configs1":
        n0 = myl = 1000
        data = [(b, pa.gen_block(a.seed, b + 1, n_i, my_i, n0, myl, 1e-3)[:3]) for b in ids]
        F0 = pa.gen_root(a.seed, n0, myl)[0]
        mode = 2
    else:
        chain = families.config3_chain(n_i, a.blocks, a.schur_dim or 95 + a.blocks - 1)
        data = list(zip(ids, chain.blocks(0, a.blocks)))
        n0, myl, my_i, F0 = chain.n0, chain.myl, chain.my_i, chain.F0()
        mode = 0
    if a.mode is not None:
        mode = a.mode
    S = n0 + myl
    res = {}
    for v in a.variants.split(","):
        bt, diag = build(pa, data, n0, S, n_i, my_i, 1 if v.endswith("mode1") else mode, v.startswith("deterministic"), a.seed)
        picked = bt.schur_mode()
        per_unit, x = measure(pa, bt, diag, n0, myl, F0, a.seed, a.warmup, a.steps, a.repeats)
        info = bt.info()
        bt.close()
        res[v] = dict(ms=statistics.median(per_unit), x=x)
        print(json.dumps(dict(shape=a.shape, blocks=a.blocks, n=n_i, S=S, variant=v, schur_mode=picked, ms_per_unit_median=round(statistics.median(per_unit), 3),
                              ms_min=round(min(per_unit), 3), ms_max=round(max(per_unit), 3), spread=round(max(per_unit) / min(per_unit), 3),
                              repeats=a.repeats, steps=a.steps, nnzL=info.get("nnzL"))), flush=True)
    for v in res:
        if v != "default" and "default" in res:
            print(json.dumps(dict(variant=v, against="default", x0_rel_diff=float(np.linalg.norm(res[v]["x"][0] - res["default"]["x"][0]) / np.linalg.norm(res["default"]["x"][0])),
                                  x_leaf_rel_diff=float(np.linalg.norm(res[v]["x"][1] - res["default"]["x"][1]) / np.linalg.norm(res["default"]["x"][1])))), flush=True)
    if "default" in res and "deterministic" in res:
        x0d, xld = res["default"]["x"]
        x0, xl = res["deterministic"]["x"]
        print(json.dumps(dict(shape=a.shape, ratio_deterministic_over_default=round(res["deterministic"]["ms"] / res["default"]["ms"], 3),
                              x0_rel_diff=float(np.linalg.norm(x0 - x0d) / np.linalg.norm(x0d)),
                              x_leaf_rel_diff=float(np.linalg.norm(xl - xld) / np.linalg.norm(xld)))), flush=True)


if __name__ == "__main__":
    main()
