#!/usr/bin/env python3
"""A/B of the leaf factorisation with the sparse root: Schur mode 1 (augmented partial factorisation into the value array) against mode 2
(blocked solves packed by block-local column), on the time-coupled family of families.py (default: the configs[3] share, 256 blocks x 50 000).

Both handles live in one process on the same blocks; after --warmup factorisations of each they alternate, --repeats times, and every
factorisation is timed with device events (pips_hip_batch_get_timing, "total" and its "schur" part).  Prints one line per mode - median, min,
max, spread (max / min) in ms - with packed_schur_rhs and the number of distinct non-empty Schur columns, then the ratio mode 2 / mode 1 and
the largest relative difference of the two value arrays."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--chain-blocks", type=int, default=None, help="blocks of the whole chain (default: configs[3], 2048)")
    ap.add_argument("--schur-dim", type=int, default=None, help="Schur dimension of the whole chain (default: configs[3], 8000)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261002)
    a = ap.parse_args()
    import pips_ipmpp_amd as pa
    import families

    t_start = time.perf_counter()

    def say(msg):
        print(f"[{time.perf_counter() - t_start:7.1f} s] {msg}", flush=True)

    whole = families.config3_chain(a.n, a.chain_blocks, a.schur_dim)
    chain = whole.prefix(a.blocks)
    data = chain.blocks(0, a.blocks)
    n0, myl, my_i, F0 = chain.n0, chain.myl, chain.my_i, chain.F0()
    S = n0 + myl
    cols = [chain.border_columns(b, data[b][1]) for b in range(a.blocks)]
    distinct = len(set(int(c) for cs in cols for c in cs))
    say(f"chain of {a.blocks} blocks x {a.n}: S = {S}, n0 = {n0}, {distinct} distinct non-empty Schur columns, max_b nb_b = {max(len(c) for c in cols)}")
    handles = {}
    vals, diags = [], []
    for b, (W, T, F) in enumerate(data):
        K, dpos = pa.kkt_leaf_assemble(a.n, W)
        diag = np.concatenate([pa.gen_diagonal(a.seed, b + 1, a.n), -1e-8 * np.ones(my_i)])
        K.val[dpos] = diag
        vals.append((K, pa.border_assemble(a.n, my_i, 0, n0, 0, A=T, F=F)))
        diags.append(diag)
    diag = torch.tensor(np.concatenate(diags), device="cuda")
    xd0 = torch.tensor(pa.gen_diagonal(a.seed, 0, n0), device="cuda")
    for mode in (1, 2):
        bt = pa.LeafBatch(a.blocks, S, device=0)
        bt.set_schur_mode(mode)
        for b, (K, Bt) in enumerate(vals):
            bt.set_block(b, K, a.n, Bt)
        bt.analyze(16)
        for b, (K, _) in enumerate(vals):
            bt.set_values(b, K.val)
        bt.set_timing(True)
        kkt = pa.KktSystem(bt, n0, 0, myl, 0, F0=F0, sparse_root=True, all_block_cols=cols)
        assert bt.schur_mode() == mode
        handles[mode] = (bt, kkt)
        say(f"mode {mode} analysed: packed_schur_rhs = {bt.info()['packed_schur_rhs']}, nnzL = {bt.info()['nnzL']}")

    def factor(mode):
        bt, kkt = handles[mode]
        kkt.factorize(diag, xd0)
        bt.sync()
        tm = bt.get_timing()
        return tm["total"][0], tm["schur"][0]

    for mode in (1, 2):
        for _ in range(a.warmup):
            factor(mode)
        say(f"mode {mode} warmed up")
    times = {1: [], 2: []}
    for _ in range(a.repeats):
        for mode in (1, 2):
            times[mode].append(factor(mode))
    sc = {mode: handles[mode][1].schur_sparse_to_host().data for mode in (1, 2)}
    print(f"leaf factorisation, sparse root, {a.blocks} blocks x {a.n}, S = {S}; {a.repeats} factorisations each, alternating, after {a.warmup} warm-up; device events, ms")
    print("mode  packed_schur_rhs  distinct_columns  median     min     max  spread  schur_phase_median")
    for mode in (1, 2):
        tot = [t for t, _ in times[mode]]
        print(f"{mode:4d}  {handles[mode][0].info()['packed_schur_rhs']:16d}  {distinct:16d}  {statistics.median(tot):6.2f}  {min(tot):6.2f}  {max(tot):6.2f}  "
              f"{max(tot) / min(tot):6.3f}  {statistics.median([s for _, s in times[mode]]):18.2f}")
    m1, m2 = (statistics.median([t for t, _ in times[m]]) for m in (1, 2))
    print(f"mode 2 / mode 1 = {m2 / m1:.3f}; value arrays differ by {np.abs(sc[1] - sc[2]).max() / np.abs(sc[1]).max():.2e} of the largest entry")
    for bt, kkt in handles.values():
        kkt.close()
        bt.close()


if __name__ == "__main__":
    main()
