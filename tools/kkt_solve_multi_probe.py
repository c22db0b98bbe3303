"""Device time of KktSystem.solve_compressed_multi on the BASELINE configs[1] shape (64 blocks x 10 000 variables, my_i = 5 000, S = 2000), one
factorisation, nrhs in {8, 32, 160}: the panel call against
  (a) a loop of solve_compressed on a handle analysed with PIPS_HIP_AUG_SWEEPS=0 - the same refined algorithm, like for like;
  (b) the default loop, whose followers go by the unrefined sweeps of the augmented factor.
HIP events on the batch's stream (the default stream), two warm-up calls, the median of --reps (20) calls; the right-hand sides are restored
before every call, outside the events.  The border products alone: nr launches of the single-vector kernels (LeafBatch.border_tmult /
border_mult) against one launch of the panel kernels (LeafBatch.border_tmult_panel / border_mult_panel).
usage: kkt_solve_multi_probe.py [--reps 20] [--blocks 64] [--n 10000] [--schur-dim 2000] [nrhs ...]      (prints)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import pips_ipmpp_amd as pa

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=64)
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--schur-dim", type=int, default=2000)
ap.add_argument("nrhs", type=int, nargs="*", default=[8, 32, 160])
a = ap.parse_args()
seed, rho, N, n_i, S = 20261002, 1e-3, a.blocks, a.n, a.schur_dim
my_i, n0, myl = n_i // 2, S // 2, S // 2


def build():
    bt = pa.LeafBatch(N, S, device=0)
    vals, diags = [], []
    for b in range(N):
        W, T, F, c, xs = pa.gen_block(seed, b + 1, n_i, my_i, n0, myl, rho)
        K, dpos = pa.kkt_leaf_assemble(n_i, W)
        diag = np.concatenate([pa.gen_diagonal(seed, b + 1, n_i), -1e-8 * np.ones(my_i)])
        K.val[dpos] = diag
        bt.set_block(b, K, n_i, pa.border_assemble(n_i, my_i, 0, n0, 0, A=T, F=F))
        vals.append(K.val)
        diags.append(diag)
    bt.analyze(16)
    bt.set_refinement_backward_error(2, 1e-15)
    for b in range(N):
        bt.set_values(b, vals[b])
    F0, c0, x0s = pa.gen_root(seed, n0, myl)
    kkt = pa.KktSystem(bt, n0, 0, myl, 0, F0=F0)
    kkt.factorize(torch.tensor(np.concatenate(diags), device="cuda"), torch.tensor(pa.gen_diagonal(seed, 0, n0), device="cuda"))
    bt.sync()
    return bt, kkt


def median_ms(call, restore, reps):
    ts = []
    for rep in range(2 + reps):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if rep >= 2:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def measure(bt, kkt, what, nrhs_list, reps, panel, loop):
    n_total = N * (n_i + my_i)
    out = {}
    for nrhs in nrhs_list:
        g = torch.Generator(device="cuda").manual_seed(nrhs)
        R0 = torch.randn((nrhs, S), dtype=torch.float64, device="cuda", generator=g)
        RL = torch.randn((nrhs, n_total), dtype=torch.float64, device="cuda", generator=g)
        B0, BL = R0.clone(), RL.clone()

        def restore():
            B0.copy_(R0)
            BL.copy_(RL)

        if panel:
            t = median_ms(lambda: kkt.solve_compressed_multi(B0, BL), restore, reps)
            info = kkt.solve_multi_info()
            out[("panel", nrhs)] = t[0]
            print(f"{what}: panel call, {nrhs} rhs: median {t[0]:.2f} ms (min {t[1]:.2f}, max {t[2]:.2f}) = {t[0] / nrhs:.3f} ms per rhs; {info}", flush=True)
            Xp0, XpL = B0.clone(), BL.clone()
        if loop:
            ways = []

            def run_loop():
                del ways[:]
                for q in range(nrhs):
                    kkt.solve_compressed(B0[q], BL[q])
                    ways.append(kkt.last_solve_path())

            t = median_ms(run_loop, restore, reps)
            out[("loop", nrhs)] = t[0]
            print(f"{what}: loop of solve_compressed, {nrhs} rhs: median {t[0]:.2f} ms (min {t[1]:.2f}, max {t[2]:.2f}) = {t[0] / nrhs:.3f} ms per rhs; ways {sorted(set(ways))}",
                  flush=True)
            if panel:
                d0 = float((Xp0 - B0).abs().max() / B0.abs().max())
                dl = float((XpL - BL).abs().max() / BL.abs().max())
                print(f"{what}: panel against loop, {nrhs} rhs: max difference {d0:.1e} of max|x0|, {dl:.1e} of max|x_leaf|", flush=True)
        del R0, RL, B0, BL
    return out


def border_products_alone(bt, nrhs_list, reps):
    n_total = N * (n_i + my_i)
    for nrhs in nrhs_list:
        Z = torch.randn((nrhs, n_total), dtype=torch.float64, device="cuda")
        X0 = torch.randn((nrhs, S), dtype=torch.float64, device="cuda")
        T = torch.zeros((nrhs, S), dtype=torch.float64, device="cuda")
        Wp = torch.zeros((nrhs, n_total), dtype=torch.float64, device="cuda")

        def tm():
            for q in range(nrhs):
                bt.border_tmult(Z[q], T[q], -1.0)

        def mm():
            for q in range(nrhs):
                bt.border_mult(X0[q], Wp[q], 1.0)

        Tp = torch.zeros((S, nrhs), dtype=torch.float64, device="cuda")
        t1 = median_ms(tm, lambda: None, reps)
        t2 = median_ms(mm, lambda: None, reps)
        t3 = median_ms(lambda: bt.border_tmult_panel(Z, Tp, -1.0), lambda: None, reps)
        t4 = median_ms(lambda: bt.border_mult_panel(X0, Wp, 1.0), lambda: None, reps)
        print(f"border products alone, {nrhs} rhs: Br^T z: {nrhs} launches of k_border_tmult {t1[0]:.3f} ms, one k_border_tmult_panel {t3[0]:.3f} ms ({t1[0] / t3[0]:.2f} x); "
              f"Br x0: {nrhs} launches of k_border_mult_rows {t2[0]:.3f} ms, one k_border_mult_panel {t4[0]:.3f} ms ({t2[0] / t4[0]:.2f} x)  [medians of {reps}]", flush=True)
        del Tp
        del Z, X0, T, Wp


print(f"configs[1] shape: {N} blocks x {n_i} variables (my_i = {my_i}), S = {S}; one factorisation; HIP events, 2 warm-up calls, median of {a.reps}", flush=True)
os.environ["PIPS_HIP_AUG_SWEEPS"] = "0"
bt, kkt = build()
ra = measure(bt, kkt, "(a) handle with PIPS_HIP_AUG_SWEEPS=0", a.nrhs, a.reps, panel=True, loop=True)
border_products_alone(bt, a.nrhs, a.reps)
kkt.close()
bt.close()
del os.environ["PIPS_HIP_AUG_SWEEPS"]
bt, kkt = build()
rb = measure(bt, kkt, "(b) default handle", a.nrhs, a.reps, panel=True, loop=True)
kkt.close()
bt.close()
for nrhs in a.nrhs:
    print(f"nrhs {nrhs}: panel {ra[('panel', nrhs)]:.2f} ms; (a) refined loop {ra[('loop', nrhs)]:.2f} ms = {ra[('loop', nrhs)] / ra[('panel', nrhs)]:.2f} x the panel call "
          f"({'faster' if ra[('panel', nrhs)] < ra[('loop', nrhs)] else 'NOT faster'}); (b) default loop {rb[('loop', nrhs)]:.2f} ms = "
          f"{rb[('loop', nrhs)] / rb[('panel', nrhs)]:.2f} x the panel call on that handle ({rb[('panel', nrhs)]:.2f} ms)")
