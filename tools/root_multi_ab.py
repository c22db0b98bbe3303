#!/usr/bin/env python3
"""A/B of the dense root's solve of many right-hand sides on the device entry (pips_hip_dense_ldl_solve_multi_dev): the per-vector sweeps
(PIPS_HIP_MULTI=0: one k_tail_rows_fwd / _bwd pair per right-hand side, L read once per right-hand side) against the default (interleaved
panels of 32 on the matrix pipe from 8 right-hand sides on, L read once per panel).

Static pivot order, a quasi-definite matrix [[H, A^T], [A, -G]] of dimension S built on the device, factorised once.  Per S and nrhs both
forms run in one process on the same handle and the same right-hand sides: --warmup solves of each, then alternating, --repeats times; every
solve is timed with device events around the call.  Prints one line per (S, nrhs, form) - median, min, max, spread (max / min) in ms - the
ratio default / per-vector, and the largest relative residual of either form."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def quasi_definite(S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n_primal = (2 * S) // 3
    m = S - n_primal
    H = torch.diag(1.0 + torch.rand(n_primal, generator=g, device="cuda", dtype=torch.float64))
    R = torch.randn(n_primal, max(1, n_primal // 8), generator=g, device="cuda", dtype=torch.float64)
    H += R @ R.T / R.shape[1]
    A = torch.randn(m, n_primal, generator=g, device="cuda", dtype=torch.float64) * (torch.rand(m, n_primal, generator=g, device="cuda") < 0.3)
    G = torch.diag(1.0 + torch.rand(m, generator=g, device="cuda", dtype=torch.float64))
    M = torch.empty(S, S, device="cuda", dtype=torch.float64)
    M[:n_primal, :n_primal] = H
    M[n_primal:, :n_primal] = A
    M[:n_primal, n_primal:] = A.T
    M[n_primal:, n_primal:] = -G
    return M, n_primal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 8000])
    ap.add_argument("--nrhs", type=int, nargs="+", default=[8, 40, 160])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import pips_ipmpp_amd as pa

    forms = {"per_vector": "0", "default": None}

    def set_form(form):
        if forms[form] is None:
            os.environ.pop("PIPS_HIP_MULTI", None)
        else:
            os.environ["PIPS_HIP_MULTI"] = forms[form]

    print(f"dense root, static order, device entry; {a.repeats} solves each, alternating, after {a.warmup} warm-up of each; device events, ms")
    print("    S  nrhs  form        path slices rows  median     min     max  spread  residual")
    for S in a.sizes:
        M, n_primal = quasi_definite(S, 20261021 + S)
        s = pa.HipDenseLdlSolver(S, n_primal=n_primal)
        s.matrixChanged_dev(M, S)
        assert s.get_inertia() == (n_primal, S - n_primal, 0)
        for nrhs in a.nrhs:
            B = torch.randn(nrhs, S, generator=torch.Generator(device="cuda").manual_seed(nrhs), device="cuda", dtype=torch.float64)
            norm_M = float(M.abs().sum(dim=1).max())

            def solve(form):
                set_form(form)
                X = B.clone()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                s.solve_multi_dev(X, nrhs, S)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1), X

            times, res, info = {f: [] for f in forms}, {}, {}
            for form in forms:
                for _ in range(a.warmup):
                    solve(form)
            for _ in range(a.repeats):
                for form in forms:
                    t, X = solve(form)
                    times[form].append(t)
                    res[form] = float(((B - X @ M).abs().max(dim=1).values / (norm_M * X.abs().max(dim=1).values + B.abs().max(dim=1).values)).max())
                    info[form] = s.info()
            for form in forms:
                t, i = times[form], info[form]
                print(f"{S:5d} {nrhs:5d}  {form:10s}  {i['last_solve_path']:4d} {i['last_solve_slices']:6d} {i['last_solve_rows']:4d}  {statistics.median(t):6.3f}  {min(t):6.3f}  {max(t):6.3f}  "
                      f"{max(t) / min(t):6.3f}  {res[form]:.2e}")
            print(f"{S:5d} {nrhs:5d}  default / per_vector = {statistics.median(times['default']) / statistics.median(times['per_vector']):.3f}", flush=True)
        s.close()
        del M
    os.environ.pop("PIPS_HIP_MULTI", None)


if __name__ == "__main__":
    main()
