"""Cost of the Hessian product in the operator of the outer solve: one Ipm::kmult (HIP events, median of 20 after a warm-up) on the
time-coupled family - by default the configs[3] share, 256 blocks x 50 000 variables - as an LP handle, as a QP handle with a
tridiagonal Hessian (2 on the diagonal, -1 beside it) on the root and on every block, and with --cross K as that QP handle with a
sparse cross Hessian R_i of K entries per row between x0 and every block (pips_ipm_create_qp_cross).
    python tools/qp_operator_probe.py [--blocks 256] [--n 50000] [--cross 2] [--out profiles/qp_operator.txt]
Builds tools/libqp_kmult_probe.so from tools/qp_operator_probe.hip on first use (hipcc, gfx950)."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def probe_library():
    src, so = os.path.join(ROOT, "tools", "qp_operator_probe.hip"), os.path.join(ROOT, "tools", "libqp_kmult_probe.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(os.path.join(ROOT, "pips-ipmpp_amd", "csrc", "harness.hip"))):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "pips-ipmpp_amd", "csrc"), "--offload-arch=gfx950", "-munsafe-fp-atomics", "-Wno-inline-asm",
                               src, "-o", so])
    return C.CDLL(so)


def general_blocks(chain, N, seed):
    """the share as block dicts of the general entry: x >= 0, equality rows only (what bench.py's ipm_end_to_end solves)"""
    rng = np.random.default_rng(seed)
    F0 = chain.F0()
    n0, myl, my_i = chain.n0, chain.myl, chain.my_i
    z = np.zeros(0)
    x0s = rng.uniform(0.5, 1.5, n0)
    blink = F0.to_scipy() @ x0s
    out = [None]
    for W, T, F in chain.blocks(0, N):
        n = W.ncols
        xs = rng.uniform(0.5, 1.5, n)
        blink = blink + F.to_scipy() @ xs
        out.append(dict(ni=n, mA=my_i, mC=0, mBL=myl, mDL=0, A=T, B=W, C=None, D=None, BL=F, DL=None, c=rng.uniform(0.5, 1.5, n),
                        xlow=np.zeros(n), xupp=np.zeros(n), ixlow=np.ones(n), ixupp=np.zeros(n), b=T.to_scipy() @ x0s + W.to_scipy() @ xs,
                        clow=z, cupp=z, iclow=z, icupp=z))
    out[0] = dict(n0=n0, mA=0, mC=0, mBL=myl, mDL=0, A=None, C=None, BL=F0, DL=None, c=rng.uniform(0.5, 1.5, n0), xlow=np.zeros(n0),
                  xupp=np.zeros(n0), ixlow=np.ones(n0), ixupp=np.zeros(n0), b=z, clow=z, cupp=z, iclow=z, icupp=z, bL=blink, dlow=z, dupp=z,
                  idlow=z, idupp=z)
    return out


def tridiagonal(n):
    rowptr = np.concatenate([[0, 1], 1 + 2 * np.arange(1, n)]).astype(np.int32)
    colidx = np.empty(2 * n - 1, np.int32)
    val = np.empty(2 * n - 1)
    colidx[0], val[0] = 0, 2.0
    colidx[1::2], colidx[2::2] = np.arange(0, n - 1), np.arange(1, n)
    val[1::2], val[2::2] = -1.0, 2.0
    return dict(rows=n, cols=n, rowptr=rowptr, colidx=colidx, val=val)


def sparse_cross(n, n0, k):
    """n x n0, k entries per row in distinct columns (k <= n0): the operator's cost does not depend on the values"""
    r = np.arange(n, dtype=np.int64)
    colidx = np.sort(np.stack([(7 * r + (n0 // k) * j) % n0 for j in range(k)], axis=1), axis=1).astype(np.int32).ravel()
    return dict(rows=n, cols=n0, rowptr=(k * np.arange(n + 1)).astype(np.int32), colidx=colidx, val=np.full(k * n, 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cross", type=int, default=0, help="entries per row of a cross Hessian R_i on a third handle (0: none)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import families
    import pips_ipmpp_amd as pa
    lib = probe_library()
    chain = families.config3_chain(a.n).prefix(a.blocks)
    blocks = general_blocks(chain, a.blocks, 20261004)
    lines = [f"one Ipm::kmult (HIP events, median of {a.reps} after 3 warm-up applications), time-coupled family: {a.blocks} blocks x {a.n} variables"]
    tri = [tridiagonal(a.n if k else chain.n0) for k in range(a.blocks + 1)]
    handles = [("LP handle", {}), ("QP handle, tridiagonal Hessian on every block", dict(hessians=tri))]
    if a.cross > 0:
        handles.append((f"the same with R_i of {a.cross} entries per row",
                        dict(hessians=tri, cross_hessians=[None] + [sparse_cross(a.n, chain.n0, a.cross) for _ in range(a.blocks)])))
    for name, kw in handles:
        ipm = pa.GeneralIpmSolver(blocks, **kw)
        ms = (C.c_float * a.reps)()
        dims = (C.c_longlong * 3)()
        rc = lib.qp_probe_kmult(ipm._h, C.c_int(3), C.c_int(a.reps), ms, dims)
        if rc:
            raise SystemExit(f"qp_probe_kmult failed ({rc})")
        t = np.sort(np.array(list(ms)))
        lines.append(f"  {name:48s} median {np.median(t) * 1e3:9.1f} us   min {t[0] * 1e3:9.1f}   max {t[-1] * 1e3:9.1f}   "
                     f"(vector [x|y|z] {dims[0]} entries, nnz(J) {dims[1]}, nnz(Q, both triangles) {dims[2]})")
        ipm.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
