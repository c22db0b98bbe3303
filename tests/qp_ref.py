"""Helpers of the convex-QP tests (no test in here): block-diagonal Hessians for the random block problems of
tests/general_lp_gen.py, a numpy restatement of the harness' interior-point loop with a Hessian, and the optimality conditions of
     min c^T x + 1/2 x^T Q x   s.t.  A x = b,  clow <= C x <= cupp,  xlow <= x <= xupp.
The restatement solves the global reduced KKT matrix [[dd + Q, A^T, C^T], [A, -reg, 0], [C, 0, nOmegaInv]] with SuperLU; predictor,
corrector, Gondzio loop and weight search are the ones of oracle.ipm_oracle.solve_general, and with a Hessian both parts of the
iterate take ONE step length min(alpha_p, alpha_d) (two lengths leave (alpha_p - alpha_d) Q dx in rQ).  Without a Hessian the
loop is oracle.ipm_oracle.solve_general's, number for number."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from oracle.ipm_oracle import mehrotra_step_length, stepbound, weight_search


def lower_dict(Q):
    """scipy matrix -> lower-triangular CSR dict in the layout of the block dicts' matrices"""
    L = sp.csr_matrix(sp.tril(sp.csr_matrix(Q)))
    L.sort_indices()
    return dict(rows=L.shape[0], cols=L.shape[1], rowptr=L.indptr.tolist(), colidx=L.indices.tolist(), val=L.data.tolist())


def block_hessians(seed, blocks, kind):
    """(list of lower-triangular dicts or None, global scipy matrix) for the blocks of a block problem.
    "pd": R R^T + diag(U(0.1, 2)) on every block, R n x n with about three entries per row;
    "psd": blocks with odd index get none, the others R R^T with R n x max(1, n // 3), density 0.5 (singular, low rank)."""
    rng = np.random.default_rng(1000 + seed)
    out, mats = [], []
    for k, b in enumerate(blocks):
        n = int(b["n0"] if k == 0 else b["ni"])
        if kind == "pd":
            R = sp.random(n, n, density=min(1.0, 3.0 / n), random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
            Q = sp.csr_matrix(R @ R.T + sp.diags(rng.uniform(0.1, 2.0, n)))
        elif kind == "psd":
            if k % 2 == 1:
                out.append(None)
                mats.append(sp.csr_matrix((n, n)))
                continue
            R = sp.random(n, max(1, n // 3), density=0.5, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
            Q = sp.csr_matrix(R @ R.T)
        else:
            raise ValueError(kind)
        Q = sp.csr_matrix((Q + Q.T) * 0.5)
        out.append(lower_dict(Q))
        mats.append(Q)
    return out, sp.block_diag(mats, format="csr")


def solve_qp(d, Q=None, max_iter=100, mutol=1e-6, artol=1e-4, trace=None, dual_reg=0.0, gondzio=2):
    """The harness algorithm on the assembled data d (oracle.ipm_oracle.assemble) with the global Hessian Q (scipy, symmetric, or
    None).  Returns the dict of oracle.ipm_oracle.solve_general; dual_objective carries -1/2 x^T Q x (the Lagrangian dual)."""
    A, C = sp.csr_matrix(d["A"]), sp.csr_matrix(d["C"])
    c, b = d["c"], d["b"]
    my, nx = A.shape
    mz = C.shape[0]
    have_q = Q is not None
    Qm = sp.csr_matrix(Q) if have_q else sp.csr_matrix((nx, nx))
    M = np.concatenate([d["iclow"], d["icupp"], d["ixlow"], d["ixupp"]]).astype(float)
    Bd = np.concatenate([d["clow"], d["cupp"], d["xlow"], d["xupp"]]).astype(float) * M
    sgn = np.concatenate([np.ones(mz), -np.ones(mz), np.ones(nx), -np.ones(nx)])
    oU, oV, oW = mz, 2 * mz, 2 * mz + nx
    ncp = 2 * mz + 2 * nx
    n_pairs = int(M.sum())
    dnorm = max([np.abs(c).max(initial=0.0), np.abs(b).max(initial=0.0), np.abs(A.data).max(initial=0.0), np.abs(C.data).max(initial=0.0),
                 np.abs(Bd).max(initial=0.0), np.abs(Qm.data).max(initial=0.0)])
    dnorm = dnorm if dnorm > 0 else 1.0
    s0 = np.sqrt(dnorm)
    x, s, y, z = np.zeros(nx), np.zeros(mz), np.zeros(my), np.zeros(mz)
    G, L = s0 * M, s0 * M
    on = M != 0
    zero_res = (np.zeros(nx), np.zeros(my), np.zeros(mz), np.zeros(mz), np.zeros(ncp))

    def residuals():
        rQ = c - A.T @ y - C.T @ z - L[oV:oW] + L[oW:]
        if have_q:
            rQ = rQ + Qm @ x
        rG = np.concatenate([(s - Bd[:oU]) * M[:oU] - G[:oU], (s - Bd[oU:oV]) * M[oU:oV] + G[oU:oV],
                             (x - Bd[oV:oW]) * M[oV:oW] - G[oV:oW], (x - Bd[oW:]) * M[oW:] + G[oW:]])
        return rQ, A @ x - b, C @ x - s, z - L[:oU] + L[oU:oV], rG

    def objectives():
        half = 0.5 * (x @ (Qm @ x)) if have_q else 0.0
        return c @ x + half, b @ y + (sgn * Bd) @ L - half

    def newton(res, rL):
        """LinearSystem::solve + step.negate() for one residual set at the current iterate"""
        rQ, rA, rC, rz, rG = res
        ratio, q = np.zeros(ncp), np.zeros(ncp)
        ratio[on] = L[on] / G[on]
        q[on] = (L[on] * rG[on] + sgn[on] * rL[on]) / G[on]
        dd = ratio[oV:oW] + ratio[oW:]
        om = ratio[:oU] + ratio[oU:oV]
        nom = np.where(om != 0, -1.0 / np.where(om != 0, om, 1.0), 0.0)
        rs = rz + q[:oU] + q[oU:oV]
        K = sp.bmat([[sp.diags(dd) + Qm if have_q else sp.diags(dd), A.T, C.T],
                     [A, -dual_reg * sp.identity(my) if dual_reg else None, None],
                     [C, None, sp.diags(nom)]], format="csc")
        sol = spl.splu(K).solve(np.concatenate([rQ + q[oV:oW] + q[oW:], rA, rC - nom * rs]))
        dx, dy, dz = sol[:nx], -sol[nx:nx + my], -sol[nx + my:]
        ds = -(nom * (rs - dz))
        dG = np.concatenate([ds - rG[:oU], rG[oU:oV] - ds, dx - rG[oV:oW], rG[oW:] - dx]) * M
        dL = np.zeros(ncp)
        dL[on] = (rL[on] - L[on] * dG[on]) / G[on]
        return [-dx, -ds, -dG], [-dy, -dz, -dL]

    # start point: one affine solve from the pushed point (Q already in the matrix and in rQ), full step, shift
    P, D = newton(residuals(), G * L)
    x, s, G = x + P[0], s + P[1], G + P[2]
    y, z, L = y + D[0], z + D[1], L + D[2]
    viol = max(0.0, -G[on].min(initial=0.0), -L[on].min(initial=0.0))
    G = G + (1e3 + 2 * viol) * M
    L = L + (1e3 + 2 * viol) * M
    status, it, mu, rnorm = 1, 0, 0.0, 0.0
    phi_min = np.inf
    for it in range(max_iter):
        res = residuals()
        rnorm = max(np.abs(r).max(initial=0.0) for r in res)
        mu = G @ L / n_pairs if n_pairs else 0.0
        pobj, dobj = objectives()
        if trace is not None:
            trace.append((it, mu, rnorm, pobj, dobj))
        if mu <= mutol and rnorm <= artol * dnorm:
            status = 0
            break
        phi = (rnorm + abs(pobj - dobj)) / dnorm
        phi_min = phi if it == 0 else min(phi_min, phi)
        if it >= 10 and phi >= 1e-8 and phi >= 1e4 * phi_min:
            status = 4
            break
        # predictor, then the corrector with the weights of the 11-point search
        P, D = newton(res, G * L)
        ap, ad = min(1.0, stepbound(G, P[2])), min(1.0, stepbound(L, D[2]))
        sigma = (((G + ap * P[2]) @ (L + ad * D[2]) / n_pairs) / mu) ** 3
        cP, cD = newton(zero_res, P[2] * D[2] - sigma * mu * M)
        ap, ad, wp, wd = weight_search(G, P[2], cP[2], L, D[2], cD[2], ap, ad)
        P = [u + wp * v for u, v in zip(P, cP)]
        D = [u + wd * v for u, v in zip(D, cD)]
        # Gondzio's correctors
        rmin, rmax = sigma * mu * 0.1, sigma * mu * 10.0
        ng = 0
        while ng < gondzio and (ap < 1.0 or ad < 1.0):
            apt, adt = min(1.0, 1.5 * ap + 0.3), min(1.0, 1.5 * ad + 0.3)
            prod = (G + apt * P[2]) * (L + adt * D[2])
            t = np.maximum(np.where(prod < rmin, rmin - prod, np.where(prod > rmax, rmax - prod, 0.0)), -rmax)
            cP, cD = newton(zero_res, -t * M)
            ape, ade, wp, wd = weight_search(G, P[2], cP[2], L, D[2], cD[2], apt, adt)
            both_one = ape >= 1.0 and ade >= 1.0
            p_better, d_better = ape >= 1.01 * ap, ade >= 1.01 * ad
            if not (both_one or p_better or d_better):
                break
            if both_one or p_better:
                P = [u + wp * v for u, v in zip(P, cP)]
                ap = ape
            if both_one or d_better:
                D = [u + wd * v for u, v in zip(D, cD)]
                ad = ade
            ng += 1
            if both_one:
                break
        ap, ad = mehrotra_step_length(G, P[2], L, D[2], n_pairs)
        if have_q:
            ap = ad = min(ap, ad)
        x, s, G = x + ap * P[0], s + ap * P[1], G + ap * P[2]
        y, z, L = y + ad * D[0], z + ad * D[1], L + ad * D[2]
        if trace is not None:
            trace[-1] = trace[-1] + (sigma, ap, ad)
    pobj, dobj = objectives()
    return dict(objective=pobj, iterations=it, mu=mu, rnorm=rnorm, status=status, dual_objective=dobj, x=x, s=s, y=y, z=z, dnorm=dnorm,
                t=G[:oU], u=G[oU:oV], v=G[oV:oW], w=G[oW:], lam=L[:oU], pi=L[oU:oV], gamma=L[oV:oW], phi=L[oW:])


def kkt_check_qp(d, Q, itr, tol):
    """The iterate satisfies the optimality conditions of the ORIGINAL bounded QP (sufficient for a convex problem): the check of
    tests/test_native_general_gpu.py with c + Q x in the stationarity row."""
    x, y, z = itr["x"], itr["y"], itr["z"]
    g = d["c"] + (sp.csr_matrix(Q) @ x if Q is not None else 0.0)
    scale = max(1.0, np.abs(d["b"]).max(initial=0.0), np.abs(d["c"]).max(initial=0.0))
    assert np.abs(d["A"] @ x - d["b"]).max(initial=0.0) < tol * scale
    act = d["C"] @ x
    assert ((act - d["clow"]) * d["iclow"]).min(initial=0.0) > -tol * scale and ((d["cupp"] - act) * d["icupp"]).min(initial=0.0) > -tol * scale
    assert ((x - d["xlow"]) * d["ixlow"]).min(initial=0.0) > -tol * scale and ((d["xupp"] - x) * d["ixupp"]).min(initial=0.0) > -tol * scale
    for k in ("lam", "pi", "gamma", "phi"):
        assert itr[k].min(initial=0.0) >= 0.0
    assert np.abs(g - d["A"].T @ y - d["C"].T @ z - itr["gamma"] + itr["phi"]).max(initial=0.0) < tol * scale      # stationarity
    assert np.abs(z - itr["lam"] + itr["pi"]).max(initial=0.0) < tol * scale
    assert np.abs(itr["gamma"] * (x - d["xlow"]) * d["ixlow"]).max(initial=0.0) < tol * scale ** 2
    assert np.abs(itr["phi"] * (d["xupp"] - x) * d["ixupp"]).max(initial=0.0) < tol * scale ** 2
    assert np.abs(itr["lam"] * (act - d["clow"]) * d["iclow"]).max(initial=0.0) < tol * scale ** 2
    assert np.abs(itr["pi"] * (d["cupp"] - act) * d["icupp"]).max(initial=0.0) < tol * scale ** 2


def long_row_case(s=0):
    """The dense-root shape of the long-row test (problem seed 500 + s): blocks, Hessian dicts and the global matrix.  Q0 = R R^T / 520 + I is dense: every
    row of its full storage has 520 entries, more than the harness' long-row threshold of 512; the leaves get diagonal Hessians."""
    from tests.general_lp_gen import random_block_lp
    blocks = random_block_lp(500 + s, 3, 520, 12, 4, 3, 2, 2, free_fraction=0.0)
    rng = np.random.default_rng(2000)
    R = rng.standard_normal((520, 520))
    mats = [sp.csr_matrix(R @ R.T / 520.0 + np.eye(520))]
    for _ in blocks[1:]:
        mats.append(sp.diags(rng.uniform(0.1, 2.0, 12)).tocsr())
    return blocks, [lower_dict(m) for m in mats], sp.block_diag(mats, format="csr")
