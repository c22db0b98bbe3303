"""The leaf solve sweeps judged on their own output: iterative refinement switched off.

Every other parity test of the leaf solves runs with one refinement step, which squares a sweep's error: a kernel wrong at 1e-5 comes out
at 1e-10 and passes.  Here refinement is off (HipLdlSolver(..., refine_steps=0), LeafBatch.set_refinement(0, 0.0), set_options(refine_steps=0);
last_refinement_steps == 0 is asserted) and every right-hand side is measured on the host, from the full symmetric K, residual in long double:

    eta(x) = ||b - K x||inf / (||K||inf ||x||inf + ||b||inf)              eta_dev <= M max(eta_ref, 2^-53)
    ||x_dev - x*||inf <= M max(||x_ref0 - x*||inf, 2^-53 ||x*||inf)

eta_ref and x_ref0 are those of oracle.OracleLdl(..., refine_steps=0) - the same algorithm, static-pivot LDL^T and two triangular sweeps in FP64 -
and x* is the oracle's solution after two refinement steps.  tests/test_unrefined_reference_cpu.py proves for every case that the oracle
perturbs no pivot and that the predicate rejects, at M = 64, the oracle's unrefined solution rounded to float32 and the same with one entry
zeroed.  Nothing is compared with the device's own earlier output; the all-zero right-hand side must come back as exact zeros.

Cases (the smallest shapes that select each kernel; info() is asserted for the cut, for more than one tail tile, for the multi path):
  1. one right-hand side, a one-block batch (and, at the model's cut, a HipLdlSolver handle): cut model / all head / all tail x the
     single-launch tail sweeps k_tail_rows_fwd/bwd / PIPS_HIP_SWEEP_LAUNCHES=1 (k_tail_fwd/bwd) x atomics / PIPS_HIP_DETERMINISTIC=1 (slots and
     gathers, k_head_fwd, k_head_dscale), on time-coupled blocks of n_i = 600 (dissection off: chain and spine kernels) and 3000 (dissected),
     tails of 2 (model), 8 and 36 (all tail) tiles; all-tail leaves of dimension 127, 128, 129, 257 (last tile empty / full / one row / one
     row past two tiles);
  2. nrhs in {2, 7, 8, 31, 32, 33, 64, 65, 256, 257} device-resident right-hand sides on one handle, n_i = 1500 (head 1610, tail 640 = 5 tiles):
     PIPS_HIP_MULTI = 0 (grid.y sweeps of the single-vector kernels), 1 / 4 / 2 (k_mpermute, k_mhead, k_mhead_dscale and k_mtail_rows_fwd/bwd<2> /
     <4> / <8>: quarter, half, whole panels), the latter three also with PIPS_HIP_SWEEP_LAUNCHES=1 (k_mtail_fwd/bwd); PIPS_HIP_MULTI unset at 7 and
     8 (the use_multi threshold); deterministic mode at 8, 33, 65 (panel by panel through d_mvslot: k_mgather_slots, k_mleaf_fwd_gather).  Rows: Gaussian,
     the last one scaled by 1e6, row 1 all zero, rows 2 / 3 unit vectors in the head / tail of the device's elimination order (from 7 rows on);
  3. batches of 3 x 3900 (10 tail tiles) and 70 x 600 (3 tail tiles), primal diagonals within 1e-2 .. 1e2 (util.unrefined_batch_problem says why): LeafBatch.solve
     three times on one handle with three right-hand sides (flag epochs advance, tickets reset), HipLdlSolver.solve_batch three times, and
     solve_dev(nrhs=33, ld=n+5) on a handle of block 0 three times with the right-hand sides scaled by 1, 2, 4 (a stale piece of the previous
     solve would be off by a factor).
Not reachable for a judged solution with the documented knobs: the default slicing falling to whole panels (sweep.n_tasks * panels > 512 needs
several right-hand sides on a large batch, which only the blocked Schur mode's internal solves have); whole panels are run through PIPS_HIP_MULTI=2.

Measured on an MI355X, largest ratio over all cases and right-hand sides of a path (backward = eta_dev / max(eta_ref, 2^-53), forward likewise):
(single-launch tail sweeps / PIPS_HIP_SWEEP_LAUNCHES=1 where they differ; "det" = deterministic mode)

    path                                                            backward           forward
    1. one rhs, model cut (batch of one and handle)                 0.0076             1.03
       one rhs, model cut, det                                      0.0073             1.03
       one rhs, all head                                            0.0083             2.54
       one rhs, all head, det                                       0.0082             2.54
       one rhs, all tail (127 .. 4500 rows)                         0.204              2.15
       one rhs, all tail, det                                       0.106              2.97
    2. PIPS_HIP_MULTI=0 (grid.y sweeps)                             0.832              10.3
       PIPS_HIP_MULTI=1 (quarter panels, k_mtail_rows<2>)           1.06 / 1.01        10.2 / 10.3
       PIPS_HIP_MULTI=4 (half panels, k_mtail_rows<4>)              1.07 / 1.05        10.2 / 10.3
       PIPS_HIP_MULTI=2 (whole panels, k_mtail_rows<8>)             1.06 / 1.08        10.3 / 10.2
       PIPS_HIP_MULTI unset, 7 and 8 rhs                            0.926              7.77
       PIPS_HIP_MULTI=1, det (slots, k_mgather_slots)               1.01 / 1.01        9.11 / 9.11
    3. LeafBatch.solve x 3, 3 x 3900                                0.665 / 0.608      1.02 / 1.11
       LeafBatch.solve x 3, 3 x 3900, det                           0.652 / 0.652      0.935 / 0.935
       LeafBatch.solve x 3, 70 x 600                                1.76 / 1.98        2.85 / 2.85
       LeafBatch.solve x 3, 70 x 600, det                           1.72 / 1.72        3.72 / 3.72
       solve_batch x 3, 3 x 3900                                    0.625 / 0.607      0.988 / 0.983
       solve_batch x 3, 70 x 600                                    2.00 / 1.95        3.43 / 2.85
       solve_dev(33, ld = n + 5) x 3, block of 3900                 1.42 / 1.28        0.94 / 1.06
       solve_dev(33, ld = n + 5) x 3, block of 600                  2.08 / 1.69        1.99 / 1.68

eta_ref lies below 2^-53 in most cases (||K||inf is near 1e4, the largest primal diagonal), so the backward ratios are mostly those against the
floor.  Largest backward ratio 2.08: M = 16, the smallest power of two that is at least 4 x 2.08 = 8.3; the forward check is held to the same M
(its largest ratio is 10.3, a Gaussian row of case 2 at nrhs = 256 - the same within 2 % on every path that solves it, the per-right-hand-side
sweeps included: the device's elimination order against the oracle's, not a kernel).
"""
import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import util as u

pytestmark = pytest.mark.gpu

M = 16       # the smallest power of two >= 4 x the largest measured backward ratio (2.08), see above; never above 64


def _judge(ref, X, path):
    """every right-hand side of ref against the predicate; the figures are printed before they are asserted"""
    X = np.atleast_2d(X)
    bw, fw = ref.backward_ratios(X), ref.forward_ratios(X)
    print(f"unrefined-ratio path={path} backward={bw.max():.4g} forward={fw.max():.4g}")
    assert M <= u.UNREFINED_M_CAP
    assert (bw <= M).all(), (path, int(np.argmax(bw)), bw.max(), ref.eta_ref[np.argmax(bw)])
    assert (fw <= M).all(), (path, int(np.argmax(fw)), fw.max())


def _env(monkeypatch, sweeps, det, multi=None):
    for k, v in (("PIPS_HIP_SWEEP_LAUNCHES", "1" if sweeps == "launches" else None), ("PIPS_HIP_DETERMINISTIC", "1" if det else None),
                 ("PIPS_HIP_MULTI", multi)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _one_block_batch(prob, force_n_head):
    bt = pa.LeafBatch(1, 0)
    bt.set_block(0, prob.blocks[0]["K"], prob.n_i)
    bt.set_options(force_n_head=force_n_head, refine_steps=0)
    bt.analyze(1)
    bt.set_values(0, prob.blocks[0]["K"].val)
    bt.factor()
    return bt


# ---- 1. one right-hand side -------------------------------------------------------------------------------------------------------------
_SINGLE = [(s, c) for s in ("chain_and_spine", "dissected") for c in ("model", "all_head", "all_tail")] + \
          [(s, "all_tail") for s in ("tail127", "tail128", "tail129", "tail257")]


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("sweeps", ["rows", "launches"])
@pytest.mark.parametrize("shape,cut", _SINGLE, ids=[f"{s}-{c}" for s, c in _SINGLE])
def test_one_right_hand_side(shape, cut, sweeps, det, monkeypatch):
    _env(monkeypatch, sweeps, det)
    if shape == "chain_and_spine":
        monkeypatch.setenv("PIPS_HIP_ND_DEPTH", "0")     # keeps the chain / spine kernels under test
    ref = u.unrefined_reference("single", shape)
    prob, n = ref.prob, ref.prob.n_leaf
    bt = _one_block_batch(prob, {"model": -1, "all_head": n, "all_tail": 0}[cut])
    info = bt.info()
    if cut == "all_head":
        assert info["n_head"] == n and info["m"] == 0, info
    elif cut == "all_tail":
        assert info["n_head"] == 0 and info["m"] == n and info["ntc"] == -(-n // 128), info     # 1, 1, 2, 3 tiles; 900 and 4500 rows: 8 and 36
    else:
        assert 0 < info["n_head"] < n and info["ntc"] > 1 and info["n_head"] + info["m"] == n, info    # head kernels and a tail of two tiles
    x = ref.B[0].copy()
    bt.solve(x)
    assert bt.last_refinement_steps() == 0
    assert bt.inertia(0) == (prob.n_i, prob.my_i, 0)
    bt.close()
    path = f"single/{cut}/{sweeps}/{'det' if det else 'atomics'}"
    _judge(ref, x, path)
    if cut == "model":       # the drop-in handle: the same engine behind pips_hip_ldl_solve
        s = pa.HipLdlSolver(prob.blocks[0]["K"], n_primal=prob.n_i, refine_steps=0)
        if det:
            s.set_deterministic()
        s.matrixChanged()
        x = ref.B[0].copy()
        s.solve(x)
        hinfo = s.info()
        assert hinfo["last_refinement_steps"] == 0 and hinfo["n_head"] == info["n_head"] and hinfo["m"] == info["m"], hinfo
        s.close()
        _judge(ref, x, path)


# ---- 2. several right-hand sides on one handle ------------------------------------------------------------------------------------------
_MULTI = [(nrhs, multi, sweeps, False) for multi in ("0", "1", "2", "4") for sweeps in ("rows", "launches") if not (multi == "0" and sweeps == "launches")
          for nrhs in u.UNREFINED_MULTI_NRHS] + \
         [(nrhs, None, "rows", False) for nrhs in (7, 8)] + \
         [(nrhs, "1", sweeps, True) for sweeps in ("rows", "launches") for nrhs in (8, 33, 65)]


def _multi_id(c):
    nrhs, multi, sweeps, det = c
    return f"{nrhs}-multi{'_unset' if multi is None else multi}-{sweeps}{'-deterministic' if det else ''}"


@pytest.mark.parametrize("case", _MULTI, ids=[_multi_id(c) for c in _MULTI])
def test_several_right_hand_sides(case, monkeypatch):
    import torch
    nrhs, multi, sweeps, det = case
    _env(monkeypatch, sweeps, False, multi)       # (a handle takes deterministic mode from set_deterministic)
    ref = u.unrefined_reference("multi", nrhs)
    prob, n = ref.prob, ref.prob.n_leaf
    s = pa.HipLdlSolver(prob.blocks[0]["K"], n_primal=prob.n_i, refine_steps=0)
    if det:
        s.set_deterministic()
    s.matrixChanged()
    Xd = torch.tensor(ref.B, device="cuda")        # device-resident: every row goes through the sweeps, the all-zero one too
    s.solve_dev(Xd, nrhs=nrhs, ld=n)
    torch.cuda.synchronize()
    X = Xd.cpu().numpy()
    info = s.info()
    assert info["last_refinement_steps"] == 0
    assert info["n_head"] > 0 and info["m"] == 640 and info["n_head"] + info["m"] == n, info      # five tail tiles
    interleaved = nrhs >= 8 if multi is None else multi != "0"
    assert info["last_multi_path"] == (2 if det else 1 if interleaved else 0), info
    assert s.get_inertia() == (prob.n_i, prob.my_i, 0)
    s.close()
    assert not X[ref.what["zero"]].any()           # exact zeros
    _judge(ref, X, f"multi/{'unset' if multi is None else multi}/{sweeps}/{'det' if det else 'atomics'}")


# ---- 3. batches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("sweeps", ["rows", "launches"])
@pytest.mark.parametrize("shape", list(u.UNREFINED_BATCH_SHAPES))
def test_batch_solved_three_times(shape, sweeps, det, monkeypatch):
    _env(monkeypatch, sweeps, det)
    prob = u._unrefined_cached_problem("batch", shape)
    N, n = prob.N, prob.n_leaf
    refs = [u.unrefined_reference("batch", (shape, b)) for b in range(N)]
    bt = pa.LeafBatch(N, prob.S)
    for b in range(N):
        bt.set_block(b, prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"])
    bt.set_refinement(0, 0.0)
    bt.analyze(4)
    for b in range(N):
        bt.set_values(b, prob.blocks[b]["K"].val)
    bt.factor()
    assert bt.info()["ntc"] > 1, bt.info()              # more than one tail tile
    X = np.empty((3, N, n))
    for rep in range(3):                                # epochs advance, tickets are reset by the last workgroup of every launch
        x = np.concatenate([refs[b].B[rep] for b in range(N)])
        bt.solve(x)
        assert bt.last_refinement_steps() == 0
        X[rep] = x.reshape(N, n)
    for b in range(N):
        assert bt.inertia(b) == (prob.n_i, prob.my_i, 0)
    bt.close()
    worst = (0.0, 0.0)
    for b in range(N):
        bw, fw = refs[b].backward_ratios(X[:, b]), refs[b].forward_ratios(X[:, b])
        worst = (max(worst[0], bw.max()), max(worst[1], fw.max()))
        assert (bw <= M).all() and (fw <= M).all(), (b, bw, fw)
    print(f"unrefined-ratio path=batch/{shape}/{sweeps}/{'det' if det else 'atomics'} backward={worst[0]:.4g} forward={worst[1]:.4g}")


@pytest.mark.parametrize("sweeps", ["rows", "launches"])
@pytest.mark.parametrize("shape", list(u.UNREFINED_BATCH_SHAPES))
def test_array_of_handles_and_strided_right_hand_sides(shape, sweeps, monkeypatch):
    import torch
    _env(monkeypatch, sweeps, False)
    prob = u._unrefined_cached_problem("batch", shape)
    N, n = prob.N, prob.n_leaf
    refs = [u.unrefined_reference("batch", (shape, b)) for b in range(N)]
    solvers = [pa.HipLdlSolver(prob.blocks[b]["K"], n_primal=prob.n_i, refine_steps=0) for b in range(N)]
    pa.HipLdlSolver.factor_schur_batch(solvers)          # (the batch engine takes its refinement setting from the first handle)
    X = np.empty((3, N, n))
    for rep in range(3):
        sol = [refs[b].B[rep].copy() for b in range(N)]
        pa.HipLdlSolver.solve_batch(solvers, sol)
        X[rep] = np.stack(sol)
    assert pa.HipLdlSolver.inertia_batch(solvers) == [(prob.n_i, prob.my_i, 0)] * N
    for s in solvers:
        s.close()
    worst = (0.0, 0.0)
    for b in range(N):
        bw, fw = refs[b].backward_ratios(X[:, b]), refs[b].forward_ratios(X[:, b])
        worst = (max(worst[0], bw.max()), max(worst[1], fw.max()))
        assert (bw <= M).all() and (fw <= M).all(), (b, bw, fw)
    print(f"unrefined-ratio path=handles/{shape}/{sweeps}/solve_batch backward={worst[0]:.4g} forward={worst[1]:.4g}")
    # a handle of block 0 alone: 33 right-hand sides in rows longer than the system; what lies behind a row's first n entries stays
    ref = u.unrefined_reference("batch_multi", shape)
    nrhs, ld = u.UNREFINED_BATCH_NRHS, n + 5
    s = pa.HipLdlSolver(prob.blocks[0]["K"], n_primal=prob.n_i, refine_steps=0)
    s.matrixChanged()
    for rep in range(3):
        scale = 2.0 ** rep                                # exact in every operation of the solve: the reference scales with it to the bit
        Xd = torch.full((nrhs, ld), 7.5, dtype=torch.float64, device="cuda")
        Xd[:, :n] = torch.tensor(ref.B * scale, device="cuda")
        s.solve_dev(Xd, nrhs=nrhs, ld=ld)
        torch.cuda.synchronize()
        Xh = Xd.cpu().numpy()
        info = s.info()
        assert info["last_refinement_steps"] == 0 and info["last_multi_path"] == 1 and info["m"] > 128, info
        assert np.all(Xh[:, n:] == 7.5)
        assert not Xh[ref.what["zero"], :n].any()
        _judge(ref, Xh[:, :n] / scale, f"handles/{shape}/{sweeps}/solve_dev_strided")
    s.close()
