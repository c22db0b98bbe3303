"""The dense root's solves (DenseLdl in csrc/denseroot.hip.h, k_root_ldl in csrc/rootkernel.hip.h) judged against a long-double reference.

The root factorises the Schur complement and solves with the factor WITHOUT refinement, so its solutions are measured as
tests/test_unrefined_sweeps_gpu.py measures the leaf sweeps, per right-hand side:

    forward    max|x - x*| <= M max(max|x_ref0 - x*|, 2^-53 max|x*|)
    backward   eta(x)      <= M max(eta(x_ref0), 2^-53)        eta(x) = ||b - M x||inf / (||M||inf ||x||inf + ||b||inf), residual in long double

x* is LAPACK's dsytrf / dsytrs solution refined on a long-double x until a correction is below 2^-58 max|x|; x_ref0 is the plain FP64 algorithm of
the same kind: the unblocked right-looking LDL^T in the given order for the static order, LAPACK's unrefined dsytrs for Bunch-Kaufman pivoting
(util.DenseRootReference).  tests/test_dense_root_reference_cpu.py proves for every case that the reference converged, that the static-order
factor has the hinted signs and no pivot the device's rule would replace, and that the predicate at M = 64 rejects a float32 factor, one entry
of L off by a relative 1e-9, a rank-one update left out, a right-hand side row dropped and a transposed read.  Nothing is compared with the
device's earlier output (bit-identity of repeated solves aside).

Matrices (util.DENSE_ROOT_CASES): [[H, A^T], [A, -G]] quasi-definite, families flat (cond about 20) and spread (diagonals over four decades, cond
1e2 .. 1e4), n in {1, 31, 32, 33, 127, 128, 129, 257, 385, 513} - the 32-wide sub-blocks of the blocked diagonal tile, the 128-wide tiles, and
three to five tile columns, from where the plan cuts K ranges - n_primal = (2 n) // 3, at n = 257 also 0, 128, 129 and 257: all dual, the sign
boundary on the tile edge, one past it, all primal.  Right-hand sides: three Gaussian ones, e_0 and e_{n-1}.  The strict upper triangle handed
to the device always holds other finite numbers, never the mirror image: the lower triangle is authoritative.  Every case asserts the inertia
(n_primal, n - n_primal, 0) exactly and, through HipDenseLdlSolver.info(), which driver factorised, the tile columns, the ranks and the pivoting mode.
  1. single launch (the default): every case, matrixChanged / solve with the five right-hand sides.
  2. a launch per step (PIPS_HIP_ROOT_LAUNCHES=1): every case with n >= 127.
  3. schedule variants of the single launch, n in {385, 513}: PIPS_HIP_ROOT_CHAIN_CU=0 (one task list) and PIPS_HIP_ROOT_DIAG_BARRIERS=1.
  4. the device entry the KKT layer uses: matrixChanged_dev on a column-major device matrix with lda = n + 3, other numbers above the diagonal and
     in the pad rows (and left as it was), then solve_dev per right-hand side; n in {129, 257}, both launch forms.
  5. one handle, several factorisations, n = 385: spread, then flat of the same shape (stale C tiles, flags or Winv of the first would show), then
     the same right-hand sides solved three times with identical bits.
  6. Bunch-Kaufman (set_pivoting(1)): flat and spread at n in {129, 385} against x_ref0 = dsytrs, zero_diagonal (N + N^T, diagonal zeroed) at
     n in {128, 300} with the inertia of eigvalsh; no perturbed pivot anywhere.
  7. two ranks, static order, flat, n = 385: tile columns {0, 2} and {1, 3}; every rank's solution is judged.

Measured on an MI355X, the largest ratio over the cases and right-hand sides of a group (the case it comes from), and the margin M of the
group: the smallest power of two that is at least 4 x the larger of the two, never above 64:

    group                                                      forward                     backward                    M
    1. single launch (with 5., single)                         3.20 (n257-p257-spread)     1.83 (n129-p86-spread)      16
    2. a launch per step (with 5., launches)                   3.26 (n257-p257-spread)     2.02 (n257-p129-spread)     16
    3. schedule variants: one list / barrier diagonal          2.73 / 1.37                 1.49 / 2.06                 16
    4. device entry: single launch / a launch per step         3.20 / 3.26                 1.83 / 2.02                 16
    6. Bunch-Kaufman, n300-zero_diagonal aside                 7.00 (n385-spread)          7.42 (n385-spread)          32
    7. two ranks (both ranks: the bits of the launch per step) 0.86                        0.77                         4

The static order stays within 3.3 units of the unblocked FP64 algorithm's own error on every driver, layout and schedule; the device entry gives
the bits of the host entry.  Bunch-Kaufman pivoting is bounded to the 128 x 128 diagonal tile, and that shows where the weight of a column lies
below its tile: the multipliers of the panel are no longer bounded by 1 / alpha = 1.56 as with dsytrf's search of the whole column.
    n300-zero_diagonal: forward 22.6, backward 36.0 - above 16, so no admissible margin holds it (4 x 36 > 64).
It is not a defect of the kernels: block elimination over 128-wide tiles in plain FP64 on the CPU, every diagonal tile solved by LAPACK's own
Bunch-Kaufman restricted to that tile, has multipliers up to 65 on this matrix and ratios of 141 / 149 - four times the device's
(tests/test_dense_root_reference_cpu.py asserts that it exceeds the margin).  n128-zero_diagonal, one tile, where the search IS the whole column,
measures 1.49 / 1.00.  The case stays, judged with the group's M = 32, as a strict expected failure: it fails the day the pivot search reaches
below the tile and the ratio falls within the margin.
"""
import os

import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import util as u

pytestmark = pytest.mark.gpu

# per group: the smallest power of two >= 4 x the largest measured ratio (see above); never above 64
M = {"single_launch": 16, "launch_per_step": 16, "variants": 16, "device_entry": 16, "bunch_kaufman": 32, "two_ranks": 4}
# beyond every admissible margin for a reason that lies in the algorithm (see above): case -> the measured (forward, backward)
_BEYOND_THE_MARGIN = {(300, None, "zero_diagonal"): (22.6, 36.0)}
_KNOBS = ("PIPS_HIP_ROOT_LAUNCHES", "PIPS_HIP_ROOT_CHAIN_CU", "PIPS_HIP_ROOT_DIAG_BARRIERS")
_FORMS = {"single": {}, "launches": dict(launches="1")}
_ID = u.dense_root_case_id
_largest = {}


@pytest.fixture(scope="module", autouse=True)
def _report_groups():
    yield
    for group, (fwd, bwd) in _largest.items():
        print(f"\ndense-root-group group={group} forward={fwd:.4g} backward={bwd:.4g} M={M[group]}")


def _env(monkeypatch, **knobs):
    """the knobs of this module: those given are set, the others unset (before the handle is created: it reads them in its constructor)"""
    for k in _KNOBS:
        v = knobs.get(k[len("PIPS_HIP_ROOT_"):].lower())
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _host_matrix(ref):
    """row-major, the lower triangle M's, the strict upper one other numbers"""
    return np.ascontiguousarray(u.dense_root_with_garbage_above(ref.M, ref.garbage_seed))


def _assert_path(s, ref, single, pivoting=0, ranks=1):
    info = s.info()
    assert info["single_launch"] == (1 if single else 0) and info["tile_columns"] == -(-ref.n // u.DENSE_ROOT_TILE), info
    assert info["ranks"] == ranks and info["pivoting"] == pivoting, info
    assert s.get_inertia() == ref.inertia, (s.get_inertia(), ref.inertia)
    return info


def _judge(ref, X, group, path, mode=0):
    fwd, bwd = ref.ratios(X, mode)
    print(f"dense-root-ratio group={group} path={path} forward={fwd.max():.4g} backward={bwd.max():.4g}")
    old = _largest.get(group, (0.0, 0.0))
    _largest[group] = (max(old[0], float(fwd.max())), max(old[1], float(bwd.max())))
    assert M[group] <= u.UNREFINED_M_CAP
    assert ref.accepts(X, M[group], mode).all(), (path, fwd, bwd)


def _factor_solve(ref, s):
    s.matrixChanged(_host_matrix(ref))
    X = ref.B.copy()
    s.solve(X)
    return X


# ---- 1. and 2. the two drivers of the static order -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", u.DENSE_ROOT_CASES, ids=[_ID(c) for c in u.DENSE_ROOT_CASES])
def test_single_launch(case, monkeypatch):
    _env(monkeypatch)
    ref = u.dense_root_reference(case)
    s = pa.HipDenseLdlSolver(ref.n, n_primal=ref.n_primal)
    X = _factor_solve(ref, s)
    _assert_path(s, ref, single=True)
    s.close()
    _judge(ref, X, "single_launch", _ID(case))


_FROM_127 = [c for c in u.DENSE_ROOT_CASES if c[0] >= 127]


@pytest.mark.parametrize("case", _FROM_127, ids=[_ID(c) for c in _FROM_127])
def test_launch_per_step(case, monkeypatch):
    _env(monkeypatch, launches="1")
    ref = u.dense_root_reference(case)
    s = pa.HipDenseLdlSolver(ref.n, n_primal=ref.n_primal)
    X = _factor_solve(ref, s)
    _assert_path(s, ref, single=False)
    s.close()
    _judge(ref, X, "launch_per_step", _ID(case))


# ---- 3. schedule variants of the single launch ---------------------------------------------------------------------------------------------
_VARIANT_CASES = [c for c in u.DENSE_ROOT_CASES if c[0] in (385, 513)]


@pytest.mark.parametrize("variant", ["one_list", "barrier_diagonal"])
@pytest.mark.parametrize("case", _VARIANT_CASES, ids=[_ID(c) for c in _VARIANT_CASES])
def test_schedule_variants(case, variant, monkeypatch):
    _env(monkeypatch, **{"one_list": dict(chain_cu="0"), "barrier_diagonal": dict(diag_barriers="1")}[variant])
    ref = u.dense_root_reference(case)
    s = pa.HipDenseLdlSolver(ref.n, n_primal=ref.n_primal)
    X = _factor_solve(ref, s)
    _assert_path(s, ref, single=True)
    s.close()
    _judge(ref, X, "variants", f"{variant}/{_ID(case)}")


# ---- 4. the device entry: column-major, lda > n ---------------------------------------------------------------------------------------------
_DEVICE_CASES = [c for c in u.DENSE_ROOT_CASES if c[0] in (129, 257)]


@pytest.mark.parametrize("form", list(_FORMS))
@pytest.mark.parametrize("case", _DEVICE_CASES, ids=[_ID(c) for c in _DEVICE_CASES])
def test_device_entry(case, form, monkeypatch):
    import torch
    _env(monkeypatch, **_FORMS[form])
    ref = u.dense_root_reference(case)
    n, lda = ref.n, ref.n + 3
    A = np.random.default_rng(ref.garbage_seed + 1).standard_normal((n, lda))       # A[c, r]: column c, lda entries apart
    A[:, :n] = np.triu(ref.M) + np.tril(A[:, :n], -1)                                 # rows r >= c of column c are M's, the others stay
    A_dev = torch.tensor(A, device="cuda")
    s = pa.HipDenseLdlSolver(n, n_primal=ref.n_primal)
    s.matrixChanged_dev(A_dev, lda)
    X = np.empty_like(ref.B)
    for k in range(ref.B.shape[0]):
        x = torch.tensor(ref.B[k], device="cuda")
        s.solve_dev(x)
        torch.cuda.synchronize()
        X[k] = x.cpu().numpy()
    _assert_path(s, ref, single=form == "single")
    s.close()
    assert np.array_equal(A_dev.cpu().numpy(), A)                                      # the caller's matrix is read, not written
    _judge(ref, X, "device_entry", f"{form}/{_ID(case)}")


# ---- 5. one handle, several factorisations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(_FORMS))
def test_one_handle_several_factorisations(form, monkeypatch):
    _env(monkeypatch, **_FORMS[form])
    group = "single_launch" if form == "single" else "launch_per_step"
    spread, flat = u.dense_root_reference((385, 256, "spread")), u.dense_root_reference((385, 256, "flat"))
    s = pa.HipDenseLdlSolver(385, n_primal=256)
    for ref, what in ((spread, "first/spread"), (flat, "second/flat")):
        X = _factor_solve(ref, s)
        _assert_path(s, ref, single=form == "single")
        _judge(ref, X, group, f"one_handle/{form}/{what}")
    again = []
    for _ in range(3):          # a solve leaves no state
        Y = flat.B.copy()
        s.solve(Y)
        again.append(Y)
    s.close()
    assert all(np.array_equal(X, Y) for Y in again)


# ---- 6. Bunch-Kaufman ------------------------------------------------------------------------------------------------------------------------
_BK_CASES = [c for c in u.DENSE_ROOT_CASES if c[0] in (129, 385) and c[1] == (2 * c[0]) // 3] + [(n, None, "zero_diagonal") for n in u.DENSE_ROOT_ZERO_DIAGONAL_SIZES]


@pytest.mark.parametrize("case", _BK_CASES, ids=[f"n{c[0]}-{c[2]}" for c in _BK_CASES])
def test_bunch_kaufman(case, monkeypatch):
    _env(monkeypatch)
    ref = u.dense_root_reference(case)
    s = pa.HipDenseLdlSolver(ref.n, n_primal=-1 if ref.n_primal is None else ref.n_primal)
    s.set_pivoting(1)
    X = _factor_solve(ref, s)
    info = _assert_path(s, ref, single=False, pivoting=1)          # (the inertia's third entry: no perturbed pivot)
    s.close()
    print(f"dense-root-bk case=n{case[0]}-{case[2]} refactorizations={info['bk_refactorizations']}")
    if case not in _BEYOND_THE_MARGIN:
        _judge(ref, X, "bunch_kaufman", f"n{case[0]}-{case[2]}", mode=1)
        return
    # the strict expected failure: inertia and path are asserted above, the predicate alone is expected to reject
    fwd, bwd = ref.ratios(X, 1)
    print(f"dense-root-ratio group=bunch_kaufman(beyond the margin) path=n{case[0]}-{case[2]} forward={fwd.max():.4g} backward={bwd.max():.4g}")
    assert np.isfinite(fwd).all() and np.isfinite(bwd).all()
    assert not ref.accepts(X, M["bunch_kaufman"], 1).all(), "within the margin now: take the case out of _BEYOND_THE_MARGIN"
    pytest.xfail("pivoting bounded to the diagonal tile: measured forward %.1f, backward %.1f x dsytrs's own error" % _BEYOND_THE_MARGIN[case])


# ---- 7. two ranks ----------------------------------------------------------------------------------------------------------------------------
_TWO_RANK_CASE = (385, 256, "flat")


def _rank_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    M0, X, garbage_seed = u.dense_root_case_inputs(_TWO_RANK_CASE)          # (the inputs alone: the parent holds the reference)
    n, n_primal = _TWO_RANK_CASE[:2]

    def allreduce(ptr, cnt):
        t = torch.as_tensor(pa.capi._DeviceDoubles(ptr, cnt), device="cuda")
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)
        torch.cuda.synchronize()

    comm = pa.ExternalComm(allreduce, n_ranks=world, rank=rank)
    s = pa.HipDenseLdlSolver(n, n_primal=n_primal)
    s.set_distributed(comm, rank, world)
    s.matrixChanged(np.ascontiguousarray(u.dense_root_with_garbage_above(M0, garbage_seed)))
    s.solve(X)
    info = s.info()
    np.savez(os.path.join(out, f"rank{rank}.npz"), X=X, inertia=np.array(s.get_inertia()),
             info=np.array([info["single_launch"], info["tile_columns"], info["ranks"], info["pivoting"]]))
    s.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks(tmp_path, monkeypatch):
    import torch.multiprocessing as mp
    _env(monkeypatch)                # (inherited by the spawned ranks)
    ref = u.dense_root_reference(_TWO_RANK_CASE)
    port = 29500 + (os.getpid() % 2000) + 211
    mp.start_processes(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    for r in range(2):
        g = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        assert tuple(g["inertia"]) == ref.inertia, g["inertia"]
        assert list(g["info"]) == [0, 4, 2, 0], g["info"]         # four tile columns: {0, 2} on rank 0, {1, 3} on rank 1
        _judge(ref, g["X"], "two_ranks", f"rank{r}")
