"""The dense root's solves of many right-hand sides (DenseLdl::solve_multi_dev in csrc/denseroot.hip.h: k_root_interleave, then the leaf solver's
interleaved tail sweeps k_mtail_rows_fwd / _bwd<NC>, k_mtail_fwd / _bwd on panels of 32) judged against a long-double reference, per right-hand
side, by the predicate of tests/test_dense_root_judged_gpu.py:

    forward    max|x - x*| <= M max(max|x_ref0 - x*|, 2^-53 max|x*|)
    backward   eta(x)      <= M max(eta(x_ref0), 2^-53)

Cases, right-hand sides (70 per case: three panels, the last with 6 columns; row 5 zero, row 40 e_0, row 69 e_{n-1}) and references:
tests/dense_root_multi_cases.py; tests/test_dense_root_multi_reference_cpu.py proves that the references converged and that the predicate at
M = 64 rejects two columns swapped inside a panel and across panels, and a column left at its right-hand side.
  1. static order, every case, the host entry with 70 right-hand sides in the four forms of the sweeps - default (quarter panels at these
     sizes), PIPS_HIP_MULTI=4 (half panels), PIPS_HIP_MULTI=2 (whole panels), PIPS_HIP_MULTI=2 with PIPS_HIP_SWEEP_LAUNCHES=1 (a launch per tile
     column) - each asserted through info(); row 5 stays exactly zero; both factorisation drivers on the two n = 385 cases.
  2. counts around the threshold, n = 257: 7 right-hand sides take the per-vector sweeps with the bits of seven single solves; 8, 32, 33, 64 and
     65 take the panels and are judged.
  3. the device entry, n in {129, 257}: ld = n + 3 with sentinels behind every vector (unchanged), the bits of the host entry, three repeated
     solves with identical bits, nrhs = 0 a no-op.  And 260 right-hand sides at n = 129: a chunk of 256 (eight panels in quarter slices, all 32
     rows of tickets and flags) and one of 4, host and device entry with equal bits, at most 4 host waits.
  4. Bunch-Kaufman: three cases judged against x_ref0 = dsytrs with their inertia; zero_leading_tile, whose pivot order is not the identity (the
     copy in and out gathers and scatters by it), factorised twice with the bounds of tests/test_root_pivoting_gpu.py.
  5. host stops: one solve of 70 right-hand sides makes at most 4 host waits (one per chunk and the read of the sweep's error word) where a
     loop over the right-hand sides makes 70; close() returns every allocation.
  6. two ranks: each rank solves the 70 right-hand sides through the panels; every rank's solution is judged.

Measured on an MI355X, the largest ratio over the cases, forms and right-hand sides of a group (the case it comes from), and the margin M of
the group: the smallest power of two that is at least 4 x the larger of the two, never above 64:

    group                                        forward                     backward                    M
    static order (1., 2., 3., 5.)                3.45 (n129-p86-spread)      2.82 (n129-p86-spread)      16
    Bunch-Kaufman (4.)                           11.89 (n385-p256-spread)    11.86 (n385-p256-spread)    64
    two ranks (6.)                               1.67                        1.36                         8

The four forms of the sweeps give the same ratios case by case (the arithmetic of a right-hand side does not depend on the slicing), the
device entry the bits of the host entry; at n = 385 the launch-per-step factorisation measures 3.15 / 2.55 (spread), the single launch
2.27 / 1.80.  Bunch-Kaufman on n385-p256-spread measures 7.0 / 7.4 with the five right-hand sides of tests/test_dense_root_judged_gpu.py and
11.9 with the 70 here; the per-vector sweeps (PIPS_HIP_MULTI=0) on the same 70 measure 12.1 / 9.2, so the figure is the factor's - the pivot
search bounded to the diagonal tile (that file's docstring) - and the number of draws, not the panels'.
zero_leading_tile: residual 7.9e-12, 5.3e-12 against LAPACK, one factorisation under a new order.  Host waits of one solve(70): 2.
"""
import os

import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import dense_root_multi_cases as mc
from tests import util as u

pytestmark = pytest.mark.gpu

# per group: the smallest power of two >= 4 x the largest measured ratio (see above); never above 64
M = {"static": 16, "bunch_kaufman": 64, "two_ranks": 8}
_KNOBS = ("PIPS_HIP_ROOT_LAUNCHES", "PIPS_HIP_MULTI", "PIPS_HIP_SWEEP_LAUNCHES")
# form -> (environment, slices per panel, single-launch sweeps) as info() must report them
_FORMS = {"default": ({}, 4, 1),
          "half_panels": ({"PIPS_HIP_MULTI": "4"}, 2, 1),
          "whole_panels": ({"PIPS_HIP_MULTI": "2"}, 1, 1),
          "column_launches": ({"PIPS_HIP_MULTI": "2", "PIPS_HIP_SWEEP_LAUNCHES": "1"}, 1, 0)}
_largest = {}


@pytest.fixture(scope="module", autouse=True)
def _report_groups():
    yield
    for group, (fwd, bwd) in _largest.items():
        print(f"\ndense-root-multi-group group={group} forward={fwd[0]:.4g} ({fwd[1]}) backward={bwd[0]:.4g} ({bwd[1]}) M={M[group]}")


def _env(monkeypatch, **knobs):
    """the knobs of this module: those given are set, the others unset (before the handle is created: it reads some in its constructor)"""
    for k in _KNOBS:
        if k in knobs:
            monkeypatch.setenv(k, knobs[k])
        else:
            monkeypatch.delenv(k, raising=False)


def _judge(ref, X, group, path, mode=0, rows=None):
    fwd, bwd = ref.ratios(X, mode)
    ok = ref.accepts(X, M[group], mode)
    if rows is not None:
        fwd, bwd, ok = fwd[:rows], bwd[:rows], ok[:rows]
    print(f"dense-root-multi-ratio group={group} path={path} forward={fwd.max():.4g} backward={bwd.max():.4g}")
    old = _largest.get(group, ((0.0, ""), (0.0, "")))
    _largest[group] = (max(old[0], (float(fwd.max()), path)), max(old[1], (float(bwd.max()), path)))
    assert M[group] <= u.UNREFINED_M_CAP
    assert ok.all(), (path, fwd, bwd)


def _solver(ref, pivoting=0):
    s = pa.HipDenseLdlSolver(ref.n, n_primal=-1 if ref.n_primal is None else ref.n_primal)
    if pivoting:
        s.set_pivoting(1)
    return s


def _assert_solve_path(s, form="default"):
    info = s.info()
    _, slices, rows = _FORMS[form]
    assert (info["last_solve_path"], info["last_solve_slices"], info["last_solve_rows"]) == (1, slices, rows), info
    return info


# ---- 1. static order: every case in the four forms of the sweeps, both factorisation drivers at n = 385 --------------------------------------
_DRIVER_CASES = [(c, "single") for c in mc.STATIC_CASES] + [(c, "launches") for c in mc.STATIC_CASES if c[0] == 385]


@pytest.mark.parametrize("form", list(_FORMS))
@pytest.mark.parametrize("case,driver", _DRIVER_CASES, ids=[f"{mc.case_id(c)}-{d}" for c, d in _DRIVER_CASES])
def test_static_order(case, driver, form, monkeypatch):
    _env(monkeypatch, **_FORMS[form][0], **({"PIPS_HIP_ROOT_LAUNCHES": "1"} if driver == "launches" else {}))
    ref = mc.reference(case, True)
    s = _solver(ref)
    s.matrixChanged(mc.host_matrix(ref))
    X = ref.B.copy()
    s.solve(X)
    info = _assert_solve_path(s, form)
    assert info["single_launch"] == (1 if driver == "single" else 0) and info["tile_columns"] == -(-ref.n // u.DENSE_ROOT_TILE), info
    assert s.get_inertia() == ref.inertia
    s.close()
    assert not X[5].any()
    _judge(ref, X, "static", f"{form}/{driver}/{mc.case_id(case)}")


# ---- 2. counts around the threshold -----------------------------------------------------------------------------------------------------------
_THRESHOLD_CASE = (257, 128, "spread")


def test_below_the_threshold_the_per_vector_sweeps_and_their_bits(monkeypatch):
    _env(monkeypatch)
    ref = mc.reference(_THRESHOLD_CASE, True)
    s = _solver(ref)
    s.matrixChanged(mc.host_matrix(ref))
    X = ref.B[:7].copy()
    s.solve(X)
    info = s.info()
    assert info["last_solve_path"] == 0 and info["last_solve_slices"] == 0, info
    for k in range(7):
        x = ref.B[k].copy()
        s.solve(x)
        assert np.array_equal(x, X[k]), k
    s.close()


@pytest.mark.parametrize("nrhs", [8, 32, 33, 64, 65])
def test_from_the_threshold_on_the_panels(nrhs, monkeypatch):
    _env(monkeypatch)
    ref = mc.reference(_THRESHOLD_CASE, True)
    s = _solver(ref)
    s.matrixChanged(mc.host_matrix(ref))
    X = ref.X_static.copy()                  # (the rows that are not solved keep x_ref0; only the solved ones are judged)
    Y = ref.B[:nrhs].copy()
    s.solve(Y)
    _assert_solve_path(s)
    s.close()
    X[:nrhs] = Y
    _judge(ref, X, "static", f"nrhs{nrhs}/{mc.case_id(_THRESHOLD_CASE)}", rows=nrhs)


# ---- 3. the device entry ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(129, 86, "spread"), (257, 128, "spread")], ids=mc.case_id)
def test_device_entry(case, monkeypatch):
    import torch
    _env(monkeypatch)
    ref = mc.reference(case, True)
    n, ld, nrhs = ref.n, ref.n + 3, mc.NRHS
    s = _solver(ref)
    s.matrixChanged(mc.host_matrix(ref))
    X_host = ref.B.copy()
    s.solve(X_host)
    padded = np.empty((nrhs, ld))
    padded[:, :n] = ref.B
    padded[:, n:] = 1e300 * (1.0 + np.arange(nrhs * 3).reshape(nrhs, 3))          # the sentinels
    got = []
    for _ in range(3):
        x_dev = torch.tensor(padded.ravel(), device="cuda")                        # exactly nrhs x ld doubles
        s.solve_multi_dev(x_dev, nrhs, ld)
        torch.cuda.synchronize()
        got.append(x_dev.cpu().numpy().reshape(nrhs, ld))
    _assert_solve_path(s)
    s.solve_multi_dev(x_dev, 0, ld)                                                # a no-op that returns 0
    torch.cuda.synchronize()
    assert np.array_equal(x_dev.cpu().numpy().reshape(nrhs, ld), got[-1])
    s.close()
    for Y in got:
        assert np.array_equal(Y[:, n:], padded[:, n:])
        assert np.array_equal(Y[:, :n], X_host)
    _judge(ref, np.ascontiguousarray(got[0][:, :n]), "static", f"device_entry/{mc.case_id(case)}")


def test_more_than_one_chunk(monkeypatch):
    """260 right-hand sides: a chunk of 256 - eight panels in quarter slices, 32 rows of tickets and flags, all there are - and one of 4, which
    stays on the panels.  The 70 right-hand sides over and over; every run of 70 is judged, host and device entry agree bit for bit."""
    import torch
    _env(monkeypatch)
    case = (129, 86, "spread")
    ref = mc.reference(case, True)
    n, nrhs = ref.n, 260
    B = ref.B[np.arange(nrhs) % mc.NRHS]
    s = _solver(ref)
    s.matrixChanged(mc.host_matrix(ref))
    X = B.copy()
    w0 = pa.host_wait_count()
    s.solve(X)
    waits = pa.host_wait_count() - w0
    _assert_solve_path(s)
    x_dev = torch.tensor(B.ravel(), device="cuda")
    s.solve_multi_dev(x_dev, nrhs, n)
    torch.cuda.synchronize()
    _assert_solve_path(s)
    s.close()
    assert waits <= 4, waits                                     # (two chunks, the error word)
    assert np.array_equal(x_dev.cpu().numpy().reshape(nrhs, n), X)
    for r0 in range(0, nrhs, mc.NRHS):
        Y = ref.X_static.copy()
        rows = min(mc.NRHS, nrhs - r0)
        Y[:rows] = X[r0:r0 + rows]
        _judge(ref, Y, "static", f"chunks/rows{r0}/{mc.case_id(case)}", rows=rows)


# ---- 4. Bunch-Kaufman -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.BK_CASES, ids=mc.case_id)
def test_bunch_kaufman(case, monkeypatch):
    _env(monkeypatch)
    ref = mc.reference(case, False)
    s = _solver(ref, pivoting=1)
    s.matrixChanged(mc.host_matrix(ref))
    X = ref.B.copy()
    s.solve(X)
    info = _assert_solve_path(s)
    assert info["pivoting"] == 1 and info["single_launch"] == 0, info
    assert s.get_inertia() == ref.inertia, (s.get_inertia(), ref.inertia)
    s.close()
    assert not X[5].any()
    _judge(ref, X, "bunch_kaufman", mc.case_id(case), mode=1)


def test_bunch_kaufman_with_a_pivot_order_of_its_own(monkeypatch):
    """zero_leading_tile of tests/test_root_pivoting_gpu.py: the order check_pivots builds is not the identity, so the copy into the panels
    gathers by it and the copy out scatters.  That test's own bounds, over all 70 right-hand sides."""
    _env(monkeypatch)
    ref = mc.reference(mc.ZERO_LEADING_TILE, False)
    Mx, B = ref.M, ref.B
    s = _solver(ref, pivoting=1)
    for rep in range(2):                                         # the second factorisation starts from the order the first one found
        s.matrixChanged(np.ascontiguousarray(np.tril(Mx)))
        X = B.copy()
        s.solve(X)
        info = _assert_solve_path(s)
        assert info["bk_refactorizations"] > 0, info
        assert s.get_inertia() == ref.inertia, (rep, s.get_inertia(), ref.inertia)
        res = np.linalg.norm(X @ Mx - B) / np.linalg.norm(B)
        err = np.linalg.norm(X - ref.X_lapack) / np.linalg.norm(ref.X_lapack)
        print(f"dense-root-multi-bk zero_leading_tile rep={rep} residual={res:.3g} against_lapack={err:.3g} refactorizations={info['bk_refactorizations']}")
        assert res < 1e-10
        assert err < 1e-8
        assert not X[5].any()
    s.close()


# ---- 5. host stops ----------------------------------------------------------------------------------------------------------------------------
def test_host_stops_and_allocations(monkeypatch):
    _env(monkeypatch)
    case = (385, 256, "flat")
    ref = mc.reference(case, True)
    live = pa.device_allocs_live()
    s = _solver(ref)
    s.matrixChanged(mc.host_matrix(ref))
    X = ref.B.copy()
    w0 = pa.host_wait_count()
    s.solve(X)
    waits = pa.host_wait_count() - w0
    _assert_solve_path(s)
    s.close()
    print(f"dense-root-multi-host-waits nrhs={mc.NRHS} waits={waits}")
    assert waits <= 4, waits
    assert pa.device_allocs_live() == live
    _judge(ref, X, "static", f"host_stops/{mc.case_id(case)}")


# ---- 6. two ranks -----------------------------------------------------------------------------------------------------------------------------
_TWO_RANK_CASE = (385, 256, "flat")


def _rank_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    M0, seed = mc.case_matrix(_TWO_RANK_CASE)                          # (the inputs alone: the parent holds the reference)
    X = mc.rhs(M0.shape[0], seed)
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
    s.matrixChanged(np.ascontiguousarray(u.dense_root_with_garbage_above(M0, seed + 900000)))
    s.solve(X)
    info = s.info()
    np.savez(os.path.join(out, f"rank{rank}.npz"), X=X, inertia=np.array(s.get_inertia()),
             info=np.array([info["single_launch"], info["tile_columns"], info["ranks"], info["pivoting"], info["last_solve_path"],
                            info["last_solve_slices"], info["last_solve_rows"]]))
    s.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks(tmp_path, monkeypatch):
    import torch.multiprocessing as mp
    _env(monkeypatch)                # (inherited by the spawned ranks)
    ref = mc.reference(_TWO_RANK_CASE, True)
    port = 29500 + (os.getpid() % 2000) + 223
    mp.start_processes(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    for r in range(2):
        g = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        assert tuple(g["inertia"]) == ref.inertia, g["inertia"]
        assert list(g["info"]) == [0, 4, 2, 0, 1, 4, 1], g["info"]     # four tile columns over two ranks; panels, quarter slices, single launches
        assert not g["X"][5].any()
        _judge(ref, g["X"], "two_ranks", f"rank{r}")
