"""KktSystem.solve_compressed_multi (KktSystem::solve_compressed_multi / solve_panel in csrc/kkt.hip.h, the kernels of csrc/borderpanel.hip.h)
judged column by column against the long-double arrowhead reference of tests/test_solve_compressed_judged_gpu.py.

The right-hand sides are the column sets of tests/solve_multi_cases.py: column j = 2^((j // 6) mod 11) x base column j mod 6 of the case's
util.ArrowheadReference, so every column of every call is judged with ArrowheadReference.ratios (backward, root_rows, forward_root,
forward_leaf: the measure of the solution over the same measure of x_ref0, the plain FP64 algorithm) after scaling it back, which is exact;
every sixth column is the all-zero right-hand side and must come back as exact zeros.  tests/test_solve_multi_reference_cpu.py shows that the
scaled columns have the scaled references to the bit and that the predicate at M = 64 rejects the six mutants, swapped columns and a column
solved with its neighbour's b0.  Nothing is compared with the device's earlier output except where bit identity is the claim (groups 3, 5).

Handles: _Handles of tests/test_solve_compressed_judged_gpu.py (LeafBatch + KktSystem, set_refinement_backward_error(2, 1e-15)), the knobs
unset.  Every case asserts solve_multi_info() - path, chunks, right-hand sides per chunk - and the leaf and root inertia (no perturbed pivot).

  1. widths       small, nrhs in {8, 31, 32, 33, 64, 257}: the threshold, a panel less one, one panel, one more, two, a second chunk of one column.
  2. strides      small, nrhs = 33, ld0 = S_full + 3, ldl = n_total + 5: the gaps hold a sentinel and keep it to the bit.
  3. below        small in deterministic mode, nrhs in {1, 7}: bit-equal to solve_compressed column by column on a twin handle, path 0,
                  solve_check_counts() advanced as by the single calls.
  4. structures   nrhs = 40 on dense_tail, time_coupled (rows of Bt beyond one pass of k_border_tmult_panel), width129 (the root panel over a
                  tile edge; leaf rows with a second pass of k_border_mult_panel), general, general_mz0 (k_z0_elim_panel, the reduced panel,
                  Bunch-Kaufman root), general_mz0 with set_root_pivoting(0), two_link_6 with the sparse root.
  5. deterministic  small and general_mz0, nrhs = 40 (k_border_tmult_panel<true>, k_gather_rows_panel, k_reduce_groups on the panel): a
                  repeated call and a second handle give the same bits.
  6. state        factorize, a single solve, a panel call (nrhs = 33), two single solves - and the same on a twin handle without the panel
                  call: last_solve_path() after each single solve and solve_check_counts() are equal, by default and with set_solve_check(2).
  7. new_factors  factorize, panel call, factorize with 1.3 x the leaf diagonals, panel call: each judged against its own reference.
  8. errors       PIPS_ERR_ARG for a NULL pointer, nrhs < 0, ld0 < S + mz0, ldl < n_total; PIPS_ERR_STATE before the first factorisation;
                  nrhs == 0 leaves both arrays untouched.
  9. the two border-panel kernels alone (LeafBatch.border_tmult_panel / border_mult_panel, the launches of solve_panel), 33 strided vectors on
                  small, time_coupled (six passes of k_border_tmult_panel) and width129 (a second pass of k_border_mult_panel): every entry
                  within gamma(n + 3) (|t0| + |alpha| sum |a||x|) of the long-double product, n the products that flow into it (the bound of
                  tests/border_cases.py: at most n + 2 roundings per term whatever the order, FMA or not); T is added to, W is stored (a
                  sentinel does not survive, rows without border entries hold exact zeros), the gaps between the vectors keep theirs.

Measured on an MI355X in one run: the largest ratio over the columns and cases of a group, and the margin M of the group - the smallest power
of two that is at least 4 x the largest of the four, never above 64:

    group            backward                        root_rows                          forward_root                   forward_leaf                      M
    1. widths        2.66 (small/33)                 1.64 (small/257)                   1.25 (small/257)               2.18 (small/33, /64)             16
    2. strides       2.17                            1.64                               1.25                           1.97                             16
    3. below         3.96 (nrhs 1 and 7, column 0)   0.83 (small/7)                     1.95 (small/7)                 2.98 (column 0)                  16
    4. structures    1.38 (width129)                 2.50 (general_mz0, static root)    3.89 (general_mz0)             2.96 (general_mz0, static root)  16
    5. deterministic 3.61 (small)                    1.52 (small)                       3.27 (general_mz0)             2.89 (small)                     16
    6. state         2.16 (check_every_second)       1.53 (default_checks)              1.16                           1.97                             16
    7. new_factors   2.46 (first)                    1.49 (second)                      2.20 (second)                  2.87 (second)                    16

Every panel chunk of that run ended its two leaf solves without a refinement step (solve_multi_info: 0, 0).  The refined single path measures
up to 2.25 (group 6 of tests/test_solve_compressed_judged_gpu.py, forward_root) and 3.96 in deterministic mode on `small` (its group 4, backward -
the figure group 3 here reproduces through the single path); the panels stay within 3.9 units of the plain FP64 algorithm's own error everywhere.
Outside deterministic mode k_border_tmult_panel sums with FP64 atomics, so those ratios move in their last digits from run to run.
"""
import ctypes as C

import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import solve_multi_cases as smc
from tests import util as u
from tests.test_solve_compressed_judged_gpu import _Handles

pytestmark = pytest.mark.gpu

# per group: the smallest power of two >= 4 x the largest measured ratio (see above); never above 64
M = {"widths": 16, "strides": 16, "below": 16, "structures": 16, "deterministic": 16, "state": 16, "new_factors": 16}
_KNOBS = ("PIPS_HIP_AUG_SWEEPS", "PIPS_HIP_MF_KONLY", "PIPS_HIP_SWEEP_LAUNCHES", "PIPS_HIP_BORDER_BACKWARD", "PIPS_HIP_SPARSE_ROOT_BAND", "PIPS_HIP_AUG_WITNESS",
          "PIPS_HIP_MULTI", "PIPS_HIP_FORCE_REDUCE")
SENTINEL = -7.25e77
_largest = {}


@pytest.fixture(scope="module", autouse=True)
def _report_groups():
    yield
    for group, r in _largest.items():
        print(f"\nsolve-multi-group group={group} " + " ".join(f"{name}={v:.4g}" for name, v in r.items()) + f" M={M[group]}")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)


def _call(h, ref, nrhs, gap0=0, gapl=0):
    """columns 0 .. nrhs - 1 of the case's set through solve_compressed_multi: (X0, XL) on the host and the whole device arrays"""
    import torch
    C0, CL = smc.columns(ref, nrhs)
    Sf, nt = ref.sys.S_full, ref.n_leaves
    B0 = torch.full((nrhs, Sf + gap0), SENTINEL, dtype=torch.float64, device="cuda")
    BL = torch.full((nrhs, nt + gapl), SENTINEL, dtype=torch.float64, device="cuda")
    B0[:, :Sf] = torch.tensor(C0, device="cuda")
    BL[:, :nt] = torch.tensor(CL, device="cuda")
    h.kkt.solve_compressed_multi(B0[:, :Sf], BL[:, :nt])
    h.bt.sync()
    return B0[:, :Sf].cpu().numpy(), BL[:, :nt].cpu().numpy(), B0.cpu().numpy(), BL.cpu().numpy()


def _judge(ref, X0, XL, group, path):
    r = smc.ratios(ref, X0, XL)
    worst = {name: (float(v.max()), int(v.argmax())) for name, v in r.items()}
    print(f"solve-multi-ratio group={group} path={path} columns={len(X0)} " + " ".join(f"{name}={v:.4g}@{j}" for name, (v, j) in worst.items()))
    old = _largest.setdefault(group, dict.fromkeys(r, 0.0))
    for name, (v, _) in worst.items():
        old[name] = max(old[name], v)
    for j in range(smc.N_BASES - 1, len(X0), smc.N_BASES):
        assert not X0[j].any() and not XL[j].any(), (path, j)
    assert M[group] <= u.UNREFINED_M_CAP
    ok = smc.accepts(ref, X0, XL, M[group])
    assert ok.all(), (path, list(np.nonzero(~ok)[0]), {name: v[~ok] for name, v in r.items()})


def _panel_info(nrhs, calls):
    return dict(path=1, chunks=(nrhs + 255) // 256, per_chunk=min(nrhs, 256), panel_calls=calls)


def _info(h):
    i = h.kkt.solve_multi_info()
    return {k: i[k] for k in ("path", "chunks", "per_chunk", "panel_calls")}, (i["lsolve_refinement_steps"], i["ltsolve_refinement_steps"])


# ---- 1. widths ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_handle():
    ref = u.arrowhead_reference("small")
    h = _Handles(ref)
    h.factorize(ref)
    yield ref, h
    h.close()


@pytest.mark.parametrize("nrhs", [8, 31, 32, 33, 64, 257])
def test_widths(nrhs, small_handle):
    ref, h = small_handle
    before = h.kkt.solve_multi_info()["panel_calls"]
    X0, XL, _, _ = _call(h, ref, nrhs)
    info, steps = _info(h)
    print(f"solve-multi-info widths/{nrhs} {info} refinement steps {steps}")
    assert info == _panel_info(nrhs, before + (nrhs + 255) // 256)
    _judge(ref, X0, XL, "widths", f"small/{nrhs}")


# ---- 2. strides -----------------------------------------------------------------------------------------------------------------------------
def test_strides(small_handle):
    ref, h = small_handle
    nrhs, Sf, nt = 33, ref.sys.S_full, ref.n_leaves
    before = h.kkt.solve_multi_info()["panel_calls"]
    X0, XL, B0, BL = _call(h, ref, nrhs, gap0=3, gapl=5)
    assert _info(h)[0] == _panel_info(nrhs, before + 1)
    assert B0.shape == (nrhs, Sf + 3) and BL.shape == (nrhs, nt + 5)
    assert np.array_equal(B0[:, Sf:], np.full((nrhs, 3), SENTINEL)) and np.array_equal(BL[:, nt:], np.full((nrhs, 5), SENTINEL))
    _judge(ref, X0, XL, "strides", "small/33/strided")


# ---- 3. below the threshold -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [1, 7])
def test_below_the_threshold_is_the_single_path(nrhs):
    ref = u.arrowhead_reference("small")
    h, twin = _Handles(ref, deterministic=True), _Handles(ref, deterministic=True)
    h.factorize(ref)
    twin.factorize(ref)
    X0, XL, _, _ = _call(h, ref, nrhs)
    ways = []
    C0, CL = smc.columns(ref, nrhs)
    for j in range(nrhs):
        b0, bl = h.torch.tensor(C0[j], device="cuda"), h.torch.tensor(CL[j], device="cuda")
        twin.kkt.solve_compressed(b0, bl)
        twin.bt.sync()
        ways.append(twin.kkt.last_solve_path())
        assert np.array_equal(b0.cpu().numpy(), X0[j]) and np.array_equal(bl.cpu().numpy(), XL[j]), j
    info = _info(h)[0]
    counts, way = (h.kkt.solve_check_counts(), twin.kkt.solve_check_counts()), h.kkt.last_solve_path()
    h.close()
    twin.close()
    print(f"solve-multi-below nrhs={nrhs} ways={ways} counts={counts}")
    assert info == dict(path=0, chunks=nrhs, per_chunk=1, panel_calls=0)
    assert counts[0] == counts[1] and way == ways[-1]
    _judge(ref, X0, XL, "below", f"small/{nrhs}/deterministic")


# ---- 4. structures --------------------------------------------------------------------------------------------------------------------------
_STRUCTURES = {"dense_tail": ("dense_tail", {}), "time_coupled": ("time_coupled", {}), "width129": ("width129", {}), "general": ("general", {}),
               "general_mz0": ("general_mz0", {}), "general_mz0_static_root": ("general_mz0", dict(pivoting=0)), "two_link_6_sparse_root": ("two_link_6", dict(sparse_root=True))}


@pytest.mark.parametrize("shape", list(_STRUCTURES))
def test_structures(shape):
    case, kw = _STRUCTURES[shape]
    ref = u.arrowhead_reference(case)
    h = _Handles(ref, sparse_root=kw.get("sparse_root", False))
    if "pivoting" in kw:
        h.kkt.set_root_pivoting(kw["pivoting"])
    h.factorize(ref)
    if case == "time_coupled":      # a row of Bt that takes several passes of 64 entries
        assert max(int(np.diff(ref.Bts[b].indptr).max()) for b in range(ref.sys.N)) > 64
    if case == "width129":          # a leaf row with more border entries than one pass of k_border_mult_panel holds (4)
        assert max(int(np.diff(ref.Bts[b].tocsc().indptr).max()) for b in range(ref.sys.N)) > 4
    if case == "general_mz0":
        assert ref.sys.mz0 == 4
    X0, XL, _, _ = _call(h, ref, 40)
    info, steps = _info(h)
    h.close()
    print(f"solve-multi-info structures/{shape} {info} refinement steps {steps}")
    assert info == _panel_info(40, 1)
    _judge(ref, X0, XL, "structures", f"{shape}/40")


# ---- 5. deterministic mode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "general_mz0"])
def test_deterministic(case):
    ref = u.arrowhead_reference(case)
    h = _Handles(ref, deterministic=True)
    h.factorize(ref)
    first = _call(h, ref, 40)
    repeated = _call(h, ref, 40)
    info = _info(h)[0]
    h.close()
    assert info == _panel_info(40, 2)
    _judge(ref, first[0], first[1], "deterministic", f"{case}/40")
    h2 = _Handles(ref, deterministic=True)
    h2.factorize(ref)
    again = _call(h2, ref, 40)
    h2.close()
    # (the comparison with the device's own earlier output that is the claim: the same columns again, on this handle and on a second one)
    assert np.array_equal(first[0], repeated[0]) and np.array_equal(first[1], repeated[1])
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


# ---- 6. the single path's state -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [None, 2], ids=["default_checks", "check_every_second"])
def test_the_panel_call_leaves_the_single_path_alone(check):
    ref = u.arrowhead_reference("small")
    h, twin = _Handles(ref), _Handles(ref)
    seen = []
    for hh, with_panel in ((h, True), (twin, False)):
        if check is not None:
            hh.kkt.set_solve_check(check)
        hh.factorize(ref)
        ways = [hh.solve(ref, 0)[2]]
        if with_panel:
            X0, XL, _, _ = _call(hh, ref, 33)
            assert _info(hh)[0] == _panel_info(33, 1)
            assert hh.kkt.last_solve_path() == ways[0]
        for k in (1, 3):
            x0, xl, way = hh.solve(ref, k)
            ways.append(way)
            assert ref.accepts(x0, xl, M["state"], k)[0]
        seen.append((ways, hh.kkt.solve_check_counts(), hh.kkt.last_ltsolve_from_factor()))
        hh.close()
    print(f"solve-multi-state check={check} with the panel call {seen[0]} without {seen[1]}")
    assert seen[0] == seen[1]
    _judge(ref, X0, XL, "state", f"small/33/check{check}")


# ---- 7. one handle, new factors -------------------------------------------------------------------------------------------------------------
def test_new_factors():
    first, second = u.arrowhead_reference("small"), u.arrowhead_reference("small_scaled")
    assert second.sys.diag_scale == u.ARROWHEAD_SECOND_DIAG_SCALE and second.sys.prob is first.sys.prob
    h = _Handles(first)
    sols = []
    for ref in (first, second):
        h.factorize(ref)
        sols.append(_call(h, ref, 40))
    info = _info(h)[0]
    h.close()
    assert info == _panel_info(40, 2)
    for ref, what, (X0, XL, _, _) in zip((first, second), ("first", "second"), sols):
        _judge(ref, X0, XL, "new_factors", f"small/{what}/40")
    # (the second factorisation is another system: the first reference does not hold for its solutions)
    assert not smc.accepts(first, sols[1][0], sols[1][1], u.UNREFINED_M_CAP)[:5].any()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    ref = u.arrowhead_reference("small")
    Sf, nt = ref.sys.S_full, ref.n_leaves
    h = _Handles(ref)
    B0 = torch.full((8, Sf), 1.5, dtype=torch.float64, device="cuda")
    BL = torch.full((8, nt), 2.5, dtype=torch.float64, device="cuda")
    lib, ptr = pa.capi.lib, pa.capi._ptr

    def raw(nrhs, b0, ld0, bl, ldl):
        rc = lib.pips_hip_kkt_solve_compressed_multi(h.kkt._h, C.c_int(nrhs), b0, C.c_longlong(ld0), bl, C.c_longlong(ldl))
        return rc, (lib.pips_hip_last_error() or b"").decode()

    rc_state, msg = raw(8, ptr(B0), Sf, ptr(BL), nt)
    assert rc_state != 0 and "pips_hip_kkt_factorize first" in msg
    with pytest.raises(pa.capi.PipsHipError, match="pips_hip_kkt_factorize first"):
        h.kkt.solve_compressed_multi(B0, BL)
    with pytest.raises(pa.capi.PipsHipError, match="pips_hip_kkt_factorize first"):      # (an empty call too, in C and through the wrapper alike)
        h.kkt.solve_compressed_multi(B0[:0], BL[:0])
    assert raw(0, ptr(B0), Sf, ptr(BL), nt)[0] == rc_state
    h.factorize(ref)
    rc_arg, msg = raw(-1, ptr(B0), Sf, ptr(BL), nt)
    assert rc_arg not in (0, rc_state) and "nrhs = -1" in msg
    rc, msg = raw(8, None, Sf, ptr(BL), nt)
    assert rc == rc_arg and "B0_dev is NULL" in msg
    rc, msg = raw(8, ptr(B0), Sf, None, nt)
    assert rc == rc_arg and "Bleaf_dev is NULL" in msg
    rc, msg = raw(8, ptr(B0), Sf - 1, ptr(BL), nt)
    assert rc == rc_arg and f"ld0 = {Sf - 1} is below S + mz0 = {Sf}" in msg
    rc, msg = raw(8, ptr(B0), Sf, ptr(BL), nt - 1)
    assert rc == rc_arg and f"ldl = {nt - 1} is below n_total = {nt}" in msg
    with pytest.raises(pa.capi.PipsHipError, match="ld0"):
        h.kkt.solve_compressed_multi(B0[:, :Sf - 1].contiguous(), BL)
    with pytest.raises(ValueError):
        h.kkt.solve_compressed_multi(B0[:7], BL)
    # nrhs == 0: nothing happens, through the C entry and through the wrapper
    assert raw(0, ptr(B0), Sf, ptr(BL), nt)[0] == 0 and raw(0, None, 0, None, 0)[0] == 0
    h.kkt.solve_compressed_multi(B0[:0], BL[:0])
    h.bt.sync()
    assert bool((B0 == 1.5).all()) and bool((BL == 2.5).all())
    assert h.kkt.solve_multi_info()["panel_calls"] == 0
    h.close()


# ---- 9. the border-panel kernels alone ------------------------------------------------------------------------------------------------------
def _gamma(n):
    eps = n * u.UNIT_ROUNDOFF
    return eps / (1.0 - eps)


@pytest.mark.parametrize("case", ["small", "time_coupled", "width129"])
def test_border_panel_kernels(case):
    import torch
    ref = u.arrowhead_reference(case)
    s, nt, nr = ref.sys, ref.n_leaves, 33
    assert s.mz0 == 0      # (the rows of Bt are the Schur rows)
    h = _Handles(ref)
    rng = np.random.default_rng(9)
    Z, X0 = rng.standard_normal((nr, nt + 5)), rng.standard_normal((nr, s.S + 3))
    Z[5, :nt] = 0.0
    X0[5, :s.S] = 0.0
    T0 = rng.standard_normal((s.S, nr + 2))
    Zd, Xd, Td = (torch.tensor(a, device="cuda") for a in (Z, X0, T0))
    Wd = torch.full((nr, nt + 5), SENTINEL, dtype=torch.float64, device="cuda")
    alpha_t, alpha_m = -1.0, 0.37
    h.bt.border_tmult_panel(Zd[:, :nt], Td[:, :nr], alpha_t)
    h.bt.border_mult_panel(Xd[:, :s.S], Wd[:, :nt], alpha_m)
    h.bt.sync()
    T, W = Td.cpu().numpy(), Wd.cpu().numpy()
    h.close()
    assert np.array_equal(T[:, nr:], T0[:, nr:]) and np.array_equal(W[:, nt:], np.full((nr, 5), SENTINEL))
    ld = np.longdouble
    want_T, mag_T, cnt_T = T0[:, :nr].astype(ld), np.abs(T0[:, :nr]).astype(ld), np.zeros(s.S)
    want_W, mag_W, cnt_W = np.zeros((nr, nt), ld), np.zeros((nr, nt), ld), np.zeros(nt)
    for b, Bt in enumerate(ref.Bts):
        sl = slice(b * s.n_leaf, (b + 1) * s.n_leaf)
        D, A = Bt.toarray().astype(ld), np.abs(Bt.toarray()).astype(ld)
        want_T += alpha_t * (D @ Z[:, sl].astype(ld).T)
        mag_T += abs(alpha_t) * (A @ np.abs(Z[:, sl]).astype(ld).T)
        cnt_T += np.diff(Bt.indptr)
        want_W[:, sl] = alpha_m * (X0[:, :s.S].astype(ld) @ D)
        mag_W[:, sl] = abs(alpha_m) * (np.abs(X0[:, :s.S]).astype(ld) @ A)
        cnt_W[sl] = np.diff(Bt.tocsc().indptr)
    err_T = np.abs(T[:, :nr].astype(ld) - want_T) / np.maximum(np.array([_gamma(n + 3) for n in cnt_T])[:, None] * mag_T, np.finfo(np.float64).tiny)
    err_W = np.abs(W[:, :nt].astype(ld) - want_W) / np.maximum(np.array([_gamma(n + 3) for n in cnt_W])[None, :] * mag_W, np.finfo(np.float64).tiny)
    print(f"border-panel-kernels case={case} largest error / bound: tmult {float(err_T.max()):.3g} mult {float(err_W.max()):.3g}")
    assert cnt_T.max() > (64 if case == "time_coupled" else 0) and cnt_W.max() > (4 if case == "width129" else 0) and (cnt_W == 0).any()
    assert not W[:, :nt][:, cnt_W == 0].any() and not W[5, :nt].any()
    assert np.array_equal(T[cnt_T == 0, :nr], T0[cnt_T == 0, :nr]) and np.array_equal(T[:, 5], T0[:, 5])
    assert float(err_T.max()) <= 1.0 and float(err_W.max()) <= 1.0
