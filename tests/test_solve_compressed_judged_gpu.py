"""solveCompressed (KktSystem::solve_enqueue in csrc/kkt.hip.h) judged against a long-double reference of the whole arrowhead system.

By sweeps of the augmented factor (Engine::forward_augmented / forward_augmented_det / backward_augmented; ways 2 and 3 of
KktSystem.last_solve_path()) solveCompressed carries no refinement, and the device's own measure covers the leaf rows only: nobody measures the
root rows r_0 = b_0 - K_0 x_0 - sum_i Br_i^T x_i, and with set_solve_check(0) or (2) the followers go way 2 on trust.  So every solution is
measured here as tests/test_dense_root_judged_gpu.py measures the root's, per right-hand side (util.ArrowheadReference):

    backward      eta(x) <= M max(eta(x_ref0), 2^-53)     eta(x) = ||b - A x||inf / (||A||inf ||x||inf + ||b||inf), residual in long double
    root_rows     the same quotient over the root rows alone: ||r_0||inf / (||A_0||inf ||x||inf + ||b_0||inf)
    forward_root  max|x - x*| <= M max(max|x_ref0 - x*|, 2^-53 max|x*|) over [x0 | y0 | z0 | ylink | zlink]
    forward_leaf  the same over the leaf part

A is [[diag(K_i), Br_i], [Br_i^T, K_0]] assembled as one CSR; x* is scipy's LU solution of it refined on a long-double x until a correction is
below 2^-58 max|x|; x_ref0 is the plain FP64 algorithm of the same kind: the oracle's solve_compressed over unrefined oracle leaves and LAPACK's
dsytrf / dsytrs on the oracle's own Schur complement.  tests/test_solve_compressed_reference_cpu.py proves for every case that the reference
converged, that no pivot is perturbed, the inertia, and that the predicate at M = 64 rejects six mutants (float32 leaves, a block's or a single
border row's Br^T z left out, a root right-hand side off by a relative 1e-11, x0 with two entries swapped, z0 without C0 x0).  Nothing is compared
with the device's earlier output, the bit-identity of a repeated solve in deterministic mode aside.

Every handle: LeafBatch + KktSystem, set_refinement_backward_error(2, 1e-15) (the sweeps are taken only then), the knobs set before the handle is
created.  Every case asserts the way of each solve (last_solve_path), solve_check_counts(), info()["augmented_sweeps"], the leaf and root inertia
(no perturbed pivot): a case that does not take the way it is named for fails.  Right-hand sides per case (util.ARROWHEAD_RHS): two Gaussian ones,
b0 = 0, b_leaf = 0 (only the border path carries anything in the forward half), e of the last Schur index in b0, all zero (exact zeros come back).
The cases with the generator's diagonals have them narrowed to 1e-2 .. 1e2 (util._arrowhead_narrow_diagonals).

  1. sweeps, measured (way 3 each): small Problem(5, 3,200,100,12,10); dense_tail Problem(3, 4,1000,500,100,100) (k_tail_border_fwd); time-coupled
     (5, 3,3000,1500,10,8,6) plain, all head (force_n_head) and with PIPS_HIP_MF_KONLY=1.
  2. sweeps on trust: set_solve_check(0) -> ways 3, 2, 2, 2, 2, 2 and (2) -> 3, 2, 3, 2, 3, 2 (the right-hand sides in an order that puts the others
     on way 2) on small and time-coupled; every way-2 solution is judged.
  3. border widths at the tile and chunk edges: schur_problem(170, S, 1, "full"), S in {1, 127, 128, 129, 257}; schur_problem(400, 129, 3, "hetero");
     each at the model's cut and with all of K_i in the dense tail (force_n_head = 0: every border row goes through k_tail_border_fwd).
  4. deterministic mode (forward_augmented_det, group-wise gather, k_reduce_groups): small, time-coupled, S = 129; a repeated solve gives the same bits.
  5. PIPS_HIP_SWEEP_LAUNCHES=1 on dense_tail: layout.cpp's aug_paths needs the single-launch tail sweeps or no tail, so augmented_sweeps == 0
     and the solves go the refined way 0 (border_backward_ok needs those sweeps too), which is judged.
  6. the refined ways as the baseline: PIPS_HIP_AUG_SWEEPS=0 with PIPS_HIP_BORDER_BACKWARD 0 (way 0) and 1 on dense_tail and time-coupled.
     6d. the same with set_deterministic(True): lsolve_det without the sweeps (k_border_rowdot into g_btm_grp, k_reduce_groups) and the Ltsolve through
     k_border_entry_products + k_gather_slots; way 0 with either value of PIPS_HIP_BORDER_BACKWARD (border_backward_ok needs !deterministic); a
     repeated solve, on the same handle and on a second one, gives the same bits.
  7. the general structure with sweeps: GeneralProblem(21, 3,400,160,80,20,6,mz0,9,5) with mz0 = 0 and mz0 = 4 (k_z0_elim, the reduced vector).
  8. sparse root: TwoLinkProblem(77, 6,120,60,4,3) and (77, 30,60,30,5,20), PIPS_HIP_SPARSE_ROOT_BAND in {1, 0}.
  9. one handle, new factors: factorize, three solves, factorize with 1.3 x the leaf diagonals (the reference rebuilt for it), three solves.

Measured on an MI355X in one run, the largest ratio over the cases and right-hand sides of a group (the path it comes from), and the margin M of
the group: the smallest power of two that is at least 4 x the largest of the four, never above 64:

    group              backward                       root_rows                      forward_root                           forward_leaf                        M
    1. measured        1.10 (small)                   1.24 (dense_tail)              3.17 (time_coupled, e_last)            1.52 (time_coupled, b_leaf = 0)    16
    2. on_trust        1.68 (small/check2)            0.88 (small/check2)            3.17 (time_coupled/check2, e_last)     1.52 (time_coupled/check0)         16
    3. widths          1.58 (width257/model)          3.40 (width1/all_tail, e_last) 3.73 (width129/all_tail, e_last)       2.98 (width129/all_tail, e_last)   32 *
    4. deterministic   3.96 (small)                   0.83 (small)                   3.17 (time_coupled, e_last)            2.98 (small)                       16
    5. sweep_launches  0.74 (way 0)                   0.81                           1.20                                   1.17                                8
    6. refined         1.03 (dense_tail, way 1)       1.03 (dense_tail, way 1)       2.25 (time_coupled, way 0, e_last)     1.53 (time_coupled, way 0)         16
    6d. refined, det.  0.88 (dense_tail, b_leaf = 0)  0.88 (dense_tail, b_leaf = 0)  3.17 (time_coupled, e_last)            1.62 (time_coupled, e_last)        16
    7. general         0.55 (general)                 1.95 (general_mz0)             3.39 (general_mz0, b_leaf = 0)         2.83 (general_mz0)                 16
    8. sparse_root     0.62 (two_link_30/amd)         0.62 (two_link_30/amd)         1.79 (two_link_30/band)                0.99 (two_link_30/amd)              8
    9. new_factors     1.10 (small/first)             0.88 (small/second)            3.50 (time_coupled/first, e_last)      2.48 (small/second)                16

  * forward_augmented sums with FP64 atomics, so the ratios of groups 1 - 3 and 5 - 9 move from run to run in their last digits; an earlier run of the
    same code measured 4.82 on width1/model, b0 = 0 (4 x 4.82 > 16), and the group's margin takes that figure.
The sweeps stay within 4 units of the plain FP64 algorithm's own error on every path, measured or on trust, and the root rows - which the device
never measures - within 3.4.  The refined ways 0 and 1 (groups 5 and 6) are not markedly below the sweeps on these well-scaled cases: reported, not
asserted.  Every group reaches the way it is named for with the documented knobs: the general structure (group 7) and the sparse root in both
orders (group 8) take the sweeps, way 3 on every solve; PIPS_HIP_BORDER_BACKWARD=1 gives way 1 on every solve of group 6, and with
PIPS_HIP_SWEEP_LAUNCHES=1 (group 5) augmented_sweeps is 0 and every solve goes way 0.
    width1/all_tail, b0 = 0: forward_root 41.6 - above 16, so no admissible margin holds it (4 x 41.6 > 64); the other three ratios are below 1.2.
It is not a defect of a kernel.  With one Schur row the root part is one number, and x_ref0's own error in it is 2.4e-15 of it on this right-hand
side against 1.4e-14 .. 1.2e-13 on the others: the denominator is small by chance, the device's error (1e-13) is x_ref0's usual one.  The same
algorithm in plain FP64 on the CPU with the leaf factorised densely in the given order, the reverse order and the order of the all-tail cut measures
48.6, 56.7 and 20.3 (tests/test_solve_compressed_reference_cpu.py asserts that each exceeds the margin).  The solve stays, judged with the group's M,
as a strict expected failure; the case's other five right-hand sides, its ways, counts and inertia are asserted as everywhere.
"""
import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import util as u

pytestmark = pytest.mark.gpu

# per group: the smallest power of two >= 4 x the largest measured ratio (see above); never above 64
M = {"measured": 16, "on_trust": 16, "widths": 32, "deterministic": 16, "sweep_launches": 8, "refined": 16, "refined_deterministic": 16, "general": 16,
     "sparse_root": 8, "new_factors": 16}
_KNOBS = ("PIPS_HIP_AUG_SWEEPS", "PIPS_HIP_MF_KONLY", "PIPS_HIP_SWEEP_LAUNCHES", "PIPS_HIP_BORDER_BACKWARD", "PIPS_HIP_SPARSE_ROOT_BAND", "PIPS_HIP_AUG_WITNESS")
_ALL = tuple(range(len(u.ARROWHEAD_RHS)))
# beyond every admissible margin for a reason that lies in the measure, not in a kernel (see above): (path, right-hand side) -> the measured forward_root
_BEYOND_THE_MARGIN = {("width1/all_tail", "b0_zero"): 41.6}
_largest = {}
_expected_failures = []


@pytest.fixture(scope="module", autouse=True)
def _report_groups():
    yield
    for group, r in _largest.items():
        print(f"\nsolve-compressed-group group={group} " + " ".join(f"{name}={v:.4g}" for name, v in r.items()) + f" M={M[group]}")


def _env(monkeypatch, **knobs):
    """the knobs of this module: those given are set, the others unset (before the handle is created and analysed)"""
    for k in _KNOBS:
        v = knobs.get(k[len("PIPS_HIP_"):].lower())
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


class _Handles:
    """LeafBatch + KktSystem of a reference's problem, as test_aug_sweeps_gpu._system (general structure: as test_border_backward_general_structure)"""

    def __init__(self, ref, force_n_head=-1, deterministic=False, sparse_root=False):
        import torch
        self.torch = torch
        s, prob = ref.sys, ref.sys.prob
        self.bt = bt = pa.LeafBatch(s.N, s.S)
        if deterministic:
            bt.set_deterministic(True)
        if sparse_root:
            bt.set_schur_mode(1)
        for b in range(s.N):
            bt.set_block(b, prob.blocks[b]["K"], s.n_primal, prob.blocks[b]["Bt"])
        if force_n_head >= 0:
            bt.set_options(force_n_head=force_n_head)
        bt.analyze(2)
        bt.set_refinement_backward_error(2, 1e-15)
        for b in range(s.N):
            bt.set_values(b, prob.blocks[b]["K"].val)
        if hasattr(prob, "dims"):
            self.kkt = pa.KktSystem(bt, s.n0, s.my0, s.myl, s.mzl, A0=prob.A0 if s.my0 else None, F0=prob.F0 if s.myl else None, G0=prob.G0 if s.mzl else None,
                                    sparse_root=sparse_root)
            if s.mz0:
                self.kkt.set_root_inequalities(prob.C0)
                self.kkt.set_zdiag0(torch.tensor(prob.z_diag0, device="cuda"))
            self.zdl = torch.tensor(prob.z_diag_link, device="cuda") if s.mzl else None
        else:
            self.kkt = pa.KktSystem(bt, s.n0, 0, s.myl, 0, F0=prob.F0, sparse_root=sparse_root)
            self.zdl = None
        self.diag = np.concatenate([blk["diag"] for blk in prob.blocks])
        self.xd0 = torch.tensor(s.x_diag0, device="cuda")

    def factorize(self, ref):
        """with the leaf diagonals of the reference's system (its diag_scale times the problem's, rounded once)"""
        self.kkt.factorize(self.torch.tensor(ref.sys.diag_scale * self.diag, device="cuda"), self.xd0, self.zdl)
        assert [self.bt.inertia(b) for b in range(ref.sys.N)] == ref.leaf_inertia and all(t[2] == 0 for t in ref.leaf_inertia)
        assert self.kkt.root_inertia() == ref.root_inertia == (ref.sys.n0, ref.sys.S - ref.sys.n0, 0)

    def solve(self, ref, k):
        """right-hand side k of the reference: (x0, xl, way)"""
        b0, bl = self.torch.tensor(ref.B0[k], device="cuda"), self.torch.tensor(ref.BL[k], device="cuda")
        self.kkt.solve_compressed(b0, bl)
        self.bt.sync()
        return b0.cpu().numpy(), bl.cpu().numpy(), self.kkt.last_solve_path()

    def close(self):
        self.kkt.close()
        self.bt.close()


def _judge(ref, k, x0, xl, group, path, way):
    r = {name: float(v[0]) for name, v in ref.ratios(x0, xl, k).items()}
    if (path, u.ARROWHEAD_RHS[k]) in _BEYOND_THE_MARGIN:
        # the strict expected failure: everything else of the case is asserted as usual, this predicate alone is expected to reject
        print(f"solve-compressed-ratio group={group}(beyond the margin) path={path}/{u.ARROWHEAD_RHS[k]} way={way} " + " ".join(f"{name}={v:.4g}" for name, v in r.items()))
        assert all(np.isfinite(v) for v in r.values())
        assert not ref.accepts(x0, xl, M[group], k)[0], "within the margin now: take the case out of _BEYOND_THE_MARGIN"
        _expected_failures.append((path, u.ARROWHEAD_RHS[k]))
        return
    print(f"solve-compressed-ratio group={group} path={path}/{u.ARROWHEAD_RHS[k]} way={way} " + " ".join(f"{name}={v:.4g}" for name, v in r.items()))
    old = _largest.setdefault(group, dict.fromkeys(r, 0.0))
    for name, v in r.items():
        old[name] = max(old[name], v)
    if ref.is_zero_rhs[k]:
        assert not x0.any() and not xl.any(), path
    assert M[group] <= u.UNREFINED_M_CAP
    assert ref.accepts(x0, xl, M[group], k)[0], (path, way, r)


def _solve_and_judge(h, ref, group, path, order=_ALL):
    """every right-hand side in the given order, each judged; the ways taken"""
    ways, sols = [], []
    for k in order:
        x0, xl, way = h.solve(ref, k)
        ways.append(way)
        sols.append((k, x0, xl, way))
    for k, x0, xl, way in sols:
        _judge(ref, k, x0, xl, group, path, way)
    return ways


# ---- 1. sweeps, every solve measured -----------------------------------------------------------------------------------------------------
_MEASURED = {"small": ("small", {}), "dense_tail": ("dense_tail", {}), "time_coupled": ("time_coupled", {}),
             "time_coupled_all_head": ("time_coupled", dict(force_head=True)), "time_coupled_k_only_fronts": ("time_coupled", dict(mf_konly="1"))}


@pytest.mark.parametrize("shape", list(_MEASURED))
def test_sweeps_measured(shape, monkeypatch):
    case, kw = _MEASURED[shape]
    _env(monkeypatch, aug_sweeps="1", mf_konly=kw.get("mf_konly"))
    ref = u.arrowhead_reference(case)
    h = _Handles(ref, force_n_head=ref.sys.n_leaf if kw.get("force_head") else -1)
    info = h.bt.info()
    assert info["augmented_sweeps"] == 1 and info["blocks_with_k_only_fronts"] == (ref.sys.N if "mf_konly" in kw else 0), info
    assert (info["m"] == 0) == (shape == "time_coupled_all_head") and (shape != "dense_tail" or info["tail_border_entries"] > 0), info
    h.factorize(ref)
    ways = _solve_and_judge(h, ref, "measured", shape)
    counts = h.kkt.solve_check_counts()
    h.close()
    assert ways == [3] * len(_ALL) and counts == (len(_ALL), 0), (ways, counts)


# ---- 2. sweeps on trust --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every,order,want", [(0, (0, 1, 2, 3, 4, 5), [3, 2, 2, 2, 2, 2]), (2, (0, 1, 2, 3, 4, 5), [3, 2, 3, 2, 3, 2]), (2, (1, 0, 3, 2, 5, 4), [3, 2, 3, 2, 3, 2])],
                         ids=["witness_only", "every_second", "every_second_swapped"])
@pytest.mark.parametrize("case", u.ARROWHEAD_WAY2_CASES)
def test_sweeps_on_trust(case, every, order, want, monkeypatch):
    _env(monkeypatch, aug_sweeps="1")
    ref = u.arrowhead_reference(case)
    h = _Handles(ref)
    assert h.bt.info()["augmented_sweeps"] == 1
    h.kkt.set_solve_check(every)
    h.factorize(ref)
    ways = _solve_and_judge(h, ref, "on_trust", f"{case}/check{every}", order)
    counts = h.kkt.solve_check_counts()
    h.close()
    assert ways == want and counts == (want.count(3), 0), (ways, counts)


# ---- 3. border widths at the tile and chunk edges -------------------------------------------------------------------------------------------
_WIDTH_CASES = [f"width{S}" for S in u.ARROWHEAD_SCHUR_WIDTHS] + ["hetero129"]


@pytest.mark.parametrize("cut", ["model", "all_tail"])
@pytest.mark.parametrize("case", _WIDTH_CASES)
def test_border_widths(case, cut, monkeypatch):
    """all_tail (force_n_head = 0): all of K_i is dense tail, so every border row goes through k_tail_border_fwd - the model's cut leaves the
    170-variable blocks without a tail, and a border tile's last row skipped there showed on hetero129 alone"""
    _env(monkeypatch, aug_sweeps="1")
    ref = u.arrowhead_reference(case)
    h = _Handles(ref, force_n_head=0 if cut == "all_tail" else -1)
    info = h.bt.info()
    assert info["augmented_sweeps"] == 1 and (cut == "model" or (info["n_head"] == 0 and info["m"] == ref.n_leaves and info["tail_border_entries"] > 0)), info
    h.factorize(ref)
    del _expected_failures[:]
    ways = _solve_and_judge(h, ref, "widths", f"{case}/{cut}")
    counts = h.kkt.solve_check_counts()
    h.close()
    assert ways == [3] * len(_ALL) and counts == (len(_ALL), 0), (ways, counts)
    assert _expected_failures == [key for key in _BEYOND_THE_MARGIN if key[0] == f"{case}/{cut}"]
    if _expected_failures:
        pytest.xfail("one Schur row: x_ref0's error in that one number is 2.4e-15 of it on this right-hand side (1.2e-13 on the first one); measured forward_root %.1f" %
                     _BEYOND_THE_MARGIN[_expected_failures[0]])


# ---- 4. deterministic mode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "time_coupled", "width129"])
def test_deterministic_sweeps(case, monkeypatch):
    _env(monkeypatch, aug_sweeps="1")
    ref = u.arrowhead_reference(case)
    h = _Handles(ref, deterministic=True)
    assert h.bt.info()["augmented_sweeps"] == 1, h.bt.info()
    h.factorize(ref)
    first = h.solve(ref, 0)
    ways = _solve_and_judge(h, ref, "deterministic", case)
    counts = h.kkt.solve_check_counts()
    h.close()
    assert first[2] == 3 and ways == [3] * len(_ALL) and counts == (len(_ALL) + 1, 0), (first[2], ways, counts)
    # (the one comparison with the device's own earlier output: the same right-hand side, solved twice, the same bits)
    h2 = _Handles(ref, deterministic=True)
    h2.factorize(ref)
    again = h2.solve(ref, 0)
    h2.close()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


# ---- 5. launch-per-column tail sweeps ----------------------------------------------------------------------------------------------------------
def test_sweep_launches_keep_the_refined_ways(monkeypatch):
    _env(monkeypatch, aug_sweeps="1", sweep_launches="1")
    ref = u.arrowhead_reference("dense_tail")
    h = _Handles(ref)
    info = h.bt.info()
    assert info["augmented_sweeps"] == 0 and info["ntc"] > 0, info
    h.factorize(ref)
    ways = _solve_and_judge(h, ref, "sweep_launches", "dense_tail")
    counts = h.kkt.solve_check_counts()
    h.close()
    assert ways == [0] * len(_ALL) and counts == (0, 0), (ways, counts)      # (the Ltsolve from the factor needs the single-launch sweeps as well)


# ---- 6. the refined ways as the baseline -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border_backward", ["0", "1"])
@pytest.mark.parametrize("case", ["dense_tail", "time_coupled"])
def test_refined_ways(case, border_backward, monkeypatch):
    _env(monkeypatch, aug_sweeps="0", border_backward=border_backward)
    ref = u.arrowhead_reference(case)
    h = _Handles(ref)
    info = h.bt.info()
    assert info["augmented_sweeps"] == 0 and info["ltsolve_from_augmented_factor"] == int(border_backward), info
    h.factorize(ref)
    ways = _solve_and_judge(h, ref, "refined", f"{case}/border_backward{border_backward}")
    counts = h.kkt.solve_check_counts()
    h.close()
    print(f"solve-compressed-ways {case}/border_backward{border_backward} {ways}")
    # (way 1 needs a refined Lsolve that took no refinement step in the same call: on these cases every one is)
    assert ways == [int(border_backward)] * len(_ALL) and counts == (0, 0), (ways, counts)


@pytest.mark.parametrize("border_backward", ["0", "1"])
@pytest.mark.parametrize("case", ["dense_tail", "time_coupled"])
def test_refined_ways_deterministic(case, border_backward, monkeypatch):
    """the deterministic Lsolve without the sweeps (lsolve_det in csrc/kkt.hip.h): refined leaf solve, k_border_rowdot into the group buffers
    (g_btm_grp), k_reduce_groups; the Ltsolve goes through k_border_entry_products + k_gather_slots.  layout.cpp's border_backward_ok needs
    !deterministic, so PIPS_HIP_BORDER_BACKWARD=1 changes nothing here: way 0 on every solve."""
    _env(monkeypatch, aug_sweeps="0", border_backward=border_backward)
    ref = u.arrowhead_reference(case)
    path = f"{case}/border_backward{border_backward}/deterministic"
    h = _Handles(ref, deterministic=True)
    info = h.bt.info()
    assert info["augmented_sweeps"] == 0 and info["ltsolve_from_augmented_factor"] == 0, info
    h.factorize(ref)
    first = h.solve(ref, 0)
    ways = _solve_and_judge(h, ref, "refined_deterministic", path)
    repeated = h.solve(ref, 0)
    counts = h.kkt.solve_check_counts()
    h.close()
    assert first[2] == repeated[2] == 0 and ways == [0] * len(_ALL) and counts == (0, 0), (first[2], repeated[2], ways, counts)
    # (the one comparison with the device's own earlier output: the same right-hand side, solved again on this handle and on a second one)
    assert np.array_equal(first[0], repeated[0]) and np.array_equal(first[1], repeated[1])
    h2 = _Handles(ref, deterministic=True)
    h2.factorize(ref)
    again = h2.solve(ref, 0)
    h2.close()
    assert again[2] == 0 and np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


# ---- 7. the general structure with sweeps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["general", "general_mz0"])
def test_general_structure_sweeps(case, monkeypatch):
    _env(monkeypatch, aug_sweeps="1")
    ref = u.arrowhead_reference(case)
    assert ref.sys.mz0 == (4 if case == "general_mz0" else 0) and ref.sys.my0 and ref.sys.mzl
    h = _Handles(ref)
    assert h.bt.info()["augmented_sweeps"] == 1, h.bt.info()
    h.factorize(ref)
    ways = _solve_and_judge(h, ref, "general", case)
    counts = h.kkt.solve_check_counts()
    h.close()
    assert ways == [3] * len(_ALL) and counts == (len(_ALL), 0), (ways, counts)


# ---- 8. sparse root ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", ["1", "0"])
@pytest.mark.parametrize("case", ["two_link_6", "two_link_30"])
def test_sparse_root(case, band, monkeypatch):
    _env(monkeypatch, aug_sweeps="1", sparse_root_band=band)
    ref = u.arrowhead_reference(case)
    h = _Handles(ref, sparse_root=True)
    assert h.kkt.sparse_root_info()["order"] == {"1": "band", "0": "amd"}[band]
    sweeps = h.bt.info()["augmented_sweeps"]
    h.factorize(ref)
    ways = _solve_and_judge(h, ref, "sparse_root", f"{case}/band{band}")
    counts = h.kkt.solve_check_counts()
    h.close()
    print(f"solve-compressed-ways {case}/band{band} augmented_sweeps={sweeps} {ways}")
    assert sweeps == 1 and ways == [3] * len(_ALL) and counts == (len(_ALL), 0), (sweeps, ways, counts)


# ---- 9. one handle, new factors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "time_coupled"])
def test_one_handle_new_factors(case, monkeypatch):
    _env(monkeypatch, aug_sweeps="1")
    first, second = u.arrowhead_reference(case), u.arrowhead_reference(case + "_scaled")
    assert second.sys.diag_scale == u.ARROWHEAD_SECOND_DIAG_SCALE and second.sys.prob is first.sys.prob
    h = _Handles(first)
    assert h.bt.info()["augmented_sweeps"] == 1
    ways = []
    for ref, what, order in ((first, "first", (0, 3, 4)), (second, "second", (1, 3, 4))):
        h.factorize(ref)
        ways += _solve_and_judge(h, ref, "new_factors", f"{case}/{what}", order)
    counts = h.kkt.solve_check_counts()
    h.close()
    assert ways == [3] * 6 and counts == (6, 0), (ways, counts)
