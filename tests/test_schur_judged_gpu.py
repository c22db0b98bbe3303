"""The Schur contribution SC -= sum_i Br_i^T K_i^-1 Br_i of a leaf batch judged against a long-double reference, at the border widths where
the kernels switch: 32, the chunk of schur_by_solves, and 128, the tile of the border strip, the Schur SYRK and k_pack_*.

The contribution is unrefined on the device in both Schur modes (mode 1 forms it from the factors, mode 2 goes through solve_once /
solve_once_multi, which carry no refinement), so it is measured as tests/test_unrefined_sweeps_gpu.py measures the sweeps, over the lower triangle:

    max|SC_dev - SC*| <= M max(err_ref0, 2^-53 max|SC*|)          err_ref0 = max|SC_ref0 - SC*|

SC* comes from the oracle's twice refined solves of the densified border columns, Br^T X and the sum over the blocks accumulated in long double
and rounded once; SC_ref0 is the oracle's plain FP64 algorithm (add_term_to_schur_compl_blocked over unrefined solves): util.SchurReference.
tests/test_schur_reference_cpu.py proves for every problem that the oracle perturbs no pivot and that the predicate rejects, at M = 64, SC_ref0
rounded to float32, a block or a border column left out, a block scaled by 1 + 1e-6, the last row past a 128-row boundary zeroed and a square
taken in the wrong order.  Nothing is compared with the device's earlier output (bit-identity of deterministic mode aside).

Problems (util.SCHUR_PROBLEMS): n_i in {170, 400}, my_i = n_i // 2 - leaves of dimension 255 and 600, 2 and 5 tail tiles when all of K is in the
tail - primal diagonals within 1e-2 .. 1e2, S split n0 = S // 2, myl = S - n0, every border column non-empty in every block (so S is the width
the kernels see) except in the heterogeneous case.  The model's own cut is head 344 + tail 256 (two tiles) at n_i = 400 and all head at
n_i = 170 (blocks that small get no tail from the cost model): asserted as such.  Every case asserts schur_mode(), the cut and the tail tiles
through info(), and the inertia (n_i, my_i, 0) of every block.
  1. S in {1, 31, 32, 33, 127, 128, 129, 257} x modes 1 (augmented) and 2 (blocked solves) x cuts model / all head / all tail, one block; S = 32,
     33 and 129 also with three blocks accumulating into one SC (atomics: the order of the additions varies).  S <= 176 takes the border split of
     the multifrontal head (launch_border_schur; info()["blocks_with_border_split"]), S = 257 does not (k_root_assemble alone).
  2. the tail launch form, mode 1, S in {33, 129}, cuts model and all tail: PIPS_HIP_TAIL_SINGLE=0 (a launch per step) and =1 (k_tail_ldl).
     info() does not say which ran; the phase timers do (one tail_update record and no tail_diag / tail_trsm record: the single launch).
  3. head variants, mode 1, model cut, S in {33, 129}: PIPS_HIP_MF=0 (scatter head), PIPS_HIP_MF_KONLY=1 (fronts on the rows of K, k_border_rows),
     the default (border split) and PIPS_HIP_MF_SPLIT=0 (fronts with full update matrices at the same widths) - info() is asserted for each.
  4. PIPS_HIP_DETERMINISTIC=1, modes 1 and 2, S in {32, 33, 129}, three blocks: judged like the others, and two fresh handles agree to the bit.
  5. heterogeneous borders, three blocks, S = 129: block 1 has only the n0 border columns, block 2 only the myl ones (bmaps that differ and
     are proper subsets); the batch, and every block factored alone and judged by the per-block quotient (a failure names the block; nothing
     outside the block's bmap may be touched).
  6. sparse root, S = 129, three blocks (all columns, and the heterogeneous borders): KktSystem(..., sparse_root=True).schur_sparse_to_host()
     after factorize.  The sparse-root handle gives no unfinalised view, so the finalised matrix is judged, against a reference that holds the
     constant root entries and diagonals of finalize too (SchurReference(finalized=True)).  The position tables (d_sctab) at a width that
     crosses a tile.
  7. second factorisation, S = 129, modes 1 and 2: set_diagonals with the same diagonals, SC zeroed, factor, judge; then a third time into the SC
     as it stands - judged against 2 SC* (the kernels accumulate into SC, they do not overwrite it).

Measured on an MI355X, largest ratio max|SC_dev - SC*| / max(err_ref0, 2^-53 max|SC*|) over the cases of a path (model / all head / all tail
where a path has the three cuts; err_ref0 lies within a few units of 2^-53 max|SC*| in every problem, so these are nearly ratios to the floor):

    path                                                            mode 1                      mode 2
    1. widths, one block                                            1.26 / 1.07 / 1.92          1.34 / 1.13 / 1.90
       widths, three blocks                                         1.33 / 1.22 / 2.02          0.97 / 0.88 / 1.64
    2. tail form, a launch per step (model / all tail)              1.26 / 1.69
       tail form, single launch (model / all tail)                  1.49 / 1.66
    3. head: scatter / K-only fronts / default / no split           1.77 / 1.38 / 1.30 / 1.17
    4. deterministic mode                                           1.31                        1.62
    5. heterogeneous borders, the batch                             1.24 / 1.22 / 1.95          0.81 / 0.88 / 1.51
       heterogeneous borders, every block alone                     1.05 / 1.07 / 1.66          0.74 / 0.74 / 1.30
    6. sparse root (finalised)                                      1.40
    7. first / second factorisation / accumulated twice             1.07 / 1.07 / 1.07          0.73 / 0.74 / 0.73

Largest ratio 2.02 in mode 1 and 1.90 in mode 2: they differ by less than 4 x, so both modes share one margin.  M = 16, the smallest power of
two that is at least 4 x 2.02 = 8.07.  (The device's elimination order against the oracle's and, in mode 1, Br^T K^-1 Br formed from the
factors instead of by solves: all of it stays within two units of the oracle's own unrefined error.)
"""
import numpy as np
import pytest

import pips_ipmpp_amd as pa
from tests import util as u
from tests.test_layout_cpu import probe as layout_probe
from tests.util import hip_lower_as_rowmajor

pytestmark = pytest.mark.gpu

M = {1: 16, 2: 16}       # per Schur mode: the smallest power of two >= 4 x the largest measured ratio (2.02), see above; never above 64
_KNOBS = ("PIPS_HIP_TAIL_SINGLE", "PIPS_HIP_MF", "PIPS_HIP_MF_KONLY", "PIPS_HIP_MF_SPLIT", "PIPS_HIP_DETERMINISTIC")
_CUTS = ("model", "all_head", "all_tail")


def _env(monkeypatch, **knobs):
    """the knobs of this module: those given are set, the others unset (before the handle is created)"""
    for k in _KNOBS:
        v = knobs.get(k[len("PIPS_HIP_"):].lower())
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _batch(prob, mode, cut, blocks=None, timing=False):
    blocks = list(range(prob.N)) if blocks is None else blocks
    bt = pa.LeafBatch(len(blocks), prob.S)
    bt.set_schur_mode(mode)
    for i, b in enumerate(blocks):
        bt.set_block(i, prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"])
    bt.set_options(force_n_head={"model": -1, "all_head": prob.n_leaf, "all_tail": 0}[cut])
    bt.analyze(2)
    for i, b in enumerate(blocks):
        bt.set_values(i, prob.blocks[b]["K"].val)
    if timing:
        bt.set_timing(True)
    return bt


def _factor(bt, prob, SC=None):
    """factor into SC (a zeroed device buffer unless one is given); the row-major lower triangle on the host"""
    import torch
    S = prob.S
    if SC is None:
        SC = torch.zeros(S * S, dtype=torch.float64, device="cuda")
    bt.factor(SC, S)
    bt.sync()
    return SC, hip_lower_as_rowmajor(SC.cpu().numpy(), S)


def _assert_path(bt, prob, mode, cut, nblocks=None):
    """schur_mode(), the cut and the tail tiles by info(), the inertia of every block"""
    nb = prob.N if nblocks is None else nblocks
    n = prob.n_leaf
    info = bt.info()
    assert bt.schur_mode() == mode
    if cut == "all_head" or (cut == "model" and prob.n_i == 170):
        assert info["n_head"] == nb * n and info["m"] == 0 and info["ntc"] == 0, info
    elif cut == "all_tail":
        assert info["n_head"] == 0 and info["m"] == nb * n and info["ntc"] == -(-n // 128) > 1, info      # 2 and 5 tiles
    else:
        assert info["n_head"] == nb * 344 and info["m"] == nb * 256 and info["ntc"] == 2, info            # head kernels and a tail of two tiles
    assert [bt.inertia(i) for i in range(nb)] == [(prob.n_i, prob.my_i, 0)] * nb
    return info


def _layout(prob):
    return layout_probe([(b["K"], prob.n_i, b["Bt"]) for b in prob.blocks], prob.S)


def _judge(ref, got, mode, path, times=1):
    r = ref.ratio(got, times)
    print(f"schur-ratio path={path} ratio={r:.4g}")
    assert M[mode] <= u.UNREFINED_M_CAP
    assert ref.accepts(got, M[mode], times), (path, r, ref.err_ref0, ref.scale)


def _key_id(key):
    return f"{key[0]}-S{key[1]}-N{key[2]}" + ("-hetero" if key[3] == "hetero" else "")


# ---- 1. border widths x Schur modes x cuts ---------------------------------------------------------------------------------------------------
_WIDTH_KEYS = [k for k in u.SCHUR_PROBLEMS if k[3] == "full" and (k[2] == 1 or k[1] in (33, 129))]


@pytest.mark.parametrize("cut", _CUTS)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("key", _WIDTH_KEYS, ids=[_key_id(k) for k in _WIDTH_KEYS])
def test_border_widths(key, mode, cut, monkeypatch):
    _env(monkeypatch)
    ref = u.schur_reference(key)
    prob = ref.prob
    bt = _batch(prob, mode, cut)
    _, got = _factor(bt, prob)
    info = _assert_path(bt, prob, mode, cut)
    if mode == 1:
        assert info["blocks_with_border_split"] == (prob.N if prob.S <= 176 else 0) and (cut == "all_tail" or info["multifrontal_head"] == 1), info
    bt.close()
    _judge(ref, got, mode, f"widths/N{prob.N}/mode{mode}/{cut}")


# ---- 2. the tail launch form -----------------------------------------------------------------------------------------------------------------
_S_33_129 = [k for k in u.SCHUR_PROBLEMS if k[3] == "full" and k[2] == 1 and k[1] in (33, 129)]


@pytest.mark.parametrize("single", ["0", "1"], ids=["launches", "single"])
@pytest.mark.parametrize("cut", ["model", "all_tail"])
@pytest.mark.parametrize("key", _S_33_129, ids=[_key_id(k) for k in _S_33_129])
def test_tail_launch_form(key, cut, single, monkeypatch):
    _env(monkeypatch, tail_single=single)
    ref = u.schur_reference(key)
    prob = ref.prob
    bt = _batch(prob, 1, cut, timing=True)
    _, got = _factor(bt, prob)
    info = _assert_path(bt, prob, 1, cut)
    tm = bt.get_timing()
    if cut == "model":     # (the host layout pass of the same blocks under the same knobs: the model's cut only, it takes no forced one)
        assert _layout(prob)["tail_single"] == (1 if single == "1" and info["m"] > 0 else 0)
    if info["m"] > 0:      # (the model's cut at n_i = 170 leaves no tail: nothing to launch either way)
        if single == "1":
            assert tm["tail_update"][1] == 1 and tm["tail_diag"][1] == 0 and tm["tail_trsm"][1] == 0, tm
        else:
            assert tm["tail_diag"][1] >= 1 and tm["tail_trsm"][1] >= 1, tm       # a launch per step
    bt.close()
    _judge(ref, got, 1, f"tail_form/{'single' if single == '1' else 'launches'}/{cut}")


# ---- 3. head variants ------------------------------------------------------------------------------------------------------------------------
_HEADS = {"scatter": dict(mf="0"), "k_only_fronts": dict(mf_konly="1"), "default": {}, "no_split": dict(mf_split="0")}


@pytest.mark.parametrize("head", list(_HEADS))
@pytest.mark.parametrize("key", _S_33_129, ids=[_key_id(k) for k in _S_33_129])
def test_head_variants(key, head, monkeypatch):
    _env(monkeypatch, **_HEADS[head])
    ref = u.schur_reference(key)
    prob = ref.prob
    bt = _batch(prob, 1, "model")
    _, got = _factor(bt, prob)
    info = _assert_path(bt, prob, 1, "model")
    want = {"scatter": (0, 0, 0), "k_only_fronts": (1, 1, 1), "default": (1, 1, 0), "no_split": (1, 0, 0)}[head]
    assert (info["multifrontal_head"], info["blocks_with_border_split"], info["blocks_with_k_only_fronts"]) == want, info
    # n_bb, the batches of launch_border_schur, by the host layout pass of the same blocks under the same knobs: the all-head leaves of
    # n_i = 170 have fronts with border rows (n_bb > 0 with the split), the head of n_i = 400 is simple leaves only (no front, n_bb = 0)
    assert (_layout(prob)["bb_batches"] > 0) == (prob.n_i == 170 and head in ("default", "k_only_fronts"))
    bt.close()
    _judge(ref, got, 1, f"head/{head}")


# ---- 4. deterministic mode -------------------------------------------------------------------------------------------------------------------
_THREE = [k for k in u.SCHUR_PROBLEMS if k[3] == "full" and k[2] == 3]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("key", _THREE, ids=[_key_id(k) for k in _THREE])
def test_deterministic_mode(key, mode, monkeypatch):
    _env(monkeypatch, deterministic="1")
    ref = u.schur_reference(key)
    prob = ref.prob
    got = []
    for _ in range(2):      # fresh handles
        bt = _batch(prob, mode, "model")
        got.append(_factor(bt, prob)[1])
        _assert_path(bt, prob, mode, "model")
        bt.close()
    _judge(ref, got[0], mode, f"deterministic/mode{mode}")
    assert np.array_equal(got[0], got[1])


# ---- 5. heterogeneous borders ----------------------------------------------------------------------------------------------------------------
_HETERO = [k for k in u.SCHUR_PROBLEMS if k[3] == "hetero"]


@pytest.mark.parametrize("cut", _CUTS)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("key", _HETERO, ids=[_key_id(k) for k in _HETERO])
def test_heterogeneous_borders(key, mode, cut, monkeypatch):
    _env(monkeypatch)
    ref = u.schur_reference(key)
    prob = ref.prob
    assert [len(m) for m in ref.bmaps] == [129, 64, 65]
    bt = _batch(prob, mode, cut)
    _, got = _factor(bt, prob)
    _assert_path(bt, prob, mode, cut)
    bt.close()
    _judge(ref, got, mode, f"hetero/mode{mode}/{cut}")
    for b in range(prob.N):         # every block alone: a failure names the block
        bt = _batch(prob, mode, cut, blocks=[b])
        _, one = _factor(bt, prob)
        _assert_path(bt, prob, mode, cut, nblocks=1)
        bt.close()
        r = ref.block_ratio(b, one)
        print(f"schur-ratio path=hetero_block/mode{mode}/{cut} ratio={r:.4g}")
        assert ref.block_accepts(b, one, M[mode]), (b, r)


# ---- 6. sparse root --------------------------------------------------------------------------------------------------------------------------
_S129_THREE = [k for k in u.SCHUR_PROBLEMS if k[1:3] == (129, 3)]


@pytest.mark.parametrize("key", _S129_THREE, ids=[_key_id(k) for k in _S129_THREE])
def test_sparse_root_value_array(key, monkeypatch):
    import torch
    _env(monkeypatch)
    ref = u.schur_reference(key, finalized=True)
    prob = ref.prob
    bt = _batch(prob, 1, "model")
    kkt = pa.KktSystem(bt, prob.n0, 0, prob.myl, 0, F0=prob.F0, sparse_root=True)
    diag = torch.tensor(np.concatenate([b["diag"] for b in prob.blocks]), device="cuda")
    kkt.factorize(diag, torch.tensor(prob.x_diag0, device="cuda"))
    SCs = kkt.schur_sparse_to_host()
    bt.sync()
    _assert_path(bt, prob, 1, "model")
    kkt.close()
    bt.close()
    assert SCs.shape == (prob.S, prob.S) and SCs.nnz <= prob.S * (prob.S + 1) // 2
    got = SCs.toarray()
    assert not np.triu(got, 1).any()                  # a lower-triangular value array
    _judge(ref, got, 1, "sparse_root")


# ---- 7. second factorisation, and accumulation into SC -------------------------------------------------------------------------------------
_S129_ONE = [k for k in u.SCHUR_PROBLEMS if k[1:] == (129, 1, "full")]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("key", _S129_ONE, ids=[_key_id(k) for k in _S129_ONE])
def test_second_factorisation_and_accumulation(key, mode, monkeypatch):
    _env(monkeypatch)
    ref = u.schur_reference(key)
    prob = ref.prob
    diag = np.concatenate([b["diag"] for b in prob.blocks])
    bt = _batch(prob, mode, "model")
    SC, got = _factor(bt, prob)
    _judge(ref, got, mode, f"refactor/mode{mode}/first")
    bt.set_diagonals(diag)
    SC.zero_()
    _, got = _factor(bt, prob, SC)
    _judge(ref, got, mode, f"refactor/mode{mode}/second")
    bt.set_diagonals(diag)
    _, got = _factor(bt, prob, SC)                    # into the SC as it stands: twice the contribution
    _assert_path(bt, prob, mode, "model")
    bt.close()
    _judge(ref, got, mode, f"refactor/mode{mode}/accumulated", times=2)
