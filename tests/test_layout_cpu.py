"""The host layout pass of a batch analysis (csrc/layout.cpp) on the CPU: pips_layout_probe runs the symbolic analysis and the layout
as the engine does, checks the properties the kernels rely on itself (return code 0) and reports totals, which must agree with the
symbolic probe of the single blocks.  Sizes are small: the file takes about five seconds on 16 CPU threads."""
import ctypes as C

import numpy as np
import pytest

import pips_ipmpp_amd as pa
import families
from tests.util import Problem

lib = pa.capi.lib
lib.pips_layout_probe.restype = C.c_int
KEYS = ("arena", "xw", "uarena", "n_sn", "levels", "spine_levels", "front_launches", "fronts_devmem", "bb_batches", "bb_stage", "tail_single",
        "border_backward", "aug_sweeps", "slots", "vslots", "n", "mf", "schur_mode", "bb_doubles", "mfU", "spine_sn")
PLENTY = 64 << 30


def probe(blocks, S, deterministic=False, free_bytes=PLENTY):
    """blocks: [(K, n_primal, Bt or None)]"""
    nb = len(blocks)
    ip = C.POINTER(C.c_int)
    keep = []

    def arr(seq):
        a = (ip * nb)()
        for i, v in enumerate(seq):
            if v is not None:
                v = np.ascontiguousarray(v, dtype=np.int32)
                keep.append(v)
                a[i] = v.ctypes.data_as(ip)
        return a

    n = np.array([K.nrows for K, _, _ in blocks], np.int32)
    npr = np.array([p for _, p, _ in blocks], np.int32)
    what = np.zeros(len(KEYS), np.int64)
    rc = lib.pips_layout_probe(nb, n.ctypes.data_as(ip), npr.ctypes.data_as(ip), arr(K.rowptr for K, _, _ in blocks), arr(K.colidx for K, _, _ in blocks),
                               S, arr(None if B is None else B.rowptr for _, _, B in blocks), arr(None if B is None else B.colidx for _, _, B in blocks),
                               int(deterministic), C.c_longlong(free_bytes), what.ctypes.data_as(C.POINTER(C.c_int64)), len(KEYS))
    if rc:
        raise pa.PipsHipError(f"pips_layout_probe failed (code {rc}): {lib.pips_hip_last_error().decode()}")
    return dict(zip(KEYS, (int(v) for v in what)))


def against_single_blocks(blocks, w):
    """sums over the symbolic probes of the single blocks (with the border where it rides in the panels: Schur mode 1)"""
    infos = [pa.symbolic_probe(K, p, B if w["schur_mode"] == 1 else None) for K, p, B in blocks]
    assert w["n"] == sum(i["n"] for i in infos) == sum(K.nrows for K, _, _ in blocks)
    assert w["n_sn"] == sum(i["n_sn"] for i in infos)
    assert w["arena"] * 8 == sum(i["arena_bytes"] for i in infos)
    assert w["xw"] >= w["n"] and w["levels"] + w["spine_levels"] == max(i["n_levels"] for i in infos)
    assert w["vslots"] >= 0 and (w["mf"] == 1 or (w["front_launches"] == 0 and w["bb_batches"] == 0))
    return infos


def random_blocks(N, n_i, n0=6, myl=6, rho=0.03, seed=3):
    prob = Problem(seed, N, n_i, n_i // 2, n0, myl, rho)
    return [(b["K"], n_i, b["Bt"]) for b in prob.blocks], prob.S


def chain_blocks(N=8, n_i=2000, L=6, n0=16):
    blks, F0, my_i, myl = families.time_coupled_blocks(N, n_i, L, n0, 12, 10, 7)
    out = []
    for W, T, F in blks:
        K, _ = pa.kkt_leaf_assemble(n_i, W)
        out.append((K, n_i, pa.border_assemble(n_i, my_i, 0, n0, 0, A=T, F=F)))
    return out, n0 + myl


@pytest.fixture(scope="module")
def chain():
    return chain_blocks()


@pytest.fixture(scope="module")
def rnd():
    return random_blocks(4, 600)


@pytest.mark.parametrize("deterministic", [False, True])
def test_time_coupled_blocks(chain, deterministic):
    blocks, S = chain
    w = probe(blocks, S, deterministic)
    against_single_blocks(blocks, w)
    assert w["mf"] == 1 and w["front_launches"] > 0 and w["fronts_devmem"] == 0
    assert w["bb_batches"] > 0 and 3072 <= w["bb_stage"] <= 6144 and w["bb_doubles"] > 0   # the chain's border takes the split
    assert w["tail_single"] == 0 or not deterministic
    assert w["spine_sn"] == 0   # (the multifrontal head and deterministic mode take no spine)


@pytest.mark.parametrize("deterministic", [False, True])
def test_random_sparsity_blocks(rnd, deterministic):
    blocks, S = rnd
    w = probe(blocks, S, deterministic)
    against_single_blocks(blocks, w)
    assert w["uarena"] > 0   # random sparsity: a dense tail in every block
    assert w["tail_single"] == (0 if deterministic else 1)
    assert w["border_backward"] == 0 or not deterministic


def test_tail_single_both_sides(rnd):
    blocks, S = rnd
    assert probe(blocks, S)["tail_single"] == 1                 # up to 16 blocks, room for the scratch copy
    assert probe(blocks, S, free_bytes=0)["tail_single"] == 0   # no room
    many, S18 = random_blocks(18, 400)
    w = probe(many, S18)
    against_single_blocks(many, w)
    assert w["tail_single"] == 0                                # more than 16 blocks: the column launches


def test_switches(chain, rnd, monkeypatch):
    blocks, S = chain
    base = probe(blocks, S)
    monkeypatch.setenv("PIPS_HIP_TAIL_SINGLE", "1")
    many, S18 = random_blocks(18, 400)
    assert probe(many, S18)["tail_single"] == 1
    monkeypatch.delenv("PIPS_HIP_TAIL_SINGLE")
    monkeypatch.setenv("PIPS_HIP_MF", "0")
    for blk, s in ((blocks, S), rnd):
        w = probe(blk, s)
        against_single_blocks(blk, w)
        assert w["mf"] == 0 and w["mfU"] == 0 and w["tail_single"] == 0
    monkeypatch.delenv("PIPS_HIP_MF")
    for budget in (12000, 8000, 6000, 4000, 3000, 2000, 1500, 1000):   # shrink the LDS budget until a front's update matrix no longer fits
        monkeypatch.setenv("PIPS_HIP_MF_LDS", str(budget))
        w = probe(blocks, S)
        against_single_blocks(blocks, w)
        if w["fronts_devmem"] > 0 or not w["mf"]:
            break
    assert w["mf"] == 1 and w["fronts_devmem"] > 0 and w["arena"] == base["arena"]
    monkeypatch.delenv("PIPS_HIP_MF_LDS")
    monkeypatch.setenv("PIPS_HIP_MF_KONLY", "1")   # fronts on the rows of K only: smaller update matrices, the same panels
    w = probe(blocks, S)
    against_single_blocks(blocks, w)
    assert w["mf"] == 1 and w["bb_batches"] == base["bb_batches"] and 0 < w["mfU"] < base["mfU"]
    assert probe(blocks, S, deterministic=True)["mfU"] == base["mfU"]   # (not in deterministic mode)


def test_blocks_without_border(rnd):
    blocks, _ = rnd
    w = probe([(K, p, None) for K, p, _ in blocks], 0)
    assert w["bb_batches"] == 0 and w["border_backward"] == 0 and w["aug_sweeps"] == 0 and w["schur_mode"] == 1


def test_input_errors(rnd):
    blocks, S = rnd
    K, p, Bt = blocks[1]
    rp, ci = np.asarray(K.rowptr), np.asarray(K.colidx)
    row = p // 2
    keep = np.ones(len(ci), bool)
    keep[rp[row] + np.nonzero(ci[rp[row]:rp[row + 1]] == row)[0]] = False
    rp2 = rp.copy()
    rp2[row + 1:] -= 1
    bad = pa.Csr(K.nrows, K.ncols, rp2, ci[keep], np.asarray(K.val)[keep])
    with pytest.raises(pa.PipsHipError, match=f"block 1 row {row} has no explicit diagonal entry"):
        probe([blocks[0], (bad, p, Bt)], S)
    upper = pa.Csr(2, 2, [0, 2, 3], [0, 1, 1], [1.0, 2.0, 3.0])
    with pytest.raises(pa.PipsHipError, match="block 1: "):
        probe([blocks[0], (upper, -1, None)], S)
