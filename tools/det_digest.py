"""SHA-256 digests of what deterministic mode computes on one rank - Schur complement, x0, xl, inertia - for the cases of the
deterministic tests (their own shapes and drivers): two builds whose digests agree compute the same bits, and the tests' 1 against
2 / 4 / 8 ranks carry that to several ranks (profiles/detplan_refactor.txt).  Also the wall time of the analysis and of the KktSystem
creation in deterministic mode on the banded problem, where the host plans of csrc/detplan.cpp are built.
usage: [PIPS_HIP_LIBRARY=other/libpipship.so] python tools/det_digest.py [--time-only]      (needs a GPU)"""
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pips_ipmpp_amd as pa  # noqa: E402
from tests import test_deterministic_blocked_schur_gpu as blocked  # noqa: E402
from tests import test_deterministic_gpu as det  # noqa: E402
from tests import test_sparse_root_blocked_gpu as packed  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def report(name, r):
    inertia = np.array([tuple(t) for t in r["inertia"]], np.int64) if "inertia" in r else np.zeros(0, np.int64)
    print(f"{name:24s} SC {sha(r['SC']) if 'SC' in r else '-':32s} x0 {sha(np.array(r['x0']))} xl {sha(np.array(r['xl']))} inertia {sha(inertia)}", flush=True)


def analysis_times(reps=5):
    """ms of LeafBatch.analyze() and of KktSystem(...) in deterministic mode on the banded problem, per repetition"""
    prob = det._problem("banded")
    out = []
    for _ in range(reps):
        bt = pa.LeafBatch(prob.N, prob.S)
        bt.set_deterministic(True)
        for b in range(prob.N):
            bt.set_block(b, prob.blocks[b]["K"], prob.n_i, prob.blocks[b]["Bt"])
        t0 = time.perf_counter()
        bt.analyze(4)
        t1 = time.perf_counter()
        kkt = pa.KktSystem(bt, prob.n0, 0, prob.myl, 0, F0=prob.F0)
        bt.sync()
        t2 = time.perf_counter()
        out.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)))
        kkt.close()
        bt.close()
    return out


def main():
    print("library", pa.capi.LIB_PATH)
    if "--time-only" not in sys.argv:
        for kind in ("random", "banded", "sparse_dissected"):
            if kind.startswith("sparse"):
                os.environ["PIPS_HIP_SPARSE_ROOT_BAND"] = det._ROOT_ORDER[kind]
            prob = det._problem(kind)
            report(kind, det._run(prob, list(range(prob.N)), True, reps=1, sparse=kind.startswith("sparse"))[0])
        os.environ.pop("PIPS_HIP_SPARSE_ROOT_BAND", None)
        prob = blocked._problem("banded")
        r = blocked._run(prob, list(range(prob.N)), True, mode=2, reps=1)[0]
        assert r["mode"] == 2
        report("mode2_dense_root", r)
        os.environ["PIPS_HIP_SPARSE_ROOT_BAND"] = packed._ROOT_ORDER["dissected"]
        prob = packed._det_problem()
        report("mode2_packed_sparse", packed._run(prob, list(range(prob.N)), True, reps=1)[0])     # (asserts the packed path itself)
        os.environ.pop("PIPS_HIP_SPARSE_ROOT_BAND", None)
        os.environ["PIPS_HIP_AUG_SWEEPS"] = "1"
        prob = det._problem("banded")
        r = det._run_aug(prob, list(range(prob.N)), True, reps=1)[0]
        assert r["paths"] == [3, 3] and r["aug"] == 1, r["paths"]
        report("augmented_sweeps", r)
        os.environ.pop("PIPS_HIP_AUG_SWEEPS", None)
    t = analysis_times()
    print("analyze ms     ", " ".join(f"{a:8.1f}" for a, _ in t))
    print("KktSystem ms   ", " ".join(f"{k:8.1f}" for _, k in t))
    print("sum ms         ", " ".join(f"{a + k:8.1f}" for a, k in t), f"  median {np.median([a + k for a, k in t]):.1f}")


if __name__ == "__main__":
    main()
