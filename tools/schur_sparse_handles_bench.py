"""The level-1.5b factorisation leg of tools/plugin_path_bench.py (all leaves of a rank through the array-of-handles entry, host pointers)
with the dense and with the sparse Schur target in one process: pips_hip_ldl_factor_schur_batch against
pips_hip_ldl_factor_schur_sparse_batch on a time-coupled chain (default 16 leaves x 2000 variables, S = 200).  Two sets of handles over the
same leaves, one warm-up call each (binding, analysis, first-touch allocations), then the two entries alternate; the median of --reps
calls each (a host clock around calls that end in a stream synchronise) and the bytes each copies back per call.
usage: schur_sparse_handles_bench.py [--blocks 16] [--n 2000] [--S 200] [--reps 7] [--out FILE]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, scipy.sparse as sp
import pips_ipmpp_amd as pa
from tests.util import TimeCoupledProblem

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=16)
ap.add_argument("--n", type=int, default=2000)
ap.add_argument("--S", type=int, default=200)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if pa.device_count() == 0:
    sys.exit("schur_sparse_handles_bench.py: no GPU - nothing is measured without one")

prob = TimeCoupledProblem(20261020, a.blocks, a.n, a.n // 2, a.S // 2, a.S - a.S // 2, 6)
S = prob.S


def handles():
    out = []
    for blk in prob.blocks:
        s = pa.HipLdlSolver(blk["K"], n_primal=prob.n_i, refine_steps=2, refine_tol=1e-15, backward_error=True)   # (the adapters' setting)
        s.set_border(blk["Bt"])
        out.append(s)
    return out


# the host's sparse Schur complement: the upper triangle of the union of the leaves' cliques and a full diagonal
cols = [np.nonzero(np.diff(np.asarray(blk["Bt"].rowptr)) > 0)[0] for blk in prob.blocks]
R = np.concatenate([np.repeat(bm, len(bm)) for bm in cols] + [np.arange(S)])
C = np.concatenate([np.tile(bm, len(bm)) for bm in cols] + [np.arange(S)])
sc = sp.coo_matrix((np.ones(len(R)), (np.minimum(R, C), np.maximum(R, C))), shape=(S, S)).tocsr()
sc.sum_duplicates(); sc.sort_indices()
sc.data[:] = 0.0
dense, sparse = handles(), handles()
SC = np.zeros((S, S))
pa.HipLdlSolver.factor_schur_batch(dense, SC)            # warm-up of each
pa.HipLdlSolver.factor_schur_sparse_batch(sparse, sc)
T = sparse[0].info()["sparse_schur_len"]
rows = np.repeat(np.arange(S), np.diff(sc.indptr))
agree = float(np.abs(sc.data - SC[sc.indices, rows]).max() / np.abs(SC).max())     # (the dense entry fills the lower triangle)
t_dense, t_sparse = [], []
for _ in range(a.reps):
    t0 = time.perf_counter(); pa.HipLdlSolver.factor_schur_batch(dense, SC); t_dense.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); pa.HipLdlSolver.factor_schur_sparse_batch(sparse, sc); t_sparse.append(time.perf_counter() - t0)
res = {"workload": f"level 1.5b factorisation leg, time-coupled chain {a.blocks} x {a.n}, S = {S}, both entries in one process, alternating after a warm-up of each",
       "reps": a.reps, "schur_mode": sparse[0].info()["schur_mode"],
       "dense_entry_ms": {"median": 1e3 * float(np.median(t_dense)), "min": 1e3 * min(t_dense), "max": 1e3 * max(t_dense)},
       "sparse_entry_ms": {"median": 1e3 * float(np.median(t_sparse)), "min": 1e3 * min(t_sparse), "max": 1e3 * max(t_sparse)},
       "bytes_copied_back_per_call": {"dense_entry": 8 * S * S, "sparse_entry": 8 * T}, "pattern_entries": int(sc.nnz), "touched_positions_T": T,
       "max_rel_difference_of_the_two_terms": agree}
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
