"""Counterpart of the reference's `gmspips` driver (Drivers/gams/gmspips/gmspips.cpp:  gmspips <numBlocks> <file stem> ...):
reads the per-block GDX files <stem>0.gdx .. <stem>{n-1}.gdx with the library's reader, hands the blocks to the device-resident
IPM as they are (bounds, two-sided rows, linking rows native on the device) and prints the objective.
   python tools/gmspips.py <numBlocks> <file stem> [mutol] [artol] [scale|scaleEqui|scaleGeo|scaleGeoEqui]
The trailing words are the reference's (gmspips.cpp:12-28): scale and scaleEqui select the equilibrium scaler, scaleGeo the
geometric-mean scaler, scaleGeoEqui both; scaleCurtisReid is not supported; the reference's other words are ignored."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pips_ipmpp_amd as pa  # noqa: E402


SCALER_WORDS = {"scale": "equilibrium", "scaleEqui": "equilibrium", "scaleGeo": "geometric", "scaleGeoEqui": "geometric_equilibrium",
                "scaleCurtisReid": "curtis_reid"}


def parse_args(argv):
    """argv without the program name -> dict(nblocks, stem, mutol, artol, scaler, ignored); numbers after the stem are mutol and
    artol in that order, scaler words select the scaler (the last one wins, as in the reference's loop over its arguments)."""
    if len(argv) < 2:
        raise ValueError("need <numBlocks> <file stem>")
    out = dict(nblocks=int(argv[0]), stem=argv[1], mutol=1e-6, artol=1e-4, scaler=None, ignored=[])   # PIPSIPMppSolver.cpp:143-149
    numbers = []
    for word in argv[2:]:
        if word in SCALER_WORDS:
            out["scaler"] = SCALER_WORDS[word]
            continue
        try:
            numbers.append(float(word))
        except ValueError:
            out["ignored"].append(word)
    if len(numbers) > 2:
        raise ValueError(f"at most two numbers (mutol, artol) after the stem, got {numbers}")
    if numbers:
        out["mutol"] = numbers[0]
    if len(numbers) > 1:
        out["artol"] = numbers[1]
    return out


def main():
    try:
        a = parse_args(sys.argv[1:])
    except ValueError as e:
        print(e)
        print(__doc__)
        return 2
    nblocks, stem, mutol, artol = a["nblocks"], a["stem"], a["mutol"], a["artol"]
    if a["ignored"]:
        print("ignored arguments:", " ".join(a["ignored"]))
    blocks = [pa.capi.gdx_read_block(f"{stem}{k}.gdx", nblocks, k) for k in range(nblocks)]
    ipm = pa.GeneralIpmSolver(blocks, dual_reg=1e-9, scaler=a["scaler"])
    if a["scaler"] is not None:
        sc = ipm.scaling()
        print(f"scaler {a['scaler']}: applied {sc['applied']}  row ratio {sc['row_ratio_before']:.6g} -> {sc['row_ratio_after']:.6g}  "
              f"column ratio {sc['col_ratio_before']:.6g} -> {sc['col_ratio_after']:.6g}  geometric passes {sc['geometric_passes']}")
    res = ipm.solve(max_iter=200, mutol=mutol, artol=artol, verbose=1)
    itr = ipm.iterate()
    names = {0: "SUCCESSFUL_TERMINATION", 1: "MAX_ITS_EXCEEDED", 2: "NUMERICAL_BREAKDOWN", 3: "NUMERICAL_TROUBLES (best iterate)", 4: "INFEASIBLE (probably)"}
    print(f"status {names.get(res['status'], res['status'])}  iterations {res['iterations']}  objective {res['objective']:.10g}  dual objective {res['dual_objective']:.10g}")
    root = blocks[0]
    my0, myl, mz0, mzl = root["mA"], root["mBL"], root["mC"], root["mDL"]
    print("linking variables:", np.array2string(itr["x"][:root["n0"]], precision=6))
    print("multipliers of the linking rows: eq", np.array2string(itr["y"][my0:my0 + myl], precision=6), " ineq", np.array2string(itr["z"][mz0:mz0 + mzl], precision=6))
    print(f"complementarity pairs {ipm.n_pairs}, statistics {ipm.stats()} {ipm.stats2()}")
    return 0 if res["status"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
