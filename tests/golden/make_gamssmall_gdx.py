"""Generates tests/golden/gamssmall_gdx.npz: the GDX files of the 26 GAMSsmall known-answer instances that tests/golden/gamssmall.json
was extracted from (per instance its per-block files <name>0.gdx .. <name>{B-1}.gdx and its unsplit model file <name>.gdx), so that the
reader tests run on the very files without the upstream PIPS-IPM++ tree.  Data only: the files as bytes (uint8), keyed
"<name>/<k>" and "<name>/whole"; the paths come from the fixture's "source" entries.

Usage, with a checkout of PIPS-IPM++:  python tests/golden/make_gamssmall_gdx.py <PIPS-IPM++ source tree>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(tree):
    data = json.load(open(os.path.join(HERE, "gamssmall.json")))["instances"]
    files = {}
    for d in data:
        for k in range(d["num_blocks"]):
            files[f"{d['name']}/{k}"] = tree + d["source"] + f"{k}.gdx"
        files[f"{d['name']}/whole"] = tree + d["source"] + ".gdx"
    arrays = {key: np.frombuffer(open(path, "rb").read(), dtype=np.uint8) for key, path in files.items()}
    np.savez_compressed(os.path.join(HERE, "gamssmall_gdx.npz"), **arrays)
    print(f"{len(arrays)} files, {sum(a.size for a in arrays.values())} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
