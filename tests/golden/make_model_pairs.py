#!/usr/bin/env python3
"""Record what tests/test_model_pairs.py needs of the reference MJCF (run where a reference checkout is): per body its parent,
its joint count and its geoms' resolved name / mesh / type / contype / conaffinity, and the arm's <exclude> body
pairs, as tools/compile_model.py's parse() reads them from so100_transfer_cube.xml, scene_so100.xml and
trs_so_arm100/so_arm100.xml (SO100_REFERENCE names the reference checkout).  Writes reference_bodies.json next to
this script; the test applies MuJoCo's collision filters to that record."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "gym-so100-c_amd", "tools"))
GEOM_KEYS = ("name", "mesh", "type", "contype", "conaffinity")


def main():
    from compile_model import parse
    _, bodies, _, excludes = parse()
    out = {"bodies": {name: {"parent": rec["parent"], "joints": len(rec["joints"]),
                             "geoms": [{k: g[k] for k in GEOM_KEYS if k in g} for g in rec["geoms"]]}
                      for name, rec in bodies.items()},
           "excludes": [list(e) for e in excludes]}
    path = os.path.join(HERE, "reference_bodies.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, len(out["bodies"]), "bodies")


if __name__ == "__main__":
    main()
