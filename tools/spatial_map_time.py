#!/usr/bin/env python3
"""Time of one spatial feature map, recorded, not asserted:

    python tools/spatial_map_time.py [--size 2048] [--radius 100] [--step 8] [--out profiles/spatial_map_time.json]

`Tissue.calculate_spatial_data(frame, radius, step, "HC density")` on a synthetic frame: the cell table is the synthetic generator's
sites (one per 900 px^2: 4660 cells at 2048^2; centroid = site, seeded areas, 30 % hair cells), the label map is empty -- the map
only takes its shape and its border labels from it.  Reported: the kernels' device time (HIP events around each launch,
tip_prof_report), the wall time of the whole call (table columns to host map), and the wall time of the vectorised numpy
restatement (tests/spatial_restate.py) of the same map on the same machine, with a check that the two maps are equal."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spatial_restate as sr  # noqa: E402
from tissue_image_processing_amd import _lib, synthetic  # noqa: E402
from tissue_image_processing_amd import tissue_info as ti  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--radius", type=float, default=100)
    ap.add_argument("--step", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_map_time.json"))
    a = ap.parse_args()
    sites, is_hc = synthetic.make_sites(a.size, a.size, seed=8)
    n = sites.shape[0]
    rng = np.random.default_rng(9)
    table = pd.DataFrame({"cy": sites[:, 0], "cx": sites[:, 1], "area": rng.integers(500, 1300, n), "perimeter": rng.uniform(90, 130, n),
                          "label": np.arange(1, n + 1), "n_neighbors": 6, "valid": 1, "type": is_hc.astype(np.int64), "empty_cell": 0})
    t = ti.Tissue(1, None, ["zo", "atoh"])
    t.type_names = ["HC"]
    t.set_labels(1, np.zeros((a.size, a.size), np.int32))
    t.set_cells_info(1, table)
    out, msg = t.calculate_spatial_data(1, a.radius, a.step, "HC density")      # warm-up: library load, workspaces
    assert msg == ""
    _lib.prof_enable(True)
    _lib.prof_reset()
    walls = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out, msg = t.calculate_spatial_data(1, a.radius, a.step, "HC density")
        walls.append(time.perf_counter() - t0)
    report = _lib.prof_report()
    _lib.prof_enable(False)
    kernels = {k: v[1] / v[0] for k, v in report.items() if k in ("window_stats", "window_value", "spatial_fill")}
    t0 = time.perf_counter()
    ref, _, n_sel = sr.spatial_map((a.size, a.size), a.step, a.radius, table.cy.to_numpy(), table.cx.to_numpy(), table.area.to_numpy(),
                                   table.type.to_numpy(), None, 0, True, "density")
    numpy_s = time.perf_counter() - t0
    res = {"size": a.size, "radius": a.radius, "step": a.step, "cells": int(n), "grid_points": int(n_sel.size),
           "distance_tests": int(n_sel.size) * int(n), "device_kernel_ms": kernels, "device_kernels_total_ms": sum(kernels.values()),
           "call_wall_ms_median": 1e3 * float(np.median(walls)), "call_wall_ms_all": [1e3 * w for w in walls],
           "numpy_restatement_wall_s": numpy_s, "maps_equal": bool(np.array_equal(out, ref))}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
