#!/usr/bin/env python3
"""Time of the hexatic-order columns of one frame, recorded, not asserted:

    python tools/order_features_time.py [--size 2048] [--out profiles/order_features_time.json]

The table is the synthetic generator's at size^2 (one site per 900 px^2: about 4 660 cells at 2048^2), its sites taken as the
centroids.  Reported: the device time of the order kernels (HIP events around each launch, tip_prof_report) in
`FramePipeline.order_features`, the wall time of that call, the wall time of the mixin's
`find_nearest_neighbors_using_voroni_tesselation` + `calc_psin` on the same table, and the wall time of scipy's `Voronoi` plus a
vectorised numpy psi6 on the same machine, with a check that the neighbour sets agree and psi6 agrees to 1e-13.  Upstream's own row
loop is not run here (the reference is not part of this repository)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pandas as pd  # noqa: E402
from tissue_image_processing_amd import _lib, synthetic, tissue_info  # noqa: E402
from tissue_image_processing_amd.pipeline import FramePipeline  # noqa: E402

KERNELS = ("order_grid", "order_count", "csr_scan", "order_fill", "delaunay", "order_row_sort", "psin")


def scipy_psi6(cy, cx):
    from scipy.spatial import Voronoi
    ridge = Voronoi(np.stack([cx, cy], axis=1)).ridge_points
    a, b = np.concatenate([ridge[:, 0], ridge[:, 1]]), np.concatenate([ridge[:, 1], ridge[:, 0]])
    th = 6.0 * np.arctan2(cy[b] - cy[a], cx[b] - cx[a])
    n = cy.size
    sc, ss = np.bincount(a, np.cos(th), n), np.bincount(a, np.sin(th), n)
    deg = np.bincount(a, minlength=n)
    return np.hypot(sc, ss) / np.maximum(deg, 1), deg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_features_time.json"))
    a = ap.parse_args()
    sites, _ = synthetic.make_sites(a.size, a.size, seed=8)
    cy, cx = np.ascontiguousarray(sites[:, 0], np.float64), np.ascontiguousarray(sites[:, 1], np.float64)
    n = cy.size
    valid = np.ones(n, np.uint8)
    pipe = FramePipeline(1, 1, 16, 16)
    got = pipe.order_features(n, valid, cy, cx)                     # warm-up: workspaces
    _lib.prof_enable(True)
    _lib.prof_reset()
    walls = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        got = pipe.order_features(n, valid, cy, cx)
        walls.append(time.perf_counter() - t0)
    report = _lib.prof_report()
    _lib.prof_enable(False)
    kernels = {k: v[1] / a.repeats for k, v in report.items() if k in KERNELS}
    t = tissue_info.Tissue(1)
    table = pd.DataFrame({"cx": cx, "cy": cy, "valid": 1, "empty_cell": 0, "type": 0, "label": np.arange(1, n + 1)})
    table["neighbors"] = [set() for _ in range(n)]
    t.set_cells_info(1, table)
    mixin = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        psi_mixin = t.calc_psin(1, table, t.find_nearest_neighbors_using_voroni_tesselation(table), n=6)
        mixin.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want, deg = scipy_psi6(cy, cx)
    scipy_s = time.perf_counter() - t0
    res = {"size": a.size, "cells": n, "device_kernel_ms_per_call": kernels, "device_kernels_total_ms_per_call": sum(kernels.values()),
           "order_features_wall_ms_median": 1e3 * float(np.median(walls)), "order_features_wall_ms_all": [1e3 * w for w in walls],
           "mixin_find_nearest_plus_calc_psin_wall_ms_median": 1e3 * float(np.median(mixin)),
           "scipy_voronoi_plus_numpy_psi_wall_ms": 1e3 * scipy_s,
           "degrees_equal": bool(np.array_equal(got["voronoi_neighbors"], deg)),
           "psi6_max_abs_difference": float(np.max(np.abs(got["psi6"] - want))),
           "mixin_psi6_max_abs_difference": float(np.max(np.abs(psi_mixin - want)))}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
