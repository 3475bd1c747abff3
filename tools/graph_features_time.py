#!/usr/bin/env python3
"""Time of the neighbour-graph columns of one frame, recorded, not asserted:

    python tools/graph_features_time.py [--size 2048] [--out profiles/graph_features_time.json]

`FramePipeline.neighbor_features(n, valid, type)` on a synthetic label map (the generator's Voronoi tessellation, one site per 900 px^2:
about 4 700 cells at 2048^2, 30 % hair cells, cells separated by one-pixel lines of label 0) that is uploaded into the pipeline's label
buffer.  Reported: the device time of the chain's kernels (HIP events around each launch, tip_prof_report), the wall time of the call
(uploads of the two byte columns to the download of the ten columns), and the wall time of the numpy restatement
(tests/graph_restate.py) of the same ten columns from the same pairs, triples and bytes on the same machine, with a check that the
two agree.  Upstream's own loops are not run here (the reference is not part of this repository)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import graph_restate as gr  # noqa: E402
from tissue_image_processing_amd import _lib, synthetic  # noqa: E402
from tissue_image_processing_amd.pipeline import FramePipeline  # noqa: E402

KERNELS = ("csr_count", "csr_scan", "csr_fill", "csr_sort", "contact_pairs", "contact_emit", "graph_counts", "graph_second", "edge_weights",
           "contact_sums")


def restated(pairs, triples, n, valid, type):
    off, adj = gr.neighbor_csr(pairs, n, valid)
    q = np.arange(n)
    empty = np.zeros(n, np.uint8)
    out = dict(n_neighbors=gr.graph_counts(off, adj, valid, empty, type, q, gr.ALL),
               valid_neighbors=gr.graph_counts(off, adj, valid, empty, type, q, gr.VALID),
               second_neighbors=[len(s) for s in gr.graph_second(off, adj, valid, type, q)],
               contact_length=gr.contact_sums(*triples, off, adj, valid, type, q, gr.ALL)[0])
    for prefix, positive in (("hc", True), ("sc", False)):
        out[prefix + "_neighbors"] = gr.graph_counts(off, adj, valid, empty, type, q, gr.TYPE, 0, positive)
        out[prefix + "_second_neighbors"] = [len(s) for s in gr.graph_second(off, adj, valid, type, q, 0, positive)]
        out[prefix + "_contact_length"] = gr.contact_sums(*triples, off, adj, valid, type, q, gr.TYPE, 0, positive)[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_features_time.json"))
    a = ap.parse_args()
    Y = X = a.size
    sites, is_hc = synthetic.make_sites(Y, X, seed=8)
    d1, d2, nearest = synthetic._two_nearest(sites, Y, X)
    labels = np.where(d2 - d1 < 1.0, 0, nearest + 1).astype(np.int32)
    n = int(labels.max())
    pipe = FramePipeline(1, 1, Y, X)
    pipe.d_labels.upload(labels)
    tab = pipe.cell_tables(max_cells=n)
    area = tab["area"]
    valid = ((area > 0.1 * area.mean()) & (area < 10 * area.mean())).astype(np.uint8)
    type = np.zeros(n, np.uint8)
    type[:is_hc.size] = is_hc[:n].astype(np.uint8)
    got = pipe.neighbor_features(n, valid, type)                  # warm-up: workspaces
    _lib.prof_enable(True)
    _lib.prof_reset()
    walls = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        got = pipe.neighbor_features(n, valid, type)
        walls.append(time.perf_counter() - t0)
    report = _lib.prof_report()
    _lib.prof_enable(False)
    kernels = {k: v[1] / a.repeats for k, v in report.items() if k in KERNELS}
    pairs = tab["pairs"]
    t0 = time.perf_counter()
    triples = gr.contact_triples(labels)
    want = restated(pairs, triples, n, valid, type)
    numpy_s = time.perf_counter() - t0
    res = {"size": a.size, "cells": n, "pairs": int(pairs.shape[0]), "columns": sorted(got),
           "device_kernel_ms_per_call": kernels, "device_kernels_total_ms_per_call": sum(kernels.values()),
           "call_wall_ms_median": 1e3 * float(np.median(walls)), "call_wall_ms_all": [1e3 * w for w in walls],
           "numpy_restatement_wall_s": numpy_s,
           "columns_equal": bool(all(np.array_equal(got[k], np.asarray(want[k], dtype=np.int64)) for k in want))}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
