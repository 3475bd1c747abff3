#!/usr/bin/env python3
"""Cost of the sensory-region filter in the sharded movie driver on one MI355X, recorded, not asserted:

    python tools/sensory_region_time.py [--frames 4] [--size 2048] [--z 30] [--runs 5] [--out profiles/sensory_region_time.json]

Synthetic frames at size^2 (the headline density: about 11 500 table rows at 2048^2).  Reported:
  * the device call per frame, FramePipeline.sensory_region (tip_sensory_region_i32_dev) on a resident frame: wall time of the call
    (upload of the rows, kernels, the one wait that sizes the sort, download) and the HIP-event time of each kernel, medians over
    --runs calls;
  * movie.process_movie frames/s with cell_types alone -- the option off, which is the code path of the commit before the filter --
    and with sensory_region=True: median and spread of --runs runs each, the two modes alternating;
  * under its own key, naming its machine: the reference method's time on the goldens' case E (11 500 rows, 3 000 HC), measured on a
    CPU machine by tools/make_goldens_sensory.py and read from tests/golden/sensory_region.npz -- the reference is not part of this
    repository and does not run next to the GPU."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELL_TYPES = dict(threshold=0.03, percentage_above_threshold=3, peak_window_size=3)


def spread(values):
    v = sorted(float(x) for x in values)
    return {"median": round(float(np.median(v)), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "all": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--z", type=int, default=30)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensory_region_time.json"))
    a = ap.parse_args()
    import torch
    from tissue_image_processing_amd import _lib, movie, synthetic
    Y = X = a.size
    T, Z = a.frames, a.z
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
    stacks = {t: torch.from_numpy(synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc)).pin_memory() for t in range(T)}
    backends = {name: movie.GpuFrameBackend(2, Z, Y, X, device=0, inflight=a.inflight, cell_types=CELL_TYPES, sensory_region=on)
                for name, on in (("cell_types", False), ("cell_types_sensory_region", True))}
    fps = {name: [] for name in backends}
    tabs = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name, backend in backends.items():
            movie.process_movie(min(T, 2), lambda t: stacks[t], backend)             # warm-up: workspaces, code objects, workers
        for _ in range(a.runs):
            for name, backend in backends.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tabs[name], _ids = movie.process_movie(T, lambda t: stacks[t], backend)
                torch.cuda.synchronize()
                fps[name].append(T / (time.perf_counter() - t0))
    res = {"frames": T, "size": [Y, X, Z], "inflight": a.inflight, "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "rows_per_frame": int(tabs["cell_types"][0]["area"].size),
           "process_movie_frames_per_s": {name: spread(v) for name, v in fps.items()},
           "process_movie_note": "cell_types: the option off, the code path of the commit before the filter; the two modes alternate run by run"}
    on = backends["cell_types_sensory_region"]
    res["hull_vertices_per_frame"] = [int(on.sensory_hulls[t].size) if t in on.sensory_hulls else 0 for t in range(T)]
    res["rows_outside_per_frame"] = [int((tabs["cell_types_sensory_region"][t]["in_sensory_region"] == 0).sum()) for t in range(T)]
    res["hair_cells_per_frame"] = [int(((tb["type"] == 1) & (tb["valid"] == 1) & (tb["area"] > 0)).sum()) for tb in tabs["cell_types"]]
    # the call alone, on a pipeline that holds one frame: labels, tables and a type map of its own
    from tissue_image_processing_amd.pipeline import FramePipeline
    pipe = FramePipeline(2, Z, Y, X)
    d = _lib.DeviceBuffer(stacks[0].numel() * 2)
    _lib.check(pipe.lib.tip_memcpy_h2d(d.ptr, stacks[0].data_ptr(), stacks[0].numel() * 2))
    pipe.project(d)
    pipe.segment(0)
    tab = pipe.cell_tables()
    d.free()
    n = tab["area"].size
    rows = pipe.cell_types(n=n, **CELL_TYPES)
    area = tab["area"].astype(np.float64)
    cy, cx = np.where(area > 0, tab["sumy"] / np.maximum(area, 1), 0.0), np.where(area > 0, tab["sumx"] / np.maximum(area, 1), 0.0)
    pipe.sensory_region(n, cy, cx, rows["type"], rows["valid"])                        # warm-up
    walls, kernels = [], {}
    _lib.prof_enable(True)
    for _ in range(a.runs):
        _lib.prof_reset()
        t0 = time.perf_counter()
        got = pipe.sensory_region(n, cy, cx, rows["type"], rows["valid"])
        walls.append(1e3 * (time.perf_counter() - t0))
        for k, (_c, ms) in _lib.prof_report().items():
            kernels.setdefault(k, []).append(ms)
    _lib.prof_enable(False)
    walls_ct = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        pipe.cell_types(n=n, **CELL_TYPES)
        walls_ct.append(1e3 * (time.perf_counter() - t0))
    res["call"] = {"rows": int(n), "hull_vertices": int(got["hull"].size), "rows_outside": int(got["outside"].sum()),
                   "sensory_region_wall_ms": spread(walls),
                   "sensory_region_wall_note": "with the launch profiler on (HIP events around every launch)",
                   "kernel_ms_median": {k: round(float(np.median(v)), 4) for k, v in sorted(kernels.items())},
                   "kernels_total_ms_median": round(float(sum(np.median(v) for v in kernels.values())), 4),
                   "cell_types_wall_ms_same_frame": spread(walls_ct)}
    for backend in backends.values():
        backend.close()
    g = np.load(os.path.join(ROOT, "tests", "golden", "sensory_region.npz"), allow_pickle=False)
    res["reference_on_cpu"] = {"machine": str(g["reference_machine"]), "case": "E: 11 500 rows, 3 000 HC, 2048 extents",
                               "detect_non_sensory_region_cells_ms": spread(1e3 * g["reference_seconds_E"]),
                               "note": "the reference's own method (scipy Delaunay + find_simplex), measured by tools/make_goldens_sensory.py"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
