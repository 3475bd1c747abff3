#!/usr/bin/env python3
"""Time of the frame-to-frame linker on the host and on the device, recorded, not asserted:

    python tools/link_time.py [--frames 6] [--repeats 5] [--out profiles/link_device_time.json]

The tables are tests/link_cases.py's movie at the 2048^2 headline density (4660 cells, sigma = 1 px jitter plus drift, 3 % of
the cells hidden per frame, fresh cells appended), search_range 100, adaptive_stop 10, memory 3: the GUI's call.  Per linked
frame (every frame but the first, which has no tracks to link to) it reports

  * the wall time of FrameLinker.link (cKDTree, scipy components, linear_sum_assignment per subnet);
  * the wall time of DeviceFrameLinker.link (one tip_link_frame_f64 call: uploads, kernels, one look at the device per round,
    download) -- after a warm-up pass, with the launch profiler off;
  * in a pass of its own with the launch profiler on, the device time of the call's kernels (HIP events around every launch,
    tip_prof_report) by kernel, and the call's statistics (links, rounds, subnets, largest subnet, final range).

Ids of the two linkers are compared in every frame.  The yardstick is the host linker measured in the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import link_cases as lc  # noqa: E402
from tissue_image_processing_amd import _lib, linking  # noqa: E402


def timed_run(linker, frames):
    """(ids per frame, seconds per frame)"""
    ids, secs = [], []
    for f in frames:
        t0 = time.perf_counter()
        ids.append(linker.link(f))
        secs.append(time.perf_counter() - t0)
    return ids, secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_device_time.json"))
    a = ap.parse_args()
    seed, n, size, _ = lc.MOVIES["C"]
    frames = lc.movie(seed, n, size, a.frames)
    _lib.lib()
    ref, _ = timed_run(linking.DeviceFrameLinker(), frames)          # warm-up: code objects, workspaces
    host, device, equal = [], [], True
    for _ in range(a.repeats):                                       # the two linkers alternate
        ids_h, s = timed_run(linking.FrameLinker(), frames)
        host.append(s[1:])
        ids_d, s = timed_run(linking.DeviceFrameLinker(), frames)
        device.append(s[1:])
        equal = equal and all(np.array_equal(x, y) for x, y in zip(ids_h, ids_d)) and all(np.array_equal(x, y) for x, y in zip(ref, ids_d))
    host, device = np.array(host), np.array(device)
    _lib.prof_enable(True)
    _lib.prof_reset()
    lk, stats = linking.DeviceFrameLinker(), []
    for f in frames:
        lk.link(f)
        stats.append(lk.last_stats)
    report = _lib.prof_report()
    _lib.prof_enable(False)
    linked = len(frames) - 1
    kernels = {k: {"launches_per_frame": v[0] / linked, "ms_per_frame": v[1] / linked} for k, v in sorted(report.items())}
    res = {"cells": n, "size": size, "frames": len(frames), "linked_frames": linked, "repeats": a.repeats,
           "features_per_frame": [int(f.shape[0]) for f in frames],
           "host_link_wall_ms_per_frame_median": 1e3 * float(np.median(host)),
           "host_link_wall_ms_per_frame_min_max": [1e3 * float(host.min()), 1e3 * float(host.max())],
           "device_link_wall_ms_per_frame_median": 1e3 * float(np.median(device)),
           "device_link_wall_ms_per_frame_min_max": [1e3 * float(device.min()), 1e3 * float(device.max())],
           "device_kernels_ms_per_frame": sum(k["ms_per_frame"] for k in kernels.values()),
           "device_kernels": kernels, "stats_per_linked_frame": stats[1:], "ids_equal": bool(equal)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
