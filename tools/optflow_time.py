"""Device time of skimage's optical_flow_tvl1 on MI355X (tip_optflow.hip): one 2048^2 frame pair (a smoothed-noise
texture moved by a smooth sub-pixel field), the per-kernel HIP-event table of the library's own stream, and a per-level
breakdown: level l's share is the time of the pair reduced to level l's size minus the time of the pair reduced to
level l+1's (the coarser levels are the same work in both).

    python tools/optflow_time.py [--size 2048] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pair(n, seed=3):
    from scipy import ndimage as ndi
    a = ndi.gaussian_filter(np.random.default_rng(seed).random((n, n)), 3.0)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    b = ndi.map_coordinates(a, [yy - 1.3 - 0.5 * np.sin(xx / 90.0), xx + 0.7], order=1, mode="nearest")
    return (a * 60000 / a.max()).astype(np.uint16), (b * 60000 / a.max()).astype(np.uint16)


def device_ms(reg, _lib, a, b, reps):
    """Median over reps of the summed kernel times (HIP events) of one flow; also the warps per level."""
    out = []
    for _ in range(reps):
        _lib.prof_reset()
        _, warps = reg.optical_flow_tvl1_levels(a, b)
        out.append(sum(ms for _, ms in _lib.prof_report().values()))
    return float(np.median(out)), warps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from tissue_image_processing_amd import _lib, _registration as reg
    _lib.init(0)
    a, b = pair(args.size)
    reg.optical_flow_tvl1(a, b)                       # warm-up (workspaces, code objects)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        reg.optical_flow_tvl1(a, b)
    wall = (time.perf_counter() - t0) / args.reps * 1e3
    _lib.prof_enable(True)
    total, warps = device_ms(reg, _lib, a, b, args.reps)
    _lib.prof_reset()
    reg.optical_flow_tvl1_levels(a, b)
    table = {k: {"count": c, "ms": round(ms, 4)} for k, (c, ms) in sorted(_lib.prof_report().items(), key=lambda kv: -kv[1][1])}
    levels, prev = [], 0.0
    sizes = [args.size]
    while min(sizes[-1], sizes[-1]) > 32 and len(sizes) < 10:
        sizes.append((sizes[-1] + 1) // 2)
    for n in reversed(sizes):                       # coarse to fine
        sa, sb = a[:n, :n], b[:n, :n]
        t, w = device_ms(reg, _lib, np.ascontiguousarray(sa), np.ascontiguousarray(sb), args.reps)
        levels.append({"size": n, "ms": round(t - prev, 4), "warps_finest": w[-1]})
        prev = t
    _lib.prof_enable(False)
    print(json.dumps({"size": args.size, "wall_ms": round(wall, 3), "device_ms": round(total, 3), "warps_per_level": warps,
                      "kernels": table, "levels_coarse_to_fine": levels}, indent=1))


if __name__ == "__main__":
    main()
