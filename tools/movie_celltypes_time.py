"""Cost of on-device cell typing in the sharded movie driver on one MI355X: wall time of movie.process_movie over N synthetic
2048^2 x 30 frames without typing, with typing (GUI defaults 0.03 / 3 without the peak test) and with the peak test, and
the HIP-event time of one FramePipeline.cell_types call (tip_cell_types_i32_dev) per kernel.  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel-level table.

    python tools/movie_celltypes_time.py [--frames 6] [--size 2048] [--z 30] [--inflight 1] [--peak 3] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--z", type=int, default=30)
    ap.add_argument("--inflight", type=int, default=1)
    ap.add_argument("--peak", type=int, default=3, help="peak window of the third mode")
    ap.add_argument("--reps", type=int, default=5, help="timed calls of the entry per mode")
    args = ap.parse_args()
    import torch
    from tissue_image_processing_amd import _lib, movie, synthetic
    Y = X = args.size
    T, Z = args.frames, args.z
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
    stacks = {t: torch.from_numpy(synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc)).pin_memory()
              for t in range(T)}
    modes = (("untyped", None),
             ("typed", dict(threshold=0.03, percentage_above_threshold=3, peak_window_size=0)),
             ("typed_peak", dict(threshold=0.03, percentage_above_threshold=3, peak_window_size=args.peak)))
    out = {"frames": T, "size": [Y, X, Z], "inflight": args.inflight}
    for name, opts in modes:
        backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, inflight=args.inflight, cell_types=opts)
        movie.process_movie(min(T, 2), lambda t: stacks[t], backend)                 # warm-up (workspaces, code objects)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rec = {"wall_s": round(wall, 4), "ms_per_frame": round(1e3 * wall / T, 3), "rows_per_frame": int(tabs[0]["area"].size)}
        if opts is not None:
            rec["positive_valid_rows"] = int(sum(int(((tb["type"] == 1) & (tb["valid"] == 1)).sum()) for tb in tabs))
            p = backend.pipe                       # (its last frame's labels and projection are still resident)
            n = int(tabs[T - 1]["area"].size) if args.inflight <= 1 else None
            _lib.prof_enable(True)
            dev_ms, wall_ms = [], []
            for _ in range(args.reps):
                _lib.prof_reset()
                t0 = time.perf_counter()
                p.cell_types(n=n, **opts)
                wall_ms.append(1e3 * (time.perf_counter() - t0))
                rep = _lib.prof_report()
                dev_ms.append(sum(ms for _, ms in rep.values()))
            _lib.prof_enable(False)
            rec["entry"] = {"device_ms_median": round(float(np.median(dev_ms)), 3),
                            "wall_ms_median": round(float(np.median(wall_ms)), 3),
                            "kernels": {k: {"count": c, "ms": round(ms, 4)}
                                        for k, (c, ms) in sorted(rep.items(), key=lambda kv: -kv[1][1])}}
        backend.close()
        out[name] = rec
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
