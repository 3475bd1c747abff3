"""Cost of the tracker's PIV mode in the sharded movie driver on one MI355X: wall time of movie.process_movie over N
synthetic 2048^2 x 30 frames with estimate_drift=True (bench.py --workload movie's exchange) against use_piv=True, and the
HIP-event time of one tip_piv_lookup_max3_i32_dev call (TV-L1 flow of a frame pair + sampling and look-up) per frame.
The frames wait in pinned host memory and run `inflight` at a time in rounds of `inflight` frames, as in bench.py.

    python tools/movie_piv_time.py [--frames 16] [--size 2048] [--z 30] [--inflight 4] [--reps 5] [--movies 3]
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
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--z", type=int, default=30)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5, help="calls of the new entry timed per frame pair")
    ap.add_argument("--movies", type=int, default=3, help="movies timed per mode")
    args = ap.parse_args()
    import torch
    from tissue_image_processing_amd import _lib, movie, synthetic
    Y = X = args.size
    T, Z = args.frames, args.z
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
    stacks = {t: torch.from_numpy(synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc)).pin_memory()
              for t in range(T)}
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, keep_planes=True, inflight=args.inflight)
    warm = [-1 - k for k in range(min(args.inflight, T))]
    tabs = backend.process_frames(warm, lambda t: stacks[0])
    backend.piv_lookup(warm[0], backend.planes[warm[0]], tabs[warm[0]])          # the flow's workspace on this thread
    for t in warm:
        backend.labels.pop(t, None)
        backend.planes.pop(t, None)

    out = {"frames": T, "size": [Y, X, Z], "inflight": args.inflight, "movies_per_mode": args.movies}
    results, walls = {}, {"estimate_drift": [], "use_piv": []}
    for _ in range(args.movies):                  # the two modes alternate
        for name, kw in (("estimate_drift", dict(estimate_drift=True)), ("use_piv", dict(use_piv=True))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend, block_frames=max(1, args.inflight), **kw)
            torch.cuda.synchronize()
            walls[name].append(time.perf_counter() - t0)
            results[name] = (tabs, ids)
    for name, w in walls.items():
        wall = float(np.median(w))
        out[name] = {"wall_s": [round(x, 4) for x in w], "ms_per_frame_median": round(1e3 * wall / T, 3),
                     "tracks": int(max(i.max() for i in results[name][1]))}
    out["use_piv_minus_estimate_drift_ms_per_frame"] = round(out["use_piv"]["ms_per_frame_median"] -
                                                             out["estimate_drift"]["ms_per_frame_median"], 3)

    # the new entry alone, on the movie's own frames (the main thread's library stream)
    tabs = results["use_piv"][0]
    _lib.prof_enable(True)
    dev_ms, wall_ms, kernels = [], [], {}
    for t in range(1, min(T, 4)):
        for _ in range(args.reps):
            _lib.prof_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            backend.piv_lookup(t, backend.planes[t - 1], tabs[t - 1])
            wall_ms.append(1e3 * (time.perf_counter() - t0))
            rep = _lib.prof_report()
            dev_ms.append(sum(ms for _, ms in rep.values()))
        kernels = rep
    _lib.prof_enable(False)
    out["piv_lookup_entry"] = {"device_ms_median": round(float(np.median(dev_ms)), 3),
                               "wall_ms_median": round(float(np.median(wall_ms)), 3),
                               "rows_per_frame": int(tabs[0]["area"].size),
                               "kernels": {k: {"count": c, "ms": round(ms, 4)}
                                           for k, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}}
    backend.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
