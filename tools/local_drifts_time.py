#!/usr/bin/env python3
"""Time of the local-drift map of one frame pair, recorded, not asserted:

    python tools/local_drifts_time.py [--size 2048] [--repeats 5] [--movie-frames 6] [--out profiles/local_drifts_time.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/local_drifts_time.py --only batched --out ""

A size^2 float64 pair (low-passed noise, the second frame shifted and perturbed) with upstream's windows (step 100, window 700:
196 at 2048^2).  Two paths, both on device-resident frames and both ending in a stream wait, timed with host clocks:
  loop     per window two tip_memcpy2d_d2d crops and one tip_phase_correlation_dev (the path local_drifts took before the batch);
  batched  one tip_phase_correlation_windows_dev call per window extent.
After a warm-up the two alternate `repeats` times; all values and the medians are recorded, with a check that the shifts are
equal.  A separate pass with the library's launch profiler on counts the kernel launches of either path (and gives the batched
path's kernel times from HIP events); the stream waits follow from them: both paths run the one correlation body, which waits
once per chunk after its two absargmax pairs (upsample 100) -- the loop once per window, the batch once per chunk.
--only batched runs the batched path alone `repeats` times, for a kernel trace with nothing else in it.
With --movie-frames N > 0: the wall time of movie.process_movie over N synthetic size^2 frames on one GPU with
local_drifts=True against estimate_drift=True, alternating."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tissue_image_processing_amd import _lib  # noqa: E402
from tissue_image_processing_amd import _registration as reg  # noqa: E402


def make_pair(size, seed=12):
    rng = np.random.default_rng(seed)
    f = np.fft.rfft2(rng.random((size, size)))
    ky, kx = np.fft.fftfreq(size)[:, None], np.fft.rfftfreq(size)[None, :]
    base = np.fft.irfft2(f * np.exp(-(ky * ky + kx * kx) * (2.0 * np.pi * 3.0) ** 2 / 2.0), (size, size))
    a = 1000.0 * (base - base.min()) / (base.max() - base.min())
    b = np.roll(a, (3, -2), axis=(0, 1)) + rng.normal(0.0, 1.0, a.shape)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


class Pair(object):
    def __init__(self, a, b):
        self.shape = a.shape
        self.da, self.db = _lib.DeviceBuffer(a.nbytes).upload(a), _lib.DeviceBuffer(b.nbytes).upload(b)
        self.windows = reg.local_drift_windows(a.shape)
        self.origins = np.array([(r0, c0, r0, c0) for r0, _, c0, _ in self.windows], np.int32)
        self.extents = [(r1 - r0, c1 - c0) for r0, r1, c0, c1 in self.windows]
        big = max(ny * nx for ny, nx in self.extents) * 8
        self.wa, self.wb = _lib.DeviceBuffer(big), _lib.DeviceBuffer(big)

    def loop(self):
        lib, W = _lib.lib(), self.shape[1]
        out = np.empty((len(self.windows), 2))
        for i, (r0, r1, c0, c1) in enumerate(self.windows):
            ny, nx = r1 - r0, c1 - c0
            for dst, src in ((self.wa, self.da), (self.wb, self.db)):
                _lib.check(lib.tip_memcpy2d_d2d(dst.ptr, nx * 8, src.ptr + (r0 * W + c0) * 8, W * 8, nx * 8, ny))
            out[i] = reg.phase_cross_correlation_dev(self.wa.ptr, self.wb.ptr, ny, nx, 100)
        return out

    def batched(self):
        return reg.correlate_windows_by_extent(self.da.ptr, self.db.ptr, self.shape, self.origins, self.extents)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def counted(fn):
    _lib.prof_enable(True)
    _lib.prof_reset()
    fn()
    rep = _lib.prof_report()
    _lib.prof_enable(False)
    return rep


def movie_walls(size, frames, z, movies):
    import torch
    from tissue_image_processing_amd import movie, synthetic
    sites_t, is_hc = synthetic.make_movie_sites(size, size, frames, seed=5)
    stacks = {t: torch.from_numpy(synthetic.make_stack(z, size, size, seed=200 + t, sites=sites_t[t], is_hc=is_hc)).pin_memory()
              for t in range(frames)}
    backend = movie.GpuFrameBackend(2, z, size, size, device=0, keep_planes=True, inflight=2)
    walls = {"estimate_drift": [], "local_drifts": []}
    try:
        for k in range(movies + 1):                  # the first movie of either mode warms up and is not recorded
            for name, kw in (("estimate_drift", dict(estimate_drift=True)), ("local_drifts", dict(local_drifts=True))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                movie.process_movie(frames, lambda t: stacks[t], backend, block_frames=2, **kw)
                torch.cuda.synchronize()
                if k:
                    walls[name].append(time.perf_counter() - t0)
    finally:
        backend.close()
    return {"frames": frames, "size": [size, size, z], "inflight": 2, "block_frames": 2,
            **{name: {"wall_s": [round(w, 4) for w in ws], "ms_per_frame_median": round(1e3 * float(np.median(ws)) / frames, 2)}
               for name, ws in walls.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("batched",), default=None)
    ap.add_argument("--movie-frames", type=int, default=6)
    ap.add_argument("--movie-z", type=int, default=10)
    ap.add_argument("--movies", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_drifts_time.json"))
    a = ap.parse_args()
    pair = Pair(*make_pair(a.size))
    if a.only == "batched":
        for _ in range(a.repeats + 1):
            pair.batched()
        return
    want, got = pair.loop(), pair.batched()          # warm-up: workspaces, code objects
    loop_ms, batched_ms = [], []
    for _ in range(a.repeats):                       # the two paths alternate
        ms, _ = timed(pair.loop)
        loop_ms.append(ms)
        ms, _ = timed(pair.batched)
        batched_ms.append(ms)
    rep_loop, rep_batched = counted(pair.loop), counted(pair.batched)
    res = {"size": a.size, "dtype": "float64", "windows": len(pair.windows),
           "windows_per_extent": {"%dx%d" % ext: pair.extents.count(ext) for ext in dict.fromkeys(pair.extents)},
           "shifts_equal": bool(np.array_equal(want, got)),
           "loop_ms": [round(v, 3) for v in loop_ms], "loop_ms_median": round(float(np.median(loop_ms)), 3),
           "batched_ms": [round(v, 3) for v in batched_ms], "batched_ms_median": round(float(np.median(batched_ms)), 3),
           "loop_ms_spread": round(max(loop_ms) - min(loop_ms), 3), "batched_ms_spread": round(max(batched_ms) - min(batched_ms), 3),
           "loop_kernel_launches": int(sum(c for c, _ in rep_loop.values())),
           "batched_kernel_launches": int(sum(c for c, _ in rep_batched.values())),
           "loop_stream_waits": int(rep_loop["absargmax"][0] // 2), "batched_stream_waits": int(rep_batched["absargmax"][0] // 2),
           "batched_kernels_hip_events": {k: {"count": c, "ms": round(ms, 3)}
                                          for k, (c, ms) in sorted(rep_batched.items(), key=lambda kv: -kv[1][1])},
           "loop_kernels_hip_events": {k: {"count": c, "ms": round(ms, 3)}
                                       for k, (c, ms) in sorted(rep_loop.items(), key=lambda kv: -kv[1][1])}}
    if a.movie_frames > 0:
        res["process_movie"] = movie_walls(a.size, a.movie_frames, a.movie_z, a.movies)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
