"""The sharded movie driver's two segmentation modes on one MI355X: frames/s of movie.process_movie over N synthetic 2048^2 x 30
frames with segmentation="classical" and "unet" (random-init network, head calibrated on frame 0 as bench.py's U-Net leg does),
each with 1 and 3 frames in flight; the host->device upload of one stack, which the driver pays per frame and bench.py's resident
frames do not; and, with HIP events on the library's stream (tip_prof_*), the device transposes of a frame-sized int32 label map
and float64 HC map (tip_transpose2d_dev, the `.T` of predict's (X, Y) results) beside a tip_memcpy_d2d of the same bytes.

    python tools/movie_unet_time.py [--frames 12] [--size 2048] [--z 30] [--inflight 1,3] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_transposes(Y, X, reps):
    """{plane: median device ms of the (X, Y) -> (Y, X) transpose and of a plain copy of the same bytes}, event-timed."""
    from tissue_image_processing_amd import _lib
    lib = _lib.lib()
    out = {}
    _lib.prof_enable(True)
    for elem, label in ((4, "labels_i32"), (8, "hc_f64")):
        nbytes = Y * X * elem
        src, dst = _lib.DeviceBuffer(nbytes), _lib.DeviceBuffer(nbytes)
        _lib.check(lib.tip_memset(src.ptr, 1, nbytes))
        ms = {"transpose": [], "memcpy_d2d": []}
        for _ in range(reps + 2):                 # (the first two calls warm up: code object, clocks)
            _lib.prof_reset()
            _lib.transpose2d_dev(src.ptr, dst.ptr, X, Y, elem)
            _lib.check(lib.tip_memcpy_d2d(dst.ptr, src.ptr, nbytes))
            _lib.check(lib.tip_sync())
            rep = _lib.prof_report()
            ms["transpose"].append(rep["transpose2d_b%d" % elem][1])
            ms["memcpy_d2d"].append(rep["memcpy_d2d"][1])
        rec = {k: round(float(np.median(v[2:])), 4) for k, v in ms.items()}
        rec["bytes"] = nbytes
        rec["transpose_GBps_read_plus_write"] = round(2e-6 * nbytes / rec["transpose"], 1)
        rec["memcpy_GBps_read_plus_write"] = round(2e-6 * nbytes / rec["memcpy_d2d"], 1)
        out[label] = rec
    _lib.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--z", type=int, default=30)
    ap.add_argument("--inflight", default="1,3")
    ap.add_argument("--reps", type=int, default=20, help="timed calls of each transpose / copy")
    args = ap.parse_args()
    import torch
    from tissue_image_processing_amd import _lib, movie, synthetic
    from tissue_image_processing_amd.prediction_local import SegmentationPredictor
    Y = X = args.size
    T, Z = args.frames, args.z
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, 2, seed=5)
    # two distinct frames, alternated (a 2048^2 x 30 stack is 0.5 GB of pinned memory)
    pair = [torch.from_numpy(synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc)).pin_memory() for t in range(2)]
    source = lambda t: pair[t % 2]
    fixed = np.stack([pair[0][1].numpy().max(0).T, pair[0][0].numpy().max(0).T]).astype(np.float64)      # (atoh, zo) as (2, X, Y)

    def factory(device):
        pred = SegmentationPredictor(None, (2, X, Y), device=device)
        padded, _ = pred.prepare_image(fixed)
        pred.model.calibrate_head(padded, 0.5)
        return pred

    out = {"frames": T, "size": [Y, X, Z]}
    _lib.init(0)
    d_stack = _lib.DeviceBuffer(pair[0].numel() * 2)
    ups = []
    for _ in range(5):
        t0 = time.perf_counter()
        _lib.check(_lib.lib().tip_memcpy_h2d(d_stack.ptr, pair[0].data_ptr(), pair[0].numel() * 2))
        ups.append(1e3 * (time.perf_counter() - t0))
    d_stack.free()
    out["upload_ms_per_frame"] = round(float(np.median(ups)), 3)
    for seg in ("classical", "unet"):
        for inflight in [int(v) for v in args.inflight.split(",")]:
            kw = dict(segmentation="unet", predictor_factory=factory) if seg == "unet" else {}
            backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, inflight=inflight, **kw)
            try:
                movie.process_movie(T, source, backend)                 # warm-up: workspaces, code objects, every worker's predictor
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tabs, ids = movie.process_movie(T, source, backend)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                rec = {"wall_s": round(wall, 4), "ms_per_frame": round(1e3 * wall / T, 3), "frames_per_s": round(T / wall, 2),
                       "rows_per_frame": int(tabs[0]["area"].size)}
                if seg == "unet":
                    rec["network_modes"] = sorted(set(str(m) for m in backend.unet_modes.values()))
            finally:
                backend.close()
            out["%s_inflight%d" % (seg, inflight)] = rec
    out["transposes"] = time_transposes(Y, X, args.reps)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
