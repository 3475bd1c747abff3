"""Where a deflate-compressed TIFF movie should be inflated, measured on one MI355X: --frames time points of bench.py's synthetic
movie (2048^2 x 30, C = 2, uint16; --distinct different ones, repeated) written by save_tiff(compression="zlib") with about 64 KB
of raw data per strip, with and without predictor 2, and once with one strip per page (predictor 2, --distinct frames).

Per file and frame: the compressed bytes and the strip count; the gather of the strips into the pinned buffer; the host-to-device
copy of that buffer; tip_inflate_strips_dev (the call's wall time, which holds its table download and sort, and the kernels'
event times) and tip_tiff_finish_u16_dev; and the host alternative on the same box -- zlib over the frame's strips on 16 threads,
the predictor undone in numpy, plus the upload of the raw frame from pinned memory.

Then process_movie, classical segmentation, frames/s from (a) the frames as pinned in-memory arrays (the array path is the parent
commit's, unchanged), (b) the compressed file with decode="device", (c) the compressed file with decode="host"; the routes
alternate --reps times after one warm-up of each, every wall time is kept, medians and spreads (max - min) reported.

    python tools/tiff_decode_time.py [--frames 6] [--distinct 2] [--size 2048] [--z 30] [--inflight 2] [--reps 3]
                                     [--out profiles/tiff_inflate_time.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(values):
    return {"median": round(float(np.median(values)), 5), "spread": round(float(max(values) - min(values)), 5),
            "all": [round(float(v), 5) for v in values]}


def host_decode(table, src, t, C, Z, pool):
    """the frame's strips through zlib on the pool's threads, the predictor undone in numpy -> (seconds inflate, seconds predictor, stack)"""
    pages = [table.pages[src.page_index(t, c, z)] for c in range(C) for z in range(Z)]
    jobs = [(pg, k) for pg in pages for k in range(pg.strips)]
    t0 = time.perf_counter()
    parts = list(pool.map(lambda j: zlib.decompress(table.buf[j[0].offsets[j[1]]:j[0].offsets[j[1]] + j[0].counts[j[1]]]), jobs))
    t1 = time.perf_counter()
    first = pages[0]
    stack = np.frombuffer(b"".join(parts), "<u2").reshape(C * Z * first.rows, first.cols)
    if first.predictor == 2:
        stack = np.cumsum(stack, axis=1, dtype=np.uint16)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, stack


def annotate(result):
    """The strip-count threshold of decode="auto", from the two measured layouts.  The device decodes one strip per wave, so with
    few strips its time is one strip's serial decode, which shrinks as 1 / strips while there are waves to spare; the host's time
    does not depend on the strip count.  With n1 strips the device took d1 and the host h1: they meet at n1 * d1 / h1 strips (of
    equal size).  movie.AUTO_DEVICE_MIN_STRIPS is the next power of two above that, checked against the many-strip layout."""
    from tissue_image_processing_amd import movie
    one, many = result["files"]["one_strip_per_page_predictor2"], result["files"]["strips_64k_predictor2"]
    n1 = one["per_frame"][0]["strips"]
    d1, h1 = one["device_route_s"]["median"], one["host_route_s"]["median"]
    cross = n1 * d1 / h1
    result["auto_threshold"] = {
        "one_strip_per_page": {"strips": n1, "device_route_s": d1, "host_route_s": h1, "faster": "device" if d1 < h1 else "host"},
        "strips_64k": {"strips": many["per_frame"][0]["strips"], "device_route_s": many["device_route_s"]["median"],
                       "host_route_s": many["host_route_s"]["median"],
                       "faster": "device" if many["device_route_s"]["median"] < many["host_route_s"]["median"] else "host"},
        "crossover_strips": round(cross, 1),
        "AUTO_DEVICE_MIN_STRIPS": movie.AUTO_DEVICE_MIN_STRIPS,
        "rule": "decode='auto' is 'device' when frame bytes / largest strip's bytes >= AUTO_DEVICE_MIN_STRIPS (16-bit deflate strips, GPU backend)",
    }
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--annotate", default=None, help="a JSON this tool wrote: only (re)compute its auto_threshold block into --out")
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--z", type=int, default=30)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "tiff_inflate_time.json"))
    args = ap.parse_args()
    if args.annotate:
        with open(args.annotate) as fh:
            result = annotate(json.load(fh))
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        print(json.dumps(result["auto_threshold"]))
        return
    import torch
    from tissue_image_processing_amd import _inflate, _lib, movie, synthetic, tiff
    T, Y, X, Z, C = args.frames, args.size, args.size, args.z, 2
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
    t0 = time.perf_counter()
    distinct = [synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc) for t in range(min(args.distinct, T))]
    frames = [distinct[t % len(distinct)] for t in range(T)]
    print("frames made in %.1f s" % (time.perf_counter() - t0), flush=True)
    tmp = tempfile.mkdtemp(prefix="tiffmovie")
    files = {}
    for name, pred, rps, n in (("strips_64k_predictor1", 1, None, T), ("strips_64k_predictor2", 2, None, T),
                               ("one_strip_per_page_predictor2", 2, Y, min(args.distinct, T))):
        path = os.path.join(tmp, name + ".tif")
        t0 = time.perf_counter()
        tiff.save_tiff(path, np.stack(frames[:n]), axes="TCZYX", compression="zlib", predictor=pred, rowsperstrip=rps)
        files[name] = (path, n)
        print("%s: %d frames, %.1f MB, written in %.1f s" % (name, n, os.path.getsize(path) / 1e6, time.perf_counter() - t0), flush=True)
    raw_bytes = C * Z * Y * X * 2
    result = {"frame": "%dx%dx%d C=%d uint16, %d raw bytes" % (Y, X, Z, C, raw_bytes), "frames": T, "distinct_frames": len(distinct),
              "host_threads": 16, "files": {}}

    lib = _lib.init(0)
    pool = ThreadPoolExecutor(16)
    pinned_raw = torch.empty(raw_bytes, dtype=torch.uint8, pin_memory=True)
    d_raw = _lib.DeviceBuffer(raw_bytes)
    for name, (path, n) in files.items():
        src = movie.tiff_frame_source(path, decode="device")
        table = tiff.tiff_page_table(path)
        rows = []
        for rep in range(2):                                   # the first pass over the file is the warm-up
            rows = []
            for t in range(n):
                t0 = time.perf_counter()
                f = src(t)
                gather = time.perf_counter() - t0
                packed, status, stack = _lib.DeviceBuffer(f.nbytes), _lib.DeviceBuffer(4 * f.n_strips), _lib.DeviceBuffer(raw_bytes)
                _lib.check(lib.tip_sync())
                t0 = time.perf_counter()
                _lib.check(lib.tip_memcpy_h2d(packed.ptr, f.host_ptr(), f.nbytes))
                h2d = time.perf_counter() - t0
                _lib.prof_enable(True)
                _lib.prof_reset()
                t0 = time.perf_counter()
                n_bad = _inflate.inflate_strips_dev(packed.ptr, f.src_bytes, packed.ptr + f.table_at, f.n_strips, 1, stack.ptr, raw_bytes, status.ptr)
                call = time.perf_counter() - t0
                t0 = time.perf_counter()
                _inflate.tiff_finish_u16_dev(stack.ptr, C * Z * Y, X, f.predictor, f.swap_bytes)
                _lib.check(lib.tip_sync())
                finish = time.perf_counter() - t0
                kernels = _lib.prof_report()
                _lib.prof_enable(False)
                assert n_bad == 0
                inflate_s, predictor_s, want = host_decode(table, src_host(path), t, C, Z, pool)
                if rep == 0:
                    assert np.array_equal(stack.download((C * Z * Y, X), np.uint16), want), (name, t)      # faster and different is not faster
                pinned_raw.numpy()[:] = want.view(np.uint8).ravel()
                t0 = time.perf_counter()
                _lib.check(lib.tip_memcpy_h2d(d_raw.ptr, pinned_raw.data_ptr(), raw_bytes))
                raw_h2d = time.perf_counter() - t0
                rows.append(dict(frame=t, compressed_bytes=int(f.src_bytes), strips=int(f.n_strips), gather_s=round(gather, 5),
                                 h2d_s=round(h2d, 5), inflate_call_s=round(call, 5),
                                 inflate_kernel_ms=round(kernels.get("inflate_strips", (0, 0.0))[1], 3),
                                 count_kernel_ms=round(kernels.get("inflate_count_bad", (0, 0.0))[1], 3),
                                 finish_call_s=round(finish, 5), finish_kernel_ms=round(kernels.get("tiff_finish_u16", (0, 0.0))[1], 3),
                                 host_inflate_16_threads_s=round(inflate_s, 5), host_predictor_numpy_s=round(predictor_s, 5),
                                 raw_h2d_s=round(raw_h2d, 5)))
                f.release()
                for b in (packed, status, stack):
                    b.free()
        dev = [r["gather_s"] + r["h2d_s"] + r["inflate_call_s"] + r["finish_call_s"] for r in rows]
        host = [r["host_inflate_16_threads_s"] + r["host_predictor_numpy_s"] + r["raw_h2d_s"] for r in rows]
        result["files"][name] = dict(file_bytes=os.path.getsize(path), per_frame=rows, device_route_s=stats(dev), host_route_s=stats(host))
        print(name, "device route", stats(dev)["median"], "s  host route (16 threads)", stats(host)["median"], "s", flush=True)

    # process_movie, classical segmentation
    pinned = [torch.from_numpy(fr).pin_memory() for fr in distinct]
    routes = {"a_arrays_pinned": lambda: (lambda t: pinned[t % len(pinned)])}
    for name in ("strips_64k_predictor2", "strips_64k_predictor1"):
        routes["b_device_decode_" + name] = lambda name=name: movie.tiff_frame_source(files[name][0], decode="device")
        routes["c_host_decode_" + name] = lambda name=name: movie.tiff_frame_source(files[name][0], decode="host")
    walls = {k: [] for k in routes}
    for rep in range(args.reps + 1):                            # rep 0 warms every route up
        for key, make in routes.items():
            backend = movie.GpuFrameBackend(C, Z, Y, X, device=0, inflight=args.inflight)
            source = make()
            _lib.check(lib.tip_sync())
            t0 = time.perf_counter()
            movie.process_movie(T, source, backend, 0, 1, None, "cpu", np.zeros((T, 2)), block_frames=max(1, args.inflight))
            wall = time.perf_counter() - t0
            backend.close()
            if rep:
                walls[key].append(wall)
            print(rep, key, "%.3f s" % wall, flush=True)
    result["process_movie"] = {k: dict(wall_s=stats(v), frames_per_s=round(T / float(np.median(v)), 2)) for k, v in walls.items()}
    result["process_movie"]["inflight"] = args.inflight
    annotate(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({k: v["frames_per_s"] for k, v in result["process_movie"].items() if isinstance(v, dict)}))


_HOST_SOURCES = {}


def src_host(path):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    if path not in _HOST_SOURCES:
        _HOST_SOURCES[path] = bim.open_image(path)
    return _HOST_SOURCES[path]


if __name__ == "__main__":
    main()
