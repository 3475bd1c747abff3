"""The device deflate call with fixed and with per-chunk dynamic Huffman codes (csrc/tip_deflate.hip), rows rule, on one GPU.

call   A Voronoi label map at SURVEY's cell density tiled to size^2 (tools/deflate_rows_time.py's), as int32 labels and as its
       uint8 type map.  After a warm-up the fixed rows call (tip_deflate_rows_dev) and the dynamic rows call
       (tip_deflate_dynamic_dev) alternate --reps times; per coding and map the JSON holds every kernel's HIP-event time (the
       library's profiler: median over the repetitions and every value), the call's wall time, the stream's bytes and its ratio,
       beside zlib level 6's bytes.  Both streams are inflated once with zlib.  --lib times another build of the library (a
       diagnostic build with -DDF_TIME_SKIP_CODES, whose dynamic kernel skips the code construction and the header: its
       streams are not checked).
movie  N synthetic size^2 x z frames, cell types on, --inflight frames in flight: process_movie with
       archive=dict(matches="rows") and with archive=dict(matches="rows", codes="dynamic"), then save_seg of each, and the
       driver's route without `archive` (download, tables, Tissue.save: tools/movie_seg_time.py's route b), alternating --reps times
       after a warm-up: medians, spreads (max - min), archive sizes, stream bytes per frame.

    python tools/deflate_dynamic_time.py call [--size 2048] [--reps 5] [--lib path] [--out call.json]
    python tools/deflate_dynamic_time.py movie [--frames 6] [--size 2048] [--z 30] [--inflight 2] [--reps 5] [--out movie.json]
    python tools/deflate_dynamic_time.py merge call.json movie.json [skip.json] --out profiles/deflate_dynamic_time.json
"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _write(out, path):
    text = json.dumps(out, indent=1)
    print(text)
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")


def call(args):
    from deflate_rows_time import voronoi_maps
    if args.lib:
        os.environ["TISSUE_HIP_LIB"] = os.path.abspath(args.lib)
    from tissue_image_processing_amd import _deflate, _lib
    _lib.init(0)
    labels, types = voronoi_maps(args.size)
    out = {"size": args.size, "reps": args.reps, "library": args.lib or "default", "maps": {}}
    for name, array, e in (("labels_int32", labels, 4), ("types_uint8", types, 1)):
        data = array.tobytes()
        src, dst = _lib.DeviceBuffer(len(data)), _lib.DeviceBuffer(_deflate.runs_bound(len(data)))
        src.upload(array)
        row_bytes = array.shape[1] * e
        calls = {"fixed": lambda: _deflate.deflate_rows_dev(src.ptr, len(data), e, row_bytes, dst.ptr, dst.nbytes),
                 "dynamic": lambda: _deflate.deflate_dynamic_dev(src.ptr, len(data), e, row_bytes, dst.ptr, dst.nbytes)}
        rec = {coding: {"wall_ms": [], "kernels_ms": {}} for coding in calls}
        for rep in range(args.reps + 1):         # rep 0 is the warm-up
            for coding, fn in calls.items():
                _lib.prof_enable(True)
                _lib.prof_reset()
                t0 = time.perf_counter()
                size, crc = fn()
                wall = 1e3 * (time.perf_counter() - t0)
                report = _lib.prof_report()
                _lib.prof_enable(False)
                assert crc == zlib.crc32(data)
                rec[coding]["bytes"] = size
                if rep == 0 and not args.lib:    # inflate each stream once
                    d = zlib.decompressobj(-15)
                    assert d.decompress(dst.download((size,), np.uint8).tobytes() + _deflate.FINAL_BLOCK) + d.flush() == data, coding
                if rep:
                    rec[coding]["wall_ms"].append(wall)
                    for kernel, (_, ms) in report.items():
                        rec[coding]["kernels_ms"].setdefault(kernel, []).append(ms)
        for coding in calls:
            rec[coding] = {"bytes": rec[coding]["bytes"], "ratio": round(rec[coding]["bytes"] / len(data), 4),
                           "wall_ms_median": round(float(np.median(rec[coding]["wall_ms"])), 4),
                           "kernels_ms_median": {k: round(float(np.median(v)), 4) for k, v in rec[coding]["kernels_ms"].items()},
                           "kernels_ms_all": {k: [round(x, 4) for x in v] for k, v in rec[coding]["kernels_ms"].items()}}
        rec["raw_bytes"] = len(data)
        rec["zlib6_bytes"] = len(zlib.compress(data, 6)) - 6
        out["maps"][name] = rec
        src.free()
        dst.free()
    _write(out, args.out)


def movie(args):
    import torch
    from movie_seg_time import stats, tissue_route
    from tissue_image_processing_amd import movie as mv, synthetic
    Y = X = args.size
    T, Z = args.frames, args.z
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
    stacks = {t: torch.from_numpy(synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc)).pin_memory()
              for t in range(T)}
    opts = dict(threshold=0.03, percentage_above_threshold=3, peak_window_size=0)
    channels = ("zo", "atoh")
    backends = {"plain": mv.GpuFrameBackend(2, Z, Y, X, device=0, inflight=args.inflight, cell_types=opts),
                "fixed": mv.GpuFrameBackend(2, Z, Y, X, device=0, inflight=args.inflight, cell_types=opts,
                                            archive=dict(type_name="HC", matches="rows")),
                "dynamic": mv.GpuFrameBackend(2, Z, Y, X, device=0, inflight=args.inflight, cell_types=opts,
                                              archive=dict(type_name="HC", matches="rows", codes="dynamic"))}
    tmp = tempfile.mkdtemp()
    paths = {k: os.path.join(tmp, k) for k in ("fixed", "dynamic", "tissue")}
    rec = {k: [] for k in ("movie_plain", "movie_fixed", "movie_dynamic", "save_seg_fixed", "save_seg_dynamic", "tissue_download",
                           "tissue_tables", "tissue_save")}

    def run(backend):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tabs, ids = mv.process_movie(T, lambda t: stacks[t], backend, block_frames=2)
        torch.cuda.synchronize()
        return tabs, ids, time.perf_counter() - t0

    for rep in range(args.reps + 1):             # rep 0 is the warm-up
        walls = {}
        for name in ("plain", "fixed", "dynamic"):
            tabs, ids, walls["movie_" + name] = run(backends[name])
            if name == "plain":
                b = tissue_route(paths["tissue"], backends[name], tabs, ids, T, Y, X, channels)
                walls.update(tissue_download=b[0], tissue_tables=b[1], tissue_save=b[2])
            else:
                t0 = time.perf_counter()
                mv.save_seg(paths[name], T, backends[name], tabs, ids, channel_names=channels)
                walls["save_seg_" + name] = time.perf_counter() - t0
        print("rep %d: %s" % (rep, {k: round(v, 3) for k, v in walls.items()}), file=sys.stderr, flush=True)
        if rep:
            for k in rec:
                rec[k].append(walls[k])
    per_frame = {k: stats([1e3 * v / T for v in rec["movie_" + k]]) for k in ("plain", "fixed", "dynamic")}
    diff = stats([1e3 * (d - f) / T for d, f in zip(rec["movie_dynamic"], rec["movie_fixed"])])
    streams = {k: [(len(backends[k].archive_frames[t]["labels"][0]), len(backends[k].archive_frames[t]["types"][0])) for t in range(T)]
               for k in ("fixed", "dynamic")}
    out = {"frames": T, "size": [Y, X, Z], "inflight": args.inflight, "reps": args.reps,
           "seconds": {k: stats(v) for k, v in rec.items()},
           "process_movie_ms_per_frame": per_frame,
           "dynamic_minus_fixed_ms_per_frame": diff,
           "difference_inside_the_spread": bool(abs(diff["median"]) <= max(per_frame["fixed"]["spread"], per_frame["dynamic"]["spread"])),
           "tissue_route_total_s": stats([rec["tissue_download"][i] + rec["tissue_tables"][i] + rec["tissue_save"][i]
                                          for i in range(args.reps)]),
           "archive_bytes": {"rows_fixed": os.path.getsize(paths["fixed"] + ".seg"), "rows_dynamic": os.path.getsize(paths["dynamic"] + ".seg"),
                             "tissue_save_zlib": os.path.getsize(paths["tissue"] + ".seg")},
           "device_stream_bytes_per_frame": {"labels_fixed": int(np.mean([s[0] for s in streams["fixed"]])),
                                             "types_fixed": int(np.mean([s[1] for s in streams["fixed"]])),
                                             "labels_dynamic": int(np.mean([s[0] for s in streams["dynamic"]])),
                                             "types_dynamic": int(np.mean([s[1] for s in streams["dynamic"]])),
                                             "raw_labels": Y * X * 4, "raw_types": Y * X}}
    for backend in backends.values():
        backend.close()
    _write(out, args.out)


def merge(args):
    out = {}
    for key, path in zip(("call", "movie", "call_without_code_construction"), args.parts):
        with open(path) as fh:
            out[key] = json.load(fh)
    _write(out, args.out)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="part", required=True)
    c = sub.add_parser("call")
    c.add_argument("--size", type=int, default=2048)
    c.add_argument("--reps", type=int, default=5)
    c.add_argument("--lib", default=None)
    c.add_argument("--out", default=None)
    m = sub.add_parser("movie")
    m.add_argument("--frames", type=int, default=6)
    m.add_argument("--size", type=int, default=2048)
    m.add_argument("--z", type=int, default=30)
    m.add_argument("--inflight", type=int, default=2)
    m.add_argument("--reps", type=int, default=5)
    m.add_argument("--out", default=None)
    g = sub.add_parser("merge")
    g.add_argument("parts", nargs="+")
    g.add_argument("--out", default=None)
    args = ap.parse_args()
    {"call": call, "movie": movie, "merge": merge}[args.part](args)


if __name__ == "__main__":
    main()
