"""The device deflate call with and without matches to the row above (csrc/tip_deflate.hip), timed with HIP events on one GPU:
a Voronoi label map at SURVEY's cell density (one cell per 900 px, zero lines between cells) tiled to size^2, as int32 labels
and as its uint8 type map.  After a warm-up the two rules alternate --reps times; per rule and map the JSON holds every kernel's
HIP-event time (the library's profiler: median over the repetitions), the call's wall time, the stream's bytes and its ratio.
--movie takes the JSON of tools/movie_seg_time.py along under "movie".

    python tools/deflate_rows_time.py [--size 2048] [--reps 5] [--movie movie_seg_time.json] [--out profiles/deflate_rows_time.json]
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def voronoi_maps(size, tile=256, seed=5):
    rng = np.random.default_rng(seed)
    n = round(tile * tile / 900.0)
    sy, sx = rng.uniform(0, tile, n), rng.uniform(0, tile, n)
    yy, xx = np.mgrid[0:tile, 0:tile]
    cell = np.argmin((yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2, axis=-1) + 1
    line = np.zeros((tile, tile), bool)
    line[:, :-1] |= cell[:, :-1] != cell[:, 1:]
    line[:-1, :] |= cell[:-1, :] != cell[1:, :]
    labels = np.where(line, 0, cell).astype(np.int32)
    reps = -(-size // tile)
    labels = np.tile(labels, (reps, reps))[:size, :size].copy()
    types = np.where(labels == 0, 255, labels % 3 == 0).astype(np.uint8)
    return labels, types


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--movie", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tissue_image_processing_amd import _deflate, _lib
    _lib.init(0)
    labels, types = voronoi_maps(args.size)
    out = {"size": args.size, "reps": args.reps, "maps": {}}
    for name, array, e in (("labels_int32", labels, 4), ("types_uint8", types, 1)):
        data = array.tobytes()
        src, dst = _lib.DeviceBuffer(len(data)), _lib.DeviceBuffer(_deflate.runs_bound(len(data)))
        src.upload(array)
        row_bytes = array.shape[1] * e
        calls = {"runs": lambda: _deflate.deflate_runs_dev(src.ptr, len(data), e, dst.ptr, dst.nbytes),
                 "rows": lambda: _deflate.deflate_rows_dev(src.ptr, len(data), e, row_bytes, dst.ptr, dst.nbytes)}
        rec = {rule: {"wall_ms": [], "kernels_ms": {}} for rule in calls}
        for rep in range(args.reps + 1):         # rep 0 is the warm-up
            for rule, call in calls.items():
                _lib.prof_enable(True)
                _lib.prof_reset()
                t0 = time.perf_counter()
                size, crc = call()
                wall = 1e3 * (time.perf_counter() - t0)
                report = _lib.prof_report()
                _lib.prof_enable(False)
                assert crc == zlib.crc32(data)
                rec[rule]["bytes"] = size
                if rep:
                    rec[rule]["wall_ms"].append(wall)
                    for kernel, (_, ms) in report.items():
                        rec[rule]["kernels_ms"].setdefault(kernel, []).append(ms)
        for rule in calls:
            stream = dst.download((rec[rule]["bytes"],), np.uint8).tobytes() if rule == "rows" else None
            if stream is not None:               # the rows stream is the last one written: inflate it once
                d = zlib.decompressobj(-15)
                assert d.decompress(stream + _deflate.FINAL_BLOCK) + d.flush() == data
            rec[rule] = {"bytes": rec[rule]["bytes"], "ratio": round(rec[rule]["bytes"] / len(data), 4),
                         "wall_ms_median": round(float(np.median(rec[rule]["wall_ms"])), 4),
                         "kernels_ms_median": {k: round(float(np.median(v)), 4) for k, v in rec[rule]["kernels_ms"].items()},
                         "kernels_ms_all": {k: [round(x, 4) for x in v] for k, v in rec[rule]["kernels_ms"].items()}}
        rec["raw_bytes"] = len(data)
        rec["zlib6_bytes"] = len(zlib.compress(data, 6)) - 6
        out["maps"][name] = rec
        src.free()
        dst.free()
    if args.movie:
        with open(args.movie) as fh:
            out["movie"] = json.load(fh)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
