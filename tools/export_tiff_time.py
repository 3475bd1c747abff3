"""Ways from a finished movie on one MI355X to the exported TIFF (tracking labels and cell types, T x 2 x 1 x Y x X uint16), timed:
N typed synthetic 2048^2 frames, one process_movie, then every route --reps times after a warm-up.

  --mode device   movie.export_tiff with codes "fixed" and "dynamic": wall time, the time of its two kernels (HIP events, milliseconds per
                  movie: export_maps_u16 and deflate_strips_*), the file size, and the size the same strips take under zlib level 6.
  --mode host     what the driver offered before: download every frame's label and type map (backend.labels[t].download,
                  fetch_cell_types), build the array on the host, save_tiff(compression="zlib") and save_tiff() uncompressed.
                  This mode uses nothing newer than save_tiff's compression keyword, so it runs on the parent commit's tree.

The JSON holds every wall time with median, min and max.  --host-json embeds a host-mode result in a device-mode one.

    python tools/export_tiff_time.py --mode device [--frames 6] [--size 2048] [--z 8] [--reps 5] [--host-json FILE] [--out FILE]
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


def stats(values):
    return {"median": round(float(np.median(values)), 4), "min": round(float(min(values)), 4), "max": round(float(max(values)), 4),
            "all": [round(float(v), 4) for v in values]}


def host_array(backend, ids, T, Y, X):
    out = np.zeros((T, 2, 1, Y, X), np.uint16)
    for t in range(T):
        labels = backend.labels[t].download((Y, X), np.int32)
        types = backend.fetch_cell_types(t)
        out[t, 0, 0] = np.insert(np.asarray(ids[t], np.int64), 0, 0)[labels].astype(np.uint16)
        types = types.copy()
        types[types == 0] = 2
        types[types == 255] = 0
        out[t, 1, 0] = types
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("device", "host"), required=True)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--z", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-json", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tissue_image_processing_amd import _lib, movie, synthetic, tiff
    Y = X = args.size
    T, Z = args.frames, args.z
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
    stacks = {t: synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)}
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, cell_types=dict(threshold=0.03, percentage_above_threshold=3, peak_window_size=0))
    tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend)
    tmp = tempfile.mkdtemp()
    out = {"mode": args.mode, "frames": T, "size": [Y, X, Z], "reps": args.reps, "rows_per_frame": int(tabs[0]["area"].size),
           "raw_bytes": T * 2 * Y * X * 2}
    if args.mode == "host":
        for name, kw in (("zlib", dict(compression="zlib")), ("uncompressed", {})):
            path, walls = os.path.join(tmp, name + ".tif"), []
            for rep in range(args.reps + 1):             # rep 0 is the warm-up
                t0 = time.perf_counter()
                tiff.save_tiff(path, host_array(backend, ids, T, Y, X), axes="TCZYX", data_type="uint16", **kw)
                walls.append(time.perf_counter() - t0)
                print("host %s rep %d: %.3f s" % (name, rep, walls[-1]), file=sys.stderr, flush=True)
            out["fetch_and_save_tiff_" + name] = {"wall_s": stats(walls[1:]), "file_bytes": os.path.getsize(path)}
    else:
        _lib.prof_enable(True)
        paths = {codes: os.path.join(tmp, codes + ".tif") for codes in ("fixed", "dynamic")}
        walls = {codes: [] for codes in paths}
        kernels = {codes: {"export_maps_u16": [], "deflate_strips": []} for codes in paths}
        for rep in range(args.reps + 1):                 # rep 0 is the warm-up; the two codes alternate
            for codes, path in paths.items():
                _lib.prof_reset()
                t0 = time.perf_counter()
                movie.export_tiff(path, T, backend, ids, codes=codes)
                walls[codes].append(time.perf_counter() - t0)
                report = _lib.prof_report()
                kernels[codes]["export_maps_u16"].append(sum(ms for name, (_, ms) in report.items() if name == "export_maps_u16"))
                kernels[codes]["deflate_strips"].append(sum(ms for name, (_, ms) in report.items() if name.startswith("deflate_strips")))
                print("device %s rep %d: %.4f s (kernels %.3f + %.3f ms)" % (codes, rep, walls[codes][-1], kernels[codes]["export_maps_u16"][-1],
                                                                             kernels[codes]["deflate_strips"][-1]), file=sys.stderr, flush=True)
        for codes, path in paths.items():
            out["export_tiff_" + codes] = {"wall_s": stats(walls[codes][1:]), "file_bytes": os.path.getsize(path),
                                           "kernel_ms_per_movie": {k: stats(v[1:]) for k, v in kernels[codes].items()}}
        _lib.prof_enable(False)
        image = tiff.read_tiff(path)[0]
        np.testing.assert_array_equal(image, host_array(backend, ids, T, Y, X))      # (the timed file is the right one)
        table = tiff.tiff_page_table(path)
        rps = table.pages[0].rows_per_strip
        planes = image.reshape(-1, Y, X)
        out["rows_per_strip"] = int(rps)
        out["zlib6_strip_bytes"] = int(sum(len(zlib.compress(p[r:r + rps].tobytes(), 6)) for p in planes for r in range(0, Y, rps)))
        for codes in ("fixed", "dynamic"):
            strips = sum(sum(pg.counts) for pg in tiff.tiff_page_table(os.path.join(tmp, codes + ".tif")).pages)
            out["export_tiff_" + codes]["strip_bytes"] = int(strips)
            out["export_tiff_" + codes]["strip_bytes_over_zlib6"] = round(strips / out["zlib6_strip_bytes"], 3)
            out["export_tiff_" + codes]["raw_over_strip_bytes"] = round(out["raw_bytes"] / strips, 2)
        if args.host_json:
            with open(args.host_json) as fh:
                out["host_routes_at_parent_commit"] = json.load(fh)
    backend.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
