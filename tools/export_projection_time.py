"""Ways from z-stacks on one MI355X to the projected movie (T x C x Y x X uint16) and its z-maps, timed: N synthetic 2048^2
two-channel frames, every route --reps times after a warm-up, the alternatives taking turns.

  --mode device   process_movie with and without keep_projection (frames/s), then movie.export_projection under predictor 1 and 2
                  x codes "fixed" and "dynamic": wall time per movie, the time of its kernels (HIP events, milliseconds per movie:
                  max_f64, projection_pages_u16, deflate_strips_*, zmap_u16), the file size and the strips' size.
  --mode host     what the driver offered before: every frame's pipe.fetch_projection() taken during process_movie (frames/s),
                  then save_tiff(..., data_type="uint16") uncompressed and with compression="zlib", predictor=2 (16 host threads).
                  This mode uses nothing newer than save_tiff's compression keyword, so it runs on the parent commit's tree.

The JSON holds every wall time with median, min and max.  --host-json embeds a host-mode result in a device-mode one.

    python tools/export_projection_time.py --mode device [--frames 6] [--size 2048] [--z 8] [--reps 5] [--host-json FILE] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("max_f64", "projection_pages_u16", "deflate_strips", "zmap_u16")


def stats(values):
    return {"median": round(float(np.median(values)), 4), "min": round(float(min(values)), 4), "max": round(float(max(values)), 4),
            "all": [round(float(v), 4) for v in values]}


def run_movie(movie, stacks, shape, **kw):
    """-> (backend, seconds of process_movie)"""
    backend = movie.GpuFrameBackend(*shape, device=0, **kw)
    t0 = time.perf_counter()
    movie.process_movie(len(stacks), lambda t: stacks[t], backend)
    return backend, time.perf_counter() - t0


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
    T, Z, C = args.frames, args.z, 2
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
    stacks = {t: synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)}
    shape = (C, Z, Y, X)
    tmp = tempfile.mkdtemp()
    out = {"mode": args.mode, "frames": T, "size": [Y, X, Z], "channels": C, "reps": args.reps, "raw_bytes": T * C * Y * X * 2}
    if args.mode == "host":
        walls, kept = [], {}
        for rep in range(args.reps + 1):                 # rep 0 is the warm-up
            backend = movie.GpuFrameBackend(*shape, device=0)
            inner = backend.process_frame

            def process_and_fetch(t, stack, inner=inner, backend=backend):
                table = inner(t, stack)
                kept[t] = backend.pipe.fetch_projection()
                return table

            backend.process_frame = process_and_fetch
            t0 = time.perf_counter()
            movie.process_movie(T, lambda t: stacks[t], backend)
            walls.append(time.perf_counter() - t0)
            backend.close()
            print("host process_movie with fetch_projection rep %d: %.3f s" % (rep, walls[-1]), file=sys.stderr, flush=True)
        out["process_movie_with_fetch_projection"] = {"wall_s": stats(walls[1:]), "frames_per_s": stats([T / w for w in walls[1:]])}
        projected = np.stack([kept[t][0] for t in range(T)])
        routes = (("uncompressed", {}), ("zlib_predictor2", dict(compression="zlib", predictor=2)))
        walls = {name: [] for name, _ in routes}
        for rep in range(args.reps + 1):                 # the two routes alternate
            for name, kw in routes:
                path = os.path.join(tmp, name + ".tif")
                t0 = time.perf_counter()
                tiff.save_tiff(path, projected, axes="TCYX", data_type="uint16", **kw)
                walls[name].append(time.perf_counter() - t0)
                print("host save_tiff %s rep %d: %.3f s" % (name, rep, walls[name][-1]), file=sys.stderr, flush=True)
        for name, _ in routes:
            out["save_tiff_" + name] = {"wall_s": stats(walls[name][1:]), "file_bytes": os.path.getsize(os.path.join(tmp, name + ".tif"))}
    else:
        walls = {False: [], True: []}
        backend = None
        for rep in range(args.reps + 1):                 # rep 0 is the warm-up; with and without take turns
            for keep in (False, True):
                if backend is not None:
                    backend.close()
                backend, wall = run_movie(movie, stacks, shape, keep_projection=keep)
                walls[keep].append(wall)
                print("process_movie keep_projection=%s rep %d: %.3f s" % (keep, rep, wall), file=sys.stderr, flush=True)
        for keep in (False, True):
            out["process_movie_keep_projection_%s" % keep] = {"wall_s": stats(walls[keep][1:]),
                                                              "frames_per_s": stats([T / w for w in walls[keep][1:]])}
        # the last backend kept its projections: every export below reads them
        routes = [(p, codes) for p in (1, 2) for codes in ("fixed", "dynamic")]
        name_of = lambda p, codes: "export_projection_predictor%d_%s" % (p, codes)
        walls = {r: [] for r in routes}
        kernels = {r: {k: [] for k in KERNELS} for r in routes}
        _lib.prof_enable(True)
        for rep in range(args.reps + 1):                 # rep 0 is the warm-up; the four routes alternate
            for r in routes:
                path = os.path.join(tmp, name_of(*r) + ".tif")
                _lib.prof_reset()
                t0 = time.perf_counter()
                movie.export_projection(path, T, backend, predictor=r[0], codes=r[1])
                walls[r].append(time.perf_counter() - t0)
                report = _lib.prof_report()
                for k in KERNELS:
                    kernels[r][k].append(sum(ms for name, (_, ms) in report.items() if name.startswith(k)))
                print("%s rep %d: %.4f s (kernels %s ms)" % (name_of(*r), rep, walls[r][-1],
                                                             " + ".join("%.3f" % kernels[r][k][-1] for k in KERNELS)), file=sys.stderr, flush=True)
        _lib.prof_enable(False)
        want = tiff.tiff_normalise(np.stack([backend.fetch_projection(t) for t in range(T)]), "uint16")
        for r in routes:
            path = os.path.join(tmp, name_of(*r) + ".tif")
            np.testing.assert_array_equal(tiff.read_tiff(path)[0], want)      # (the timed file is the right one)
            table = tiff.tiff_page_table(path)
            strips = int(sum(sum(pg.counts) for pg in table.pages))
            both = [a + b for a, b in zip(kernels[r]["projection_pages_u16"][1:], kernels[r]["deflate_strips"][1:])]
            out[name_of(*r)] = {"wall_s": stats(walls[r][1:]), "file_bytes": os.path.getsize(path), "strip_bytes": strips,
                                "raw_over_strip_bytes": round(out["raw_bytes"] / strips, 3), "rows_per_strip": int(table.pages[0].rows_per_strip),
                                "kernel_ms_per_movie": {k: stats(v[1:]) for k, v in kernels[r].items()},
                                "page_and_deflate_kernels_share_of_wall": stats([ms / 1000.0 / w for ms, w in zip(both, walls[r][1:])])}
        out["zmap_file_bytes"] = os.path.getsize(os.path.join(tmp, "zmap_" + name_of(*routes[0]) + ".npy"))
        backend.close()
        if args.host_json:
            with open(args.host_json) as fh:
                out["host_routes_at_parent_commit"] = json.load(fh)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
