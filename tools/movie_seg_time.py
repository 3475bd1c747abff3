"""Ways from a finished movie on one MI355X to a `.seg` archive, timed: N synthetic 2048^2 frames, cell types on.

  (a) GpuFrameBackend(archive=...) + movie.save_seg: the label and type maps are deflated on the device inside process_movie
      (csrc/tip_deflate.hip), save_seg wraps the streams and builds the frame tables from what the driver kept.  Its cost is
      what `archive` adds to process_movie plus the save_seg call.
  (a') the same with archive=dict(matches="rows"): matches to the row above beside the runs (tip_deflate_rows_dev), a smaller
      archive from a slower deflate call.
  (b) what the driver offers without `archive`: download every frame's label and type map, put them into a Tissue with the
      frame's table (calculate_frame_cellinfo on the downloaded labels, the type columns from process_movie's tables, the
      track ids) and call Tissue.save, which deflates every member with the host's zlib.

After a warm-up of both, the routes alternate --reps times; the JSON holds every wall time, the medians and the spreads
(max - min), the archive sizes and process_movie's wall per frame with and without `archive`.

    python tools/movie_seg_time.py [--frames 6] [--size 2048] [--z 30] [--inflight 2] [--reps 5] [--out profiles/movie_seg_time.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tissue_route(path, backend, tabs, ids, T, Y, X, channel_names):
    """Route (b) -> seconds spent on (download, tables, Tissue.save)."""
    from tissue_image_processing_amd.tissue_info import Tissue
    t0 = time.perf_counter()
    labels = [backend.labels[t].download((Y, X), np.int32) for t in range(T)]
    types = [backend.fetch_cell_types(t) for t in range(T)]
    t1 = time.perf_counter()
    tissue = Tissue(T, channel_names=channel_names)
    tissue.type_names = ["HC"]
    for t in range(T):
        tissue.set_labels(t + 1, labels[t], reset_data=True)
        tissue.calculate_frame_cellinfo(t + 1)
        info = tissue.get_cells_info(t + 1)
        rows = np.flatnonzero(tabs[t]["area"] > 0)
        info.loc[rows, "mean_intensity_HC"] = tabs[t]["mean_intensity"][rows]
        info.loc[:, "valid"] = tabs[t]["valid"].astype(int)
        info.loc[:, "type"] = tabs[t]["type"].astype(np.int64)
        info.loc[:, "label"] = np.asarray(ids[t], np.int64)
        tissue.set_cell_types(t + 1, types[t])
        tissue.drifts[t] = tabs[t]["drift"]
    t2 = time.perf_counter()
    for _ in tissue.save(path):
        pass
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2


def stats(values):
    return {"median": round(float(np.median(values)), 4), "spread": round(float(max(values) - min(values)), 4),
            "all": [round(float(v), 4) for v in values]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--z", type=int, default=30)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from tissue_image_processing_amd import movie, synthetic
    Y = X = args.size
    T, Z = args.frames, args.z
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
    stacks = {t: torch.from_numpy(synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc)).pin_memory()
              for t in range(T)}
    opts = dict(threshold=0.03, percentage_above_threshold=3, peak_window_size=0)
    channels = ("zo", "atoh")
    plain = movie.GpuFrameBackend(2, Z, Y, X, device=0, inflight=args.inflight, cell_types=opts)
    arch = movie.GpuFrameBackend(2, Z, Y, X, device=0, inflight=args.inflight, cell_types=opts, archive=dict(type_name="HC"))
    arch_rows = movie.GpuFrameBackend(2, Z, Y, X, device=0, inflight=args.inflight, cell_types=opts,
                                      archive=dict(type_name="HC", matches="rows"))
    tmp = tempfile.mkdtemp()
    path_a, path_b, path_r = os.path.join(tmp, "a"), os.path.join(tmp, "b"), os.path.join(tmp, "a_rows")
    rec = {k: [] for k in ("movie_plain", "movie_archive", "save_seg", "b_download", "b_tables", "b_save", "movie_archive_rows",
                           "save_seg_rows")}

    def run(backend):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend, block_frames=2)
        torch.cuda.synchronize()
        return tabs, ids, time.perf_counter() - t0

    for rep in range(args.reps + 1):             # rep 0 is the warm-up (workspaces, code objects, pandas' first calls)
        tabs_p, ids_p, w_plain = run(plain)
        tabs_a, ids_a, w_arch = run(arch)
        t0 = time.perf_counter()
        movie.save_seg(path_a, T, arch, tabs_a, ids_a, channel_names=channels)
        w_save = time.perf_counter() - t0
        b = tissue_route(path_b, plain, tabs_p, ids_p, T, Y, X, channels)
        tabs_r, ids_r, w_rows = run(arch_rows)
        t0 = time.perf_counter()
        movie.save_seg(path_r, T, arch_rows, tabs_r, ids_r, channel_names=channels)
        w_save_rows = time.perf_counter() - t0
        print("rep %d: movie %.3f / %.3f / %.3f s (plain, runs, rows), save_seg %.3f / %.3f s, Tissue route %.3f + %.3f + %.3f s"
              % ((rep, w_plain, w_arch, w_rows, w_save, w_save_rows) + b), file=sys.stderr, flush=True)
        if rep:
            for k, v in zip(rec, (w_plain, w_arch, w_save) + b + (w_rows, w_save_rows)):
                rec[k].append(v)
    n = args.reps
    a_total = [rec["movie_archive"][i] - rec["movie_plain"][i] + rec["save_seg"][i] for i in range(n)]
    r_total = [rec["movie_archive_rows"][i] - rec["movie_plain"][i] + rec["save_seg_rows"][i] for i in range(n)]
    streams_r = [(len(arch_rows.archive_frames[t]["labels"][0]), len(arch_rows.archive_frames[t]["types"][0])) for t in range(T)]
    b_total = [rec["b_download"][i] + rec["b_tables"][i] + rec["b_save"][i] for i in range(n)]
    streams = [(len(arch.archive_frames[t]["labels"][0]), len(arch.archive_frames[t]["types"][0])) for t in range(T)]
    out = {"frames": T, "size": [Y, X, Z], "inflight": args.inflight, "reps": n, "rows_per_frame": int(tabs_a[0]["area"].size),
           "seconds": {k: stats(v) for k, v in rec.items()},
           "route_a_total_s": stats(a_total), "route_a_rows_total_s": stats(r_total), "route_b_total_s": stats(b_total),
           "route_a_save_seg_only_s": stats(rec["save_seg"]),
           "process_movie_ms_per_frame": {"plain": round(1e3 * float(np.median(rec["movie_plain"])) / T, 3),
                                          "archive": round(1e3 * float(np.median(rec["movie_archive"])) / T, 3),
                                          "archive_rows": round(1e3 * float(np.median(rec["movie_archive_rows"])) / T, 3)},
           "archive_bytes": {"a": os.path.getsize(path_a + ".seg"), "a_rows": os.path.getsize(path_r + ".seg"),
                             "b": os.path.getsize(path_b + ".seg")},
           "device_stream_bytes_per_frame": {"labels": int(np.mean([s[0] for s in streams])), "types": int(np.mean([s[1] for s in streams])),
                                             "labels_rows": int(np.mean([s[0] for s in streams_r])),
                                             "types_rows": int(np.mean([s[1] for s in streams_r])),
                                             "raw_labels": Y * X * 4, "raw_types": Y * X}}
    out["a_below_b_by_more_than_bs_spread"] = bool(out["route_b_total_s"]["median"] - out["route_a_total_s"]["median"]
                                                   > out["route_b_total_s"]["spread"])
    plain.close()
    arch.close()
    arch_rows.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
