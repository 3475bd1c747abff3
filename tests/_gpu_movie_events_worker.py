"""Worker for the GPU end-to-end test of movie.find_events: the movie of _gpu_movie_seg_worker.py (Z 6, 128 x 160, 5 frames, typed,
inflight 2, block_frames 1) with its SITES edited so that events happen, through process_movie -> find_events ->
save_seg(events=...); every rank on GPU 0, collectives over gloo; rank 0 writes argv[1] + ".seg".  The test module imports
run_movie for its one-process run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _gpu_movie_seg_worker as w      # noqa: E402

# (site, first frame) lists, sites counted in make_movie_sites(Y, X, T, seed=8)'s order; an added site is a (y, x) position
EDITS = dict(remove=[(9, 2)], add=[((64.0, 80.0), 3)], hc_on=[(4, 3)])


def stacks(edits=None):
    from tissue_image_processing_amd import synthetic
    edits = EDITS if edits is None else edits
    sites_t, is_hc = synthetic.make_movie_sites(w.Y, w.X, w.T, seed=8)
    frames = []
    for t in range(w.T):
        sites, hc = sites_t[t].copy(), is_hc.copy()
        for site, first in edits["hc_on"]:
            if t >= first:
                hc[site] = True
        for pos, first in edits["add"]:
            if t >= first:
                sites, hc = np.vstack([sites, np.asarray(pos, np.float64)[None]]), np.append(hc, False)
        gone = [site for site, first in edits["remove"] if t >= first]
        sites, hc = np.delete(sites, gone, axis=0), np.delete(hc, gone)
        frames.append(synthetic.make_stack(w.Z, w.Y, w.X, seed=80 + t, sites=sites, is_hc=hc))
    return frames


def run_movie(out_path, rank, world, dist, frames=None):
    """-> (events table on rank 0, path of the archive on rank 0)"""
    from tissue_image_processing_amd import movie
    frames = stacks() if frames is None else frames
    backend = movie.GpuFrameBackend(2, w.Z, w.Y, w.X, device=0, inflight=2, cell_types=w.CELL_TYPES, archive=dict(type_name="HC"))
    try:
        tabs, ids = movie.process_movie(w.T, lambda t: frames[t], backend, rank, world, dist, "cpu", w.drifts(), block_frames=1)
        events = movie.find_events(w.T, backend, tabs, ids, rank, world, dist, "cpu")
        path = movie.save_seg(out_path, w.T, backend, tabs, ids, rank, world, dist, "cpu", channel_names=w.CHANNELS, events=events)
    finally:
        backend.close()
    return events, path


if __name__ == "__main__":
    from gloo_launch import gloo_group
    with gloo_group(single=False) as (rank, world, dist):
        run_movie(sys.argv[1], rank, world, dist)
