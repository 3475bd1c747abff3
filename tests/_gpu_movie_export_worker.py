"""Worker for the GPU tests of movie.export_tiff: 4 frames of 64 x 64 typed synthetic stacks (Z 6), every rank on GPU 0, collectives
over gloo.  Every rank calls export_tiff; rank 0 writes argv[1].  The test module imports run_movie for its one-process run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Z, Y, X, T = 6, 64, 64, 4
CELL_TYPES = dict(atoh_channel=1, threshold=0.03, percentage_above_threshold=3, peak_window_size=3)


def stacks():
    from tissue_image_processing_amd import synthetic
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=8)
    return [synthetic.make_stack(Z, Y, X, seed=80 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)]


def run_movie(out_path, rank, world, dist, frames=None, **export):
    """-> (backend, ids, export_tiff's result); the caller closes the backend."""
    from tissue_image_processing_amd import movie
    frames = stacks() if frames is None else frames
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, cell_types=CELL_TYPES)
    drifts = np.zeros((T, 2))
    drifts[1:] = (-0.5, 0.3)
    _, ids = movie.process_movie(T, lambda t: frames[t], backend, rank, world, dist, "cpu", drifts)
    path = movie.export_tiff(out_path, T, backend, ids, rank, world, dist, "cpu", **export)
    return backend, ids, path


if __name__ == "__main__":
    from gloo_launch import gloo_group
    with gloo_group(single=False) as (rank, world, dist):
        backend = run_movie(sys.argv[1], rank, world, dist)[0]
        backend.close()
