"""Worker for the GPU tests of movie.export_projection: 4 frames of 64 x 64 synthetic stacks (Z 6, C 2), every rank on GPU 0,
collectives over gloo, the backend keeping every frame's projection.  Every rank calls export_projection; rank 0 writes argv[1] and
the z-map file beside it.  The test module imports run_movie for its one-process runs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Z, Y, X, T, C = 6, 64, 64, 4, 2


def stacks():
    from tissue_image_processing_amd import synthetic
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=8)
    return [synthetic.make_stack(Z, Y, X, seed=80 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)]


def run_movie(rank, world, dist, keep_projection=True):
    """-> the backend after process_movie; the caller exports from it and closes it."""
    from tissue_image_processing_amd import movie
    frames = stacks()
    backend = movie.GpuFrameBackend(C, Z, Y, X, device=0, keep_projection=keep_projection)
    drifts = np.zeros((T, 2))
    drifts[1:] = (-0.5, 0.3)
    movie.process_movie(T, lambda t: frames[t], backend, rank, world, dist, "cpu", drifts)
    return backend


if __name__ == "__main__":
    from gloo_launch import gloo_group
    from tissue_image_processing_amd import movie
    with gloo_group(single=False) as (rank, world, dist):
        backend = run_movie(rank, world, dist)
        try:
            movie.export_projection(sys.argv[1], T, backend, rank, world, dist, "cpu")
        finally:
            backend.close()
