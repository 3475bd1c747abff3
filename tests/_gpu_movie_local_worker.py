"""GPU side of the process_movie(local_drifts=...) tests: the small drifting movie on a GpuFrameBackend that installs given
label maps and planes (_gpu_movie_piv_worker.installed_backend_class), and the worker for the 2-process run (both ranks on
GPU 0, collectives over gloo)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MULTI = dict(window_size=48, step_size=16)       # 144 x 168: 48 windows, extents 48 x 48 and 48 x 56 (Bluestein rows)
SINGLE = dict(window_size=143, step_size=32)     # one window, the whole frame


def run(out_path, rank, world, dist):
    from _gpu_movie_piv_worker import installed_backend_class
    from _movie_worker import drifting_movie
    from tissue_image_processing_amd import movie
    frames = drifting_movie(4)
    backend = installed_backend_class()(*frames[0][0].shape)
    try:
        tabs, ids = movie.process_movie(len(frames), lambda t: frames[t], backend, rank, world, dist, "cpu", block_frames=1,
                                        local_drifts=MULTI)
    finally:
        backend.close()
    if rank == 0:
        np.savez(out_path, n=len(frames), **{"ids_%d" % t: ids[t] for t in range(len(frames))})


if __name__ == "__main__":
    from gloo_launch import gloo_group
    with gloo_group(single=False) as (rank, world, dist):
        run(sys.argv[1], rank, world, dist)
