"""Worker for the GPU movie tests of the sensory-region filter: 4 frames of 256 x 256 (Z 6, inflight 2, block_frames 1) with
cell_types, neighbor_features and an archive; frame 3's Atoh channel is dark but for a disc inside each of TWO cells, so it has two
hair cells and they span no hull.
Every rank drives GPU 0, collectives over gloo; rank 0 writes the gathered tables to argv[1] (argv[2]: "1" = sensory_region on).
The test module imports run_movie for its one-process runs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Z, Y, X, T = 6, 256, 256, 4
TWO_HC_FRAME = 3
CELL_TYPES = dict(atoh_channel=1, threshold=0.03, percentage_above_threshold=3, peak_window_size=3)
CHANNELS = ("zo", "atoh")


def stacks():
    from tissue_image_processing_amd import synthetic
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=12)
    out = [synthetic.make_stack(Z, Y, X, seed=120 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)]
    # frame 3: a disc of radius 6 round the two sites nearest the frame's centre, the same in every plane; the discs cover 0.35 % of
    # the frame, so its 99th percentile -- the typing's cut -- is 0, and only a cell that holds a disc has a positive 97th percentile
    sites = sites_t[TWO_HC_FRAME]
    yy, xx = np.mgrid[0:Y, 0:X]
    atoh = np.zeros((Y, X), np.uint16)
    for k in np.argsort(((sites - (Y / 2, X / 2)) ** 2).sum(axis=1))[:2]:
        atoh[(yy - sites[k, 0]) ** 2 + (xx - sites[k, 1]) ** 2 <= 36] = 2000
    out[TWO_HC_FRAME][1] = atoh[None]
    return out


def run_movie(out_path, rank, world, dist, sensory, frames=None, **options):
    """-> (backend, tables, ids, path of the archive on rank 0); the caller closes the backend."""
    from tissue_image_processing_amd import movie
    frames = stacks() if frames is None else frames
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, inflight=2, cell_types=CELL_TYPES, neighbor_features=True, archive=True,
                                    sensory_region=sensory, **options)
    tabs, ids = movie.process_movie(T, lambda t: frames[t], backend, rank, world, dist, "cpu", np.zeros((T, 2)), block_frames=1)
    path = movie.save_seg(out_path, T, backend, tabs, ids, rank, world, dist, "cpu", channel_names=CHANNELS)
    return backend, tabs, ids, path


if __name__ == "__main__":
    import warnings
    from gloo_launch import gloo_group
    with gloo_group(single=False) as (rank, world, dist):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            backend, tabs, ids, _ = run_movie(sys.argv[1], rank, world, dist, sys.argv[2] == "1")
        backend.close()
        if rank == 0:
            out = dict(n=T, columns=np.asarray([name for name, _ in backend.extra_columns]))
            for t in range(T):
                for k in tabs[t]:
                    out["%s_%d" % (k, t)] = tabs[t][k]
            np.savez(sys.argv[1] + ".npz", **out)
