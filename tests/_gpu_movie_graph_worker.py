"""Worker for the GPU movie test with neighbour-graph columns: one rank, cell typing and neighbor_features on.  Rank 0 writes the
gathered tables to argv[1] and the label maps of its frames to argv[1].labels.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(out_path, rank, world, dist):
    from tissue_image_processing_amd import movie, synthetic
    Z, Y, X, T = 6, 128, 128, 3
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=9)
    stacks = [synthetic.make_stack(Z, Y, X, seed=90 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)]
    opts = dict(atoh_channel=1, threshold=0.03, percentage_above_threshold=3, peak_window_size=3)
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, cell_types=opts, neighbor_features=True)
    tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend, rank, world, dist, "cpu", np.zeros((T, 2)), block_frames=1)
    labels = {"labels_%d" % t: backend.labels[t].download((Y, X), np.int32) for t in backend.labels}
    backend.close()
    if rank == 0:
        out = dict(n=T, columns=np.asarray([name for name, _ in backend.extra_columns]))
        for t in range(T):
            for k in tabs[t]:
                out["%s_%d" % (k, t)] = tabs[t][k]
        np.savez(out_path, **out)
        np.savez(out_path + ".labels.npz", **labels)


if __name__ == "__main__":
    from gloo_launch import gloo_group
    with gloo_group(single=False) as (rank, world, dist):
        run(sys.argv[1], rank, world, dist)
