"""Worker for the GPU movie test with the order columns: one rank, order_features on, validity by the area rule.  Rank 0 writes the
gathered tables to argv[1]."""
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
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, order_features=True)
    tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend, rank, world, dist, "cpu", np.zeros((T, 2)), block_frames=1)
    backend.close()
    if rank == 0:
        out = dict(n=T, columns=np.asarray([name for name, _ in backend.extra_columns]))
        for t in range(T):
            for k in tabs[t]:
                out["%s_%d" % (k, t)] = tabs[t][k]
        np.savez(out_path, **out)


if __name__ == "__main__":
    from gloo_launch import gloo_group
    with gloo_group(single=False) as (rank, world, dist):
        run(sys.argv[1], rank, world, dist)
