"""Worker for the 2-process GPU movie test with cell typing: both ranks drive the SAME GPU (device 0), collectives over gloo.
Rank 0 writes the gathered tables and ids to argv[1]; every rank writes the type maps of its own frames to argv[1].rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(out_path, rank, world, dist):
    from tissue_image_processing_amd import movie, synthetic
    Z, Y, X, T = 6, 128, 160, 5
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=8)
    stacks = [synthetic.make_stack(Z, Y, X, seed=80 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)]
    opts = dict(atoh_channel=1, threshold=0.03, percentage_above_threshold=3, peak_window_size=3)
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, inflight=2, cell_types=opts)
    drifts = np.zeros((T, 2))
    drifts[1:] = (-0.5, 0.3)
    tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend, rank, world, dist, "cpu", drifts, block_frames=1)
    np.savez(out_path + ".rank%d.npz" % rank, **{"map_%d" % t: backend.fetch_cell_types(t) for t in backend.type_maps})
    backend.close()
    if rank == 0:
        out = dict(n=T)
        for t in range(T):
            out["ids_%d" % t] = ids[t]
            for k in ("area", "type", "valid", "mean_intensity"):
                out["%s_%d" % (k, t)] = tabs[t][k]
        np.savez(out_path, **out)


if __name__ == "__main__":
    from gloo_launch import gloo_group
    with gloo_group(single=False) as (rank, world, dist):
        run(sys.argv[1], rank, world, dist)
