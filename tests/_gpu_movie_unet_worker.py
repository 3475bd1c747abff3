"""GPU side of the U-Net-mode movie tests: the synthetic movie, the one predictor factory every run uses, and the worker of the
1- and 2-process runs (both ranks on GPU 0, collectives over gloo).  Every rank writes what it keeps of its own frames (label,
HC and type maps, network modes, watershed flags) to argv[1].rank<r>.npz; rank 0 writes the gathered tables and ids to argv[1]."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

Z, Y, X, T = 6, 128, 160, 5          # the padded network input is 128 x 256 (see test_gpu_movie_unet.py)
MOVIE_SEED, FRACTION = 8, 0.5        # movie seed and calibrated foreground fraction of the non-degeneracy condition
CELL_TYPES = dict(threshold=0.03, percentage_above_threshold=3, peak_window_size=3)
DRIFT = (-6.5, 4.3)                  # the `drifts` row of every frame t >= 1


def movie_stacks(Yf=Y, Xf=X, frames=T, seed=MOVIE_SEED):
    from tissue_image_processing_amd import synthetic
    sites_t, is_hc = synthetic.make_movie_sites(Yf, Xf, frames, seed=seed)
    return [synthetic.make_stack(Z, Yf, Xf, seed=10 * seed + t, sites=sites_t[t], is_hc=is_hc) for t in range(frames)]


def drift_rows(frames=T):
    d = np.zeros((frames, 2))
    d[1:] = DRIFT
    return d


def predictor_factory(stacks, fraction=FRACTION):
    """factory(device) -> a random-init SegmentationPredictor whose head is calibrated on ONE fixed image, the max over z of
    frame 0's stack as (atoh, zo) planes transposed the way segment_unet hands them over: all predictors are identical."""
    Xf, Yf = stacks[0].shape[3], stacks[0].shape[2]
    fixed = np.stack([stacks[0][1].max(0).T, stacks[0][0].max(0).T]).astype(np.float64)      # (2, X, Y)

    def factory(device):
        from tissue_image_processing_amd.prediction_local import SegmentationPredictor
        pred = SegmentationPredictor(None, (2, Xf, Yf), device=device)
        padded, _ = pred.prepare_image(fixed)
        pred.model.calibrate_head(padded, fraction)
        return pred

    return factory


def run(out_path, rank, world, dist):
    from tissue_image_processing_amd import movie
    stacks = movie_stacks()
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, segmentation="unet", predictor_factory=predictor_factory(stacks),
                                    inflight=2, keep_hc=True, cell_types=CELL_TYPES)
    try:
        tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend, rank, world, dist, "cpu", drift_rows(), block_frames=1)
        own = {}
        for t in backend.labels:
            own["labels_%d" % t] = backend.labels[t].download((Y, X), np.int32)
            own["hc_%d" % t] = backend.fetch_hc(t)
            own["types_%d" % t] = backend.fetch_cell_types(t)
            own["mode_%d" % t] = np.array(str(backend.unet_modes[t]))
            own["flags_%d" % t] = np.int64(backend.ws_flags[t])
        np.savez(out_path + ".rank%d.npz" % rank, **own)
    finally:
        backend.close()
    if rank == 0:
        out = dict(n=T)
        for t in range(T):
            out["ids_%d" % t] = ids[t]
            for k in ("area", "cy", "cx", "type", "valid", "mean_intensity", "drift"):
                out["%s_%d" % (k, t)] = tabs[t][k]
        np.savez(out_path, **out)


if __name__ == "__main__":
    from gloo_launch import gloo_group
    with gloo_group(single=False) as (rank, world, dist):
        run(sys.argv[1], rank, world, dist)
