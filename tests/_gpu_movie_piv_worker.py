"""GPU side of the process_movie(use_piv=True) tests: a GpuFrameBackend that installs given label maps and planes, the
synthetic square movie, and the worker for the 2-process runs (both ranks on GPU 0, collectives over gloo)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def installed_backend_class():
    from tissue_image_processing_amd import movie

    class InstalledBackend(movie.GpuFrameBackend):
        """GpuFrameBackend whose frames are (label map, float64 reference-channel plane) pairs put on the device as they
        are: the driver's device step (piv_lookup) runs on given data; the tables come from the oracle's regionprops."""

        def __init__(self, Y, X):
            super().__init__(2, 4, Y, X, device=0, keep_planes=True)

        def process_frame(self, t, frame):
            import torch
            from oracle import oracle as orc
            from tissue_image_processing_amd import _lib
            labels, plane = frame
            lab = np.ascontiguousarray(labels, np.int32)
            self.labels[t] = _lib.DeviceBuffer(lab.nbytes).upload(lab)
            self.planes[t] = torch.from_numpy(np.ascontiguousarray(plane, np.float64)).to(torch.device("cuda", 0))
            torch.cuda.synchronize()
            rp = orc.regionprops(lab)
            area = rp["area"]
            return dict(area=area, cy=np.where(area > 0, rp["cy"], 0.0), cx=np.where(area > 0, rp["cx"], 0.0))

    return InstalledBackend


def synthetic_movie(Y, X, T, Z=6, seed=7):
    from tissue_image_processing_amd import synthetic
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=seed)
    return [synthetic.make_stack(Z, Y, X, seed=10 * seed + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)]


def run(out_path, mode, rank, world, dist):
    from tissue_image_processing_amd import movie
    Z, T = 6, 4
    Y, X = (256, 256) if mode == "square" else (128, 256)      # non-square: rows < columns, cells right of row index 127
    stacks = synthetic_movie(Y, X, T, Z)
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, keep_planes=True, inflight=2)
    try:
        tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend, rank, world, dist, "cpu", block_frames=1, use_piv=True)
    finally:
        backend.close()
    if rank == 0:
        np.savez(out_path, n=T, **{"ids_%d" % t: ids[t] for t in range(T)}, **{"area_%d" % t: tabs[t]["area"] for t in range(T)})


if __name__ == "__main__":
    from gloo_launch import gloo_group
    try:
        with gloo_group(single=False) as (rank, world, dist):
            run(sys.argv[1], sys.argv[2], rank, world, dist)
    except IndexError as e:      # (the group is gone by now, without a barrier)
        with open("%s.rank%s.err" % (sys.argv[1], os.environ["RANK"]), "w") as f:
            f.write(str(e))
