"""CPU stand-in for movie.process_movie(use_piv=True): a backend whose piv_lookup restates the device step in numpy
(tests/tvl1_restate.tvl1 on the uint16-truncated planes, then upstream's transposed sampling and the label look-up), and
the worker for the gloo runs of tests/test_movie_piv.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _movie_worker import OracleBackend  # noqa: E402


def piv_hits(flow, labels, table):
    """Steps 3 and 4 of the PIV tracker (ti.py:2061-2106) in numpy: rows = round(cx), cols = round(cy) over every row
    (numpy's wrap and IndexError), cx -= flow[0][rows, cols], cy -= flow[1][rows, cols], then the 3x3-max-filtered label
    map at (round(cy), round(cx)); -1 outside the frame and for absent rows."""
    from oracle import oracle as orc
    cx = np.array(table["cx"], dtype=np.float64)
    cy = np.array(table["cy"], dtype=np.float64)
    rows = np.round(cx).astype(np.int64)
    cols = np.round(cy).astype(np.int64)
    cx -= flow[0][rows, cols]
    cy -= flow[1][rows, cols]
    lab = orc.maximum_filter(np.ascontiguousarray(labels, np.int32), (3, 3), mode="constant")
    Y, X = lab.shape
    qy, qx = np.round(cy).astype(np.int64), np.round(cx).astype(np.int64)
    ok = (qy >= 0) & (qy < Y) & (qx >= 0) & (qx < X)
    out = np.full(qy.shape, -1, np.int32)
    out[ok] = lab[qy[ok], qx[ok]]
    return np.where(np.asarray(table["area"]) > 0, out, -1).astype(np.int32)


class PivOracleBackend(OracleBackend):
    """OracleBackend plus the PIV step, in numpy."""

    def piv_lookup(self, t, prev_plane, prev_table):
        import tvl1_restate as R
        prev = np.asarray(prev_plane.numpy() if hasattr(prev_plane, "numpy") else prev_plane)
        flow, _ = R.tvl1(prev.astype(np.uint16), self.planes[t].astype(np.uint16))
        return piv_hits(flow, self.labels[t], prev_table)


def golden_frames(crop=False):
    """The reference's use_piv run (tests/golden/piv_tracking.npz) as (label map, float64 plane) frames.  The planes carry
    a fractional part below 1, which astype(uint16) drops: they truncate to the golden's uint16 images.  crop: the 64 x 128
    top of the first two frames (cells right of the last row index: upstream's IndexError)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "piv_tracking.npz"))
    frac = np.random.default_rng(11).uniform(0.0, 0.999, g["images"].shape)
    planes = g["images"].astype(np.float64) + frac
    labs = g["labels"]
    if crop:
        return [(labs[t, :64, :], planes[t, :64, :]) for t in range(2)]
    return [(labs[t], planes[t]) for t in range(labs.shape[0])]


def main():
    import torch.distributed as dist
    from tissue_image_processing_amd import movie
    out_path, mode = sys.argv[1], sys.argv[2]
    block = int(sys.argv[3]) if len(sys.argv) > 3 and int(sys.argv[3]) > 0 else None
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    frames = golden_frames(crop=(mode == "crop"))
    try:
        tabs, ids = movie.process_movie(len(frames), lambda t: frames[t], PivOracleBackend(), rank, world, dist, "cpu",
                                        block_frames=block, use_piv=True)
    except IndexError as e:
        with open("%s.rank%d.err" % (out_path, rank), "w") as f:
            f.write(str(e))
        dist.destroy_process_group()
        return
    if rank == 0:
        np.savez(out_path, n=len(frames), drifts=np.array([tb["drift"] for tb in tabs]),
                 **{"ids_%d" % t: ids[t] for t in range(len(frames))})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
