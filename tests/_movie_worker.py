"""The CPU stand-ins for GpuFrameBackend (oracle / numpy arithmetic behind the same interface) with their test movies, and
the worker for the gloo tests of movie.process_movie in tests/test_movie_sharding.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TYPE_COLUMNS = (("type", np.uint8), ("valid", np.uint8), ("mean_intensity", np.float64))


def lookup_max3(labels, qy, qx):
    """The oracle's 3x3-max-filtered label map (zeros beyond the border) at (qy, qx) as int32; -1 for a point outside the frame."""
    from oracle import oracle as orc
    mx = orc.maximum_filter(np.ascontiguousarray(labels, np.int32), (3, 3), mode="constant")
    Y, X = mx.shape
    ok = (qy >= 0) & (qy < Y) & (qx >= 0) & (qx < X)
    out = np.full(qy.shape, -1, np.int32)
    out[ok] = mx[qy[ok], qx[ok]]
    return out


class OracleBackend(object):
    """Stands in for GpuFrameBackend on CPU: same interface, oracle arithmetic (test infrastructure)."""

    def __init__(self):
        self.labels = {}
        self.planes = {}

    def process_frame(self, t, labels):
        from oracle import oracle as orc
        if isinstance(labels, tuple):      # (label map, reference-channel plane): the drift-estimating driver
            labels, plane = labels
            self.planes[t] = np.ascontiguousarray(plane, np.float64)
        self.labels[t] = np.ascontiguousarray(labels, np.int32)
        rp = orc.regionprops(labels)
        area = rp["area"]
        return dict(area=area, cy=np.where(area > 0, rp["cy"], 0.0), cx=np.where(area > 0, rp["cx"], 0.0))

    def lookup(self, t, qy, qx):
        return lookup_max3(self.labels[t], qy, qx)

    def plane(self, t):
        import torch
        return torch.from_numpy(self.planes[t])

    def empty_plane(self):
        import torch
        return torch.empty(next(iter(self.planes.values())).shape, dtype=torch.float64)

    def drift(self, t, prev_plane):
        from oracle import oracle as orc
        sh = orc.phase_cross_correlation(prev_plane.numpy(), self.planes[t], upsample_factor=100)
        return float(sh[0]), float(sh[1])


def drifting_movie(n_frames=5, step=(2, -3)):
    """The first golden label frame inside a zero margin, rolled by `step` per frame, with a smooth plane rolled alike:
    every frame has the same cells, so a correct drift estimate makes every frame's ids equal to the first frame's."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "tracking.npz"))
    lab0 = np.pad(g["labels"][0], 24)
    rng = np.random.default_rng(3)
    from oracle import oracle as orc
    plane0 = orc.blur_image(rng.random(lab0.shape), 2.0) * 1000.0
    frames = []
    for t in range(n_frames):
        sh = (t * step[0], t * step[1])
        frames.append((np.roll(lab0, sh, axis=(0, 1)), np.roll(plane0, sh, axis=(0, 1))))
    return frames


# -- use_piv ------------------------------------------------------------------------------------------------------
def piv_hits(flow, labels, table):
    """Steps 3 and 4 of the PIV tracker (ti.py:2061-2106) in numpy: rows = round(cx), cols = round(cy) over every row
    (numpy's wrap and IndexError), cx -= flow[0][rows, cols], cy -= flow[1][rows, cols], then the 3x3-max-filtered label
    map at (round(cy), round(cx)); -1 outside the frame and for absent rows."""
    cx = np.array(table["cx"], dtype=np.float64)
    cy = np.array(table["cy"], dtype=np.float64)
    rows = np.round(cx).astype(np.int64)
    cols = np.round(cy).astype(np.int64)
    cx -= flow[0][rows, cols]
    cy -= flow[1][rows, cols]
    out = lookup_max3(np.asarray(labels, np.int32), np.round(cy).astype(np.int64), np.round(cx).astype(np.int64))
    return np.where(np.asarray(table["area"]) > 0, out, -1).astype(np.int32)


class PivOracleBackend(OracleBackend):
    """OracleBackend plus the PIV step: a numpy restatement of the device step (tests/tvl1_restate.tvl1 on the
    uint16-truncated planes, then upstream's transposed sampling and the label look-up)."""

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


# -- cell types ---------------------------------------------------------------------------------------------------
def numpy_cell_types(labels, marker, threshold=0.1, percentage_above_threshold=90, type_index=0, min_cell_area=0.1,
                     max_cell_area=10):
    """calc_cell_types on a fresh table without the peak test, in plain numpy (np.percentile per label): per row 0..n-1
    the type byte, the validity and the mean intensity."""
    n = int(labels.max())
    area = np.bincount(labels.ravel(), minlength=n + 1)[1:n + 1]
    isum = np.bincount(labels.ravel(), weights=marker.ravel(), minlength=n + 1)[1:n + 1]
    mean = np.mean(area)
    valid = ((area > min_cell_area * mean) & (area < max_cell_area * mean)).astype(np.uint8)
    cut = threshold * np.percentile(marker, 99)
    typ = np.zeros(n, np.uint8)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_intensity = np.where(area > 0, isum / area, np.nan)
    for l in range(1, n + 1):
        if area[l - 1] and np.percentile(marker[labels == l], 100 - percentage_above_threshold) > cut:
            typ[l - 1] = 1 << type_index
    return typ, valid, mean_intensity


class TypingBackend(OracleBackend):
    """Stands in for GpuFrameBackend(cell_types=...) on CPU: frames are (label map, marker plane); with typed=False it
    behaves as a backend without cell typing (no extra columns)."""

    def __init__(self, typed):
        super().__init__()
        self.extra_columns = TYPE_COLUMNS if typed else ()

    def process_frame(self, t, frame):
        out = super().process_frame(t, frame)
        if self.extra_columns:
            out["type"], out["valid"], out["mean_intensity"] = numpy_cell_types(*frame, threshold=0.4)
        return out


def typed_movie(n_frames):
    """The golden tracking frames cycled, with a marker plane per frame: integer values (ties), a few bright cells, one
    label removed from every third frame (absent rows) and a single-pixel label."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "tracking.npz"))
    labs = list(g["labels"])
    rng = np.random.default_rng(11)
    frames = []
    for t in range(n_frames):
        lab = labs[t % len(labs)].copy()
        n = int(lab.max())
        if t % 3 == 0:
            lab[lab == 5] = 0
        lab[0, 0] = n + 1
        bright = rng.random(n + 2) < 0.3
        marker = np.round(rng.normal(10, 3, lab.shape)) + np.where(bright[lab], 40.0, 0.0)
        marker[lab == 0] = 0.0
        frames.append((lab, marker))
    return frames


def save_ids(out_path, ids, **more):
    np.savez(out_path, n=len(ids), **{"ids_%d" % t: v for t, v in enumerate(ids)}, **more)


def main():
    from gloo_launch import gloo_group
    from tissue_image_processing_amd import movie
    out_path, n_rep = sys.argv[1], int(sys.argv[2])
    n_keep = int(sys.argv[3]) if len(sys.argv) > 3 else 0          # > 0: only the first n_keep frames (uneven shards, T < world)
    block = int(sys.argv[4]) if len(sys.argv) > 4 and int(sys.argv[4]) > 0 else None   # frames per rank and round
    with gloo_group() as (rank, world, dist):
        if n_rep == 0:     # the drift-estimating variant (drifts are NOT given), both stitchers
            frames = drifting_movie(n_frames=n_keep or 5)
            tabs, ids = movie.process_movie(len(frames), lambda t: frames[t], OracleBackend(), rank, world, dist, "cpu",
                                            estimate_drift=True, block_frames=block)
            tabs2, ids2 = movie.process_movie(len(frames), lambda t: frames[t], OracleBackend(), rank, world, dist, "cpu",
                                              estimate_drift=True, stitcher="linker", block_frames=block)
            if rank == 0:
                save_ids(out_path, ids, drifts=np.array([tb["drift"] for tb in tabs]),
                         **{"lids_%d" % t: ids2[t] for t in range(len(frames))})
            return
        g = np.load(os.path.join(ROOT, "tests", "golden", "tracking.npz"))
        labs = list(g["labels"])
        frames = (labs + labs[::-1]) * n_rep          # a longer movie out of the golden frames
        if n_keep:
            frames = frames[:n_keep]
        drifts = np.zeros((len(frames), 2))
        drifts[1:] = (0.5, -0.3)
        tabs, ids = movie.process_movie(len(frames), lambda t: frames[t], OracleBackend(), rank, world, dist, "cpu", drifts,
                                        block_frames=block)
        if rank == 0:
            save_ids(out_path, ids)


if __name__ == "__main__":
    main()
