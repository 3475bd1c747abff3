"""The CPU stand-in for GpuFrameBackend.local_drift_lookup (oracle phase correlation per window, the mean and look-up rule in
numpy) and the worker for the gloo runs of tests/test_movie_local_drifts.py: movie.process_movie(local_drifts=...)."""
import sys

import numpy as np

from _movie_worker import OracleBackend, drifting_movie, save_ids
from gloo_launch import gloo_group

MULTI = dict(window_size=48, step_size=16)       # 144 x 168: 6 x 8 = 48 windows, extents 48 x 48 and 48 x 56
SINGLE = dict(window_size=143, step_size=32)     # one window, the whole 144 x 168 frame


def windows_of(shape, step_size, window_size):
    """Upstream's window loop (ti.py:2152-2163), restated: (r0, r1, c0, c1) in loop order."""
    H, W = shape
    out = []
    for r0 in range(0, H - window_size, step_size):
        r1 = H if r0 + step_size + window_size > H else r0 + window_size
        for c0 in range(0, W - window_size, step_size):
            c1 = W if c0 + step_size + window_size > W else c0 + window_size
            out.append((r0, r1, c0, c1))
    return out


def local_hits(prev_plane, cur_plane, labels, table, step_size, window_size):
    """The local-drift step in numpy: per window the oracle's refined shift (upsample 100) between the two planes; per row of
    `table` the mean (d_row, d_col) of the windows that contain (round(cy), round(cx)) -- sums in window loop order, then one
    division by the count -- and the 3x3-max-filtered label map at (round(cy - d_row), round(cx - d_col)).  Returns (int32
    hits, -1 where no window contains the point or the moved point leaves the frame; the window shifts)."""
    from oracle import oracle as orc
    from _movie_worker import lookup_max3
    cy, cx = np.asarray(table["cy"], np.float64), np.asarray(table["cx"], np.float64)
    rows, cols = np.round(cy).astype(np.int64), np.round(cx).astype(np.int64)
    s_row, s_col, cnt = np.zeros(cy.shape), np.zeros(cy.shape), np.zeros(cy.shape)
    shifts = []
    for r0, r1, c0, c1 in windows_of(prev_plane.shape, step_size, window_size):
        sh = orc.phase_cross_correlation(prev_plane[r0:r1, c0:c1], cur_plane[r0:r1, c0:c1], upsample_factor=100)
        shifts.append((float(sh[0]), float(sh[1])))
        inside = (rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1)
        s_row[inside] += sh[0]
        s_col[inside] += sh[1]
        cnt[inside] += 1
    ok = cnt > 0
    safe = np.where(ok, cnt, 1.0)
    qy = np.where(ok, np.round(cy - s_row / safe), -1).astype(np.int64)
    qx = np.where(ok, np.round(cx - s_col / safe), -1).astype(np.int64)
    return np.where(ok, lookup_max3(labels, qy, qx), -1).astype(np.int32), shifts


class LocalOracleBackend(OracleBackend):
    """OracleBackend plus the local-drift step; like GpuFrameBackend it knows its frame extents before the first frame."""

    def __init__(self, Y, X):
        super().__init__()
        self.Y, self.X = Y, X
        self.local_drifts = {}

    def local_drift_lookup(self, t, prev_plane, prev_table, step_size=100, window_size=700):
        prev = np.asarray(prev_plane.numpy() if hasattr(prev_plane, "numpy") else prev_plane)
        hits, self.local_drifts[t] = local_hits(prev, self.planes[t], self.labels[t], prev_table, step_size, window_size)
        return hits


def main():
    from tissue_image_processing_amd import movie
    out_path, mode = sys.argv[1], sys.argv[2]
    block = int(sys.argv[3]) if len(sys.argv) > 3 and int(sys.argv[3]) > 0 else None
    frames = drifting_movie(5)
    with gloo_group() as (rank, world, dist):
        backend = LocalOracleBackend(*frames[0][0].shape)
        tabs, ids = movie.process_movie(len(frames), lambda t: frames[t], backend, rank, world, dist, "cpu", block_frames=block,
                                        local_drifts={"multi": MULTI, "single": SINGLE}[mode])
        if rank == 0:
            save_ids(out_path, ids, drifts=np.array([tb["drift"] for tb in tabs]))


if __name__ == "__main__":
    main()
