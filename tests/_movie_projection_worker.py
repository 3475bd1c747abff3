"""Worker for the gloo tests of movie.export_projection (tests/test_export_projection_host.py; CPU): every rank's backend is a stub
that holds its own frames' float64 projections and int64 z-maps on the host and makes its strips with numpy and the host's zlib."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gloo_launch import gloo_group  # noqa: E402

C, Y, X, ROWS_PER_STRIP = 2, 22, 30, 5      # the last strip holds 2 rows


def projection_movie(n_frames):
    """-> per frame (float64 projection (C, Y, X), int64 z-map (Y, X)).  Frame 1 holds the movie's maximum; the others stay below
    0.8 of it, so a frame scaled by its own maximum would differ from the movie's scaling.  The z-maps reach beyond 65535."""
    frames = []
    for t in range(n_frames):
        rng = np.random.default_rng(40 + t)
        proj = rng.random((C, Y, X)) * (4000.0 if t == 1 else 3000.0 - 200.0 * t)
        proj[0, 3] = 0.0
        if t == 1:
            proj[1, 7, 11] = 4096.5
        zmap = rng.integers(0, 30, (Y, X)).astype(np.int64)
        zmap[t % Y, 2] = 65536 + 7 * t
        frames.append((proj, zmap))
    return frames


def expected_movie(frames):
    """tiff_normalise of the WHOLE stacked movie, and the z-map file's array"""
    from tissue_image_processing_amd.tiff import tiff_normalise
    movie = tiff_normalise(np.stack([f[0] for f in frames]), "uint16")
    zmaps = np.stack([f[1] for f in frames]).astype("uint16").reshape(len(frames), 1, 1, Y, X)
    return movie, zmaps


def difference(page):
    """TIFF predictor 2 of a uint16 page: x differences modulo 2^16, the first column as it is"""
    return np.concatenate([page[:, :1], np.diff(page, axis=1)], axis=1).astype(np.uint16)


class HostProjectionBackend(object):
    """What export_projection asks of a backend: C, Y, X, the frames it holds (projections, zmaps), projection_max,
    projection_page_strips and zmap_u16."""

    def __init__(self, frames, owned):
        self.C, self.Y, self.X = C, Y, X
        self.projections = {t: frames[t][0] for t in owned}
        self.zmaps = {t: frames[t][1] for t in owned}
        self.calls = []

    def projection_max(self, t):
        return float(self.projections[t].max())

    def projection_page_strips(self, t, scale_max, rowsperstrip, codes, predictor):
        self.calls.append((t, rowsperstrip, codes, predictor))
        pages = np.round((self.projections[t] / scale_max) * 65535).astype(np.uint16)
        pages = [difference(p) if predictor == 2 else p for p in pages]
        return [[zlib.compress(p[r:r + rowsperstrip].tobytes(), 6) for r in range(0, self.Y, rowsperstrip)] for p in pages]

    def zmap_u16(self, t):
        return self.zmaps[t].astype(np.uint16)


def main():
    from tissue_image_processing_amd import movie
    from tissue_image_processing_amd.pipeline import frames_for_rank
    out_path, n_frames, predictor, missing = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    frames = projection_movie(n_frames)
    with gloo_group() as (rank, world, dist):
        owned = [t for t in frames_for_rank(n_frames, rank, world) if t != missing]
        backend = HostProjectionBackend(frames, owned)
        try:
            got = movie.export_projection(out_path, n_frames, backend, rank, world, dist, "cpu", rowsperstrip=ROWS_PER_STRIP,
                                          predictor=predictor)
            zmap_path = os.path.join(os.path.dirname(out_path), "zmap_%s.npy" % os.path.basename(out_path)[:-4])
            assert got == ((out_path, zmap_path) if rank == 0 else None)
            assert sorted(c[0] for c in backend.calls) == sorted(owned)
            assert all(c[1:] == (ROWS_PER_STRIP, "dynamic", predictor) for c in backend.calls)
        except ValueError as e:
            assert not backend.calls                  # nothing was encoded
            with open("%s.rank%d.err" % (out_path, rank), "w") as fh:
                fh.write(str(e))


if __name__ == "__main__":
    main()
