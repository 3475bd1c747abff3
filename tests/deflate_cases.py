"""The inputs the run-only deflate encoder is tested on, shared by the restatement's CPU tests and the device tests:
CASES is a list of (name, bytes, elem_bytes); restated(name) caches deflate_restate.deflate_runs of a case."""
import numpy as np

import deflate_restate as dr

_cache = {}


def voronoi_pair(ny=96, nx=128, seed=5):
    """(int32 label map with zero lines, uint8 type map) of a Voronoi tessellation at SURVEY's cell density (one cell per 900
    px): a pixel whose right or lower neighbour lies in another cell is a line pixel (label 0); the type map holds 1 on every
    third cell, 0 on the others and 255 on lines, as the device paints it."""
    if ("voronoi", ny, nx, seed) not in _cache:
        rng = np.random.default_rng(seed)
        n = max(2, round(ny * nx / 900.0))
        sy, sx = rng.uniform(0, ny, n), rng.uniform(0, nx, n)
        yy, xx = np.mgrid[0:ny, 0:nx]
        cell = np.argmin((yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2, axis=-1) + 1
        line = np.zeros((ny, nx), bool)
        line[:, :-1] |= cell[:, :-1] != cell[:, 1:]
        line[:-1, :] |= cell[:-1, :] != cell[1:, :]
        labels = np.where(line, 0, cell).astype(np.int32)
        types = np.where(labels == 0, 255, (labels % 3 == 0)).astype(np.uint8)
        _cache[("voronoi", ny, nx, seed)] = (labels, types)
    return _cache[("voronoi", ny, nx, seed)]


def _straddle(nbytes, e):
    """noise with one constant run of 40 elements across the chunk edge at 65536 (or up to the end when the buffer ends there)"""
    rng = np.random.default_rng(nbytes + e)
    a = rng.integers(0, 256, nbytes, dtype=np.uint8)
    lo, hi = dr.CHUNK - 20 * e, min(nbytes, dr.CHUNK + 20 * e)
    a[lo:hi] = np.tile(np.arange(1, e + 1, dtype=np.uint8), (hi - lo) // e)
    return a.tobytes()


def _build():
    rng = np.random.default_rng(11)
    cases = []
    for e in (1, 2, 4):
        cases.append(("empty_e%d" % e, b"", e))
        cases.append(("one_e%d" % e, bytes(range(7, 7 + e)), e))
    for n in list(range(255, 261)) + list(range(511, 518)):
        cases.append(("const_%dB_e1" % n, b"\x05" * n, 1))
    for e in (4, 2):
        for n in list(range(63, 67)) + list(range(127, 131)):
            cases.append(("const_%del_e%d" % (n, e), bytes(range(200, 200 + e)) * n, e))
    for e in (1, 2, 4):
        # alternating elements (no element repeats), pairs of equal elements (runs of one repeat), and uniform noise
        a, b = bytes(range(1, 1 + e)), bytes(range(150, 150 + e))
        cases.append(("alternating_e%d" % e, (a + b) * 300, e))
        cases.append(("pairs_e%d" % e, (a + a + b + b) * 150, e))
        cases.append(("noise_e%d" % e, rng.integers(0, 256, 3000 * e, dtype=np.uint8).tobytes(), e))
    # no byte below 144 and no repeat: nine bits per byte, the bound's worst case, over a whole chunk and a part of one
    cases.append(("worst_e1", (np.arange(dr.CHUNK + 1000) % 2 + 200).astype(np.uint8).tobytes(), 1))
    for n in (65535, 65536, 65537):
        cases.append(("edge_%dB_e1" % n, _straddle(n, 1), 1))
    for n in (65532, 65536, 65540):
        cases.append(("edge_%dB_e4" % n, _straddle(n, 4), 4))
    labels, types = voronoi_pair()
    cases.append(("voronoi_labels", labels.tobytes(), 4))
    cases.append(("voronoi_types", types.tobytes(), 1))
    # three chunks of a label map and a ragged tail: more than one workgroup, chunk sizes scanned and compacted
    big = np.tile(labels, (6, 3)).astype(np.int32)
    cases.append(("voronoi_tiled", big.tobytes()[:3 * dr.CHUNK + 1236], 4))
    cases.append(("voronoi_tiled_u16", big.astype(np.uint16).tobytes(), 2))
    return cases


CASES = _build()
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}


def restated(name):
    if ("stream", name) not in _cache:
        _, data, e = BY_NAME[name]
        _cache[("stream", name)] = dr.deflate_runs(data, e)
    return _cache[("stream", name)]
