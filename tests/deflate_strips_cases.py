"""The pages the strip-wise zlib encoder (tip_deflate_strips) is tested on, shared by the restatement's CPU tests and the device
tests: CASES maps a name to (pages (n_pages, rows, cols) of uint8 or uint16, rows_per_strip); restated(name, codes) caches
deflate_strips_restate.deflate_strips of a case."""
import numpy as np

import deflate_strips_restate as sr
from deflate_cases import voronoi_pair

_cache = {}


def _maps(ny, nx, dtype, seed=5):
    """one page of a Voronoi pair: the label map as uint16, or the type map (uint8)"""
    labels, types = voronoi_pair(ny, nx, seed)
    return (labels.astype(np.uint16) if np.dtype(dtype) == np.uint16 else types)[None]


def _noise(ny, nx, dtype):
    rng = np.random.default_rng(ny * nx)
    return rng.integers(0, np.iinfo(dtype).max + 1, (1, ny, nx)).astype(dtype)


def _build():
    cases = {}
    for dtype, tag in ((np.uint8, "u8"), (np.uint16, "u16")):
        cases["ragged_40x48_rps7_" + tag] = (_maps(40, 48, dtype), 7)                 # the last strip holds 5 rows
        cases["voronoi_96x128_rps16_" + tag] = (_maps(96, 128, dtype), 16)
        cases["voronoi_96x128_rps96_" + tag] = (_maps(96, 128, dtype), 96)            # one strip per page
        cases["width37_" + tag] = (_maps(30, 37, dtype), 4)                           # uint16: a row of 74 bytes, no aligned dword above
        cases["rows_3000x8_rps1_" + tag] = (_maps(3000, 8, dtype), 1)                 # more strips than the grid has workgroups
        cases["three_pages_" + tag] = (np.concatenate([_maps(40, 48, dtype, seed=s) for s in (5, 6, 7)]), 7)
        cases["noise_40x48_rps7_" + tag] = (_noise(40, 48, dtype), 7)                 # streams longer than their input
        cases["zero_pages_" + tag] = (np.zeros((0, 40, 48), dtype), 7)
    cases["full_8x4096_rps8_u16"] = (_maps(8, 4096, np.uint16), 8)                     # a strip of exactly 65536 bytes
    cases["full_16x4096_rps16_u8"] = (_maps(16, 4096, np.uint8), 16)
    return cases


CASES = _build()
NAMES = sorted(CASES)
RATIO_CASE = dict(shape=(192, 256), rows_per_strip=16)      # the issue's compression condition: both Voronoi planes as uint16


def ratio_pages():
    labels, types = voronoi_pair(*RATIO_CASE["shape"])
    return np.stack([labels.astype(np.uint16), types.astype(np.uint16)])


def restated(name, codes):
    if (name, codes) not in _cache:
        pages, rps = CASES[name]
        _cache[(name, codes)] = sr.deflate_strips(pages, rps, codes)
    return _cache[(name, codes)]
