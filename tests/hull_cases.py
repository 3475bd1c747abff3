"""Point sets of the sensory-region tests (CPU and GPU): each case is the columns cx, cy and the selection bytes type, valid, empty
(type None: every row spans the hull).  exact(name) is the restatement's answer (tests/hull_restate.py, rational arithmetic),
computed once per process."""
import functools
import os

import numpy as np

import hull_restate as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CASES = ("A", "B", "D", "E")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "sensory_region.npz"), allow_pickle=False)


def golden_case(tag):
    g = golden()
    return dict(cx=g["cx_" + tag], cy=g["cy_" + tag], type=g["type_" + tag], valid=g["valid_" + tag], empty=g["empty_cell_" + tag])


def _all(cx, cy):
    return dict(cx=np.asarray(cx, np.float64), cy=np.asarray(cy, np.float64), type=None, valid=None, empty=None)


def _with_queries(hx, hy, qx, qy):
    """hull points (selected) followed by query rows (type 0: tested, but spanning nothing)"""
    n, m = len(hx), len(qx)
    sel = np.r_[np.ones(n, np.uint8), np.zeros(m, np.uint8)]
    return dict(cx=np.r_[np.asarray(hx, np.float64), np.asarray(qx, np.float64)], cy=np.r_[np.asarray(hy, np.float64), np.asarray(qy, np.float64)],
                type=sel, valid=np.ones(n + m, np.uint8), empty=np.zeros(n + m, np.uint8))


def circle200():
    """200 integer-rounded points of a circle of radius 1000: nearly every point is a vertex, with many near-collinear triples"""
    a = 2 * np.pi * np.arange(200) / 200
    return _all(np.round(1000 * np.cos(a)) + 1500, np.round(1000 * np.sin(a)) + 1500)


def duplicates():
    """60 points on a coarse grid, every one three times (in shuffled order): the lowest position stands for its twins"""
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, 12, 60).astype(float), rng.integers(0, 12, 60).astype(float)
    order = rng.permutation(180)
    return _all(np.tile(x, 3)[order], np.tile(y, 3)[order])


POLY = (np.array([0.0, 40.0, 70.0, 64.0, 30.0, -10.0, -16.0]), np.array([0.0, -8.0, 20.0, 60.0, 80.0, 50.0, 10.0]))   # counter-clockwise, strictly convex, plus an interior point below


def _poly():
    return np.r_[POLY[0], 30.0], np.r_[POLY[1], 30.0]


def query_vertices():
    hx, hy = _poly()
    return _with_queries(hx, hy, POLY[0], POLY[1])


def _edge_midpoints():
    x, y = POLY
    return (x + np.roll(x, -1)) / 2, (y + np.roll(y, -1)) / 2        # halves of small even integers: exact, and exactly on the edge


def query_edges():
    hx, hy = _poly()
    mx, my = _edge_midpoints()
    return _with_queries(hx, hy, mx, my)


def query_nextafter():
    """every edge midpoint moved by one ulp in x and in y, to either side: the Fraction truth decides which side each lies on"""
    hx, hy = _poly()
    mx, my = _edge_midpoints()
    qx = np.r_[np.nextafter(mx, np.inf), np.nextafter(mx, -np.inf), mx, mx]
    qy = np.r_[my, my, np.nextafter(my, np.inf), np.nextafter(my, -np.inf)]
    return _with_queries(hx, hy, qx, qy)


def random70000():
    """more than one workgroup, more than 65 536 points, nearly all dropped by the octagon"""
    rng = np.random.default_rng(70)
    return _all(rng.normal(0, 300, 70000), rng.normal(0, 200, 70000))


def circle5000():
    """5 000 integer-rounded points of a circle of radius 100 000: all survive the octagon, so the sort pads to 8192 entries -- four
    LDS chunks and the steps between chunks --, the tangent kernel runs 20 workgroups over 20 tiles and the emit loop 20 trips"""
    a = 2 * np.pi * np.arange(5000) / 5000
    return _all(np.round(100000 * np.cos(a)) + 150000, np.round(100000 * np.sin(a)) + 150000)


def circle70000():
    """70 000 distinct points of a circle of radius 10^7: more survivors than the hull entries take (65 536)"""
    a = 2 * np.pi * np.arange(70000) / 70000
    return _all(np.round(1e7 * np.cos(a)), np.round(1e7 * np.sin(a)))


BIG = dict(random70000=random70000, circle5000=circle5000)        # GPU against the host entry only: too large for rational arithmetic
CASES = dict(circle200=circle200, duplicates=duplicates, query_vertices=query_vertices, query_edges=query_edges,
             query_nextafter=query_nextafter)
CASES.update({"golden_" + tag: functools.partial(golden_case, tag) for tag in GOLDEN_CASES})
DEGENERATE = dict(one=_all([3.0], [4.0]), two=_all([3.0, 5.0], [4.0, 4.0]), twins=_all([3.0, 3.0, 3.0, 5.0], [4.0, 4.0, 4.0, 1.0]),
                  collinear5=_all([0.0, 1.0, 2.0, 3.0, 4.0], [0.5, 1.0, 1.5, 2.0, 2.5]))


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or BIG[name])()


@functools.lru_cache(maxsize=None)
def exact(name):
    c = case(name)
    return hr.sensory_region(c["cx"], c["cy"], c["type"], c["valid"], c["empty"])


@functools.lru_cache(maxsize=None)
def host(name):
    """tip_sensory_region_host on the case (no device): what the GPU tests compare with"""
    from tissue_image_processing_amd import _segmentation as seg
    c = case(name)
    return seg.sensory_region_host(c["cx"], c["cy"], c["type"], c["valid"], c["empty"])
