"""The sensory-region filter restated in numpy + fractions.Fraction (csrc/tip_hull.hip): exact orientation, exact
convex hull, exact strict-outside test, and the row selection of ti.py:614-620 -- no floating decision anywhere."""
from fractions import Fraction

import numpy as np


class NoHull(ValueError):
    pass


def orient(a, b, p):
    """the sign of (b - a) x (p - a) over the rationals; a, b, p: (x, y) pairs of Fractions"""
    d = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
    return (d > 0) - (d < 0)


def exact_points(x, y):
    return [(Fraction(float(u)), Fraction(float(v))) for u, v in zip(x, y)]


def convex_hull(pts, rows=None):
    """positions (into pts) of the strict hull vertices of pts[rows], counter-clockwise from the lexicographically smallest
    (x, then y); the lowest position stands for coincident points; NoHull for fewer than three vertices"""
    rows = range(len(pts)) if rows is None else [int(r) for r in rows]
    order = sorted(rows, key=lambda i: (pts[i][0], pts[i][1], i))
    uniq = [i for k, i in enumerate(order) if k == 0 or pts[order[k - 1]] != pts[i]]
    if len(uniq) < 3:
        raise NoHull("%d distinct points" % len(uniq))

    def chain(seq):
        out = []
        for i in seq:
            while len(out) >= 2 and orient(pts[out[-2]], pts[out[-1]], pts[i]) <= 0:
                out.pop()
            out.append(i)
        return out

    lower, upper = chain(uniq), chain(uniq[::-1])
    hull = lower[:-1] + upper[:-1]
    if len(hull) < 3:
        raise NoHull("all points on one line")
    return hull


def outside(pts, hull, q):
    """True when q lies strictly outside the counter-clockwise convex polygon pts[hull]"""
    return any(orient(pts[hull[k]], pts[hull[(k + 1) % len(hull)]], q) < 0 for k in range(len(hull)))


def hair_rows(type, valid, empty):
    """ti.py:616: type == 1 and empty_cell == 0 and valid == 1 -- equalities"""
    return np.flatnonzero((np.asarray(type) == 1) & (np.asarray(empty) == 0) & (np.asarray(valid) == 1))


def sensory_region(cx, cy, type=None, valid=None, empty=None):
    """(outside flags uint8[n] over EVERY row, hull row positions); type None: every row is a hull point"""
    cx, cy = np.asarray(cx, np.float64), np.asarray(cy, np.float64)
    pts = exact_points(cx, cy)
    rows = None if type is None else hair_rows(type, valid, np.zeros(cx.size) if empty is None else empty)
    hull = convex_hull(pts, rows)
    return np.array([1 if outside(pts, hull, p) else 0 for p in pts], np.uint8), np.array(hull, np.int32)


def margins(cx, cy, hull):
    """float distance of every row to the hull's boundary (the golden tool's band test; not a decision)"""
    p = np.stack([np.asarray(cx, float), np.asarray(cy, float)], axis=1)
    a = p[np.asarray(hull)]
    b = np.roll(a, -1, axis=0)
    ab = b - a
    t = np.clip(((p[:, None, :] - a[None]) * ab[None]).sum(-1) / (ab * ab).sum(-1)[None], 0.0, 1.0)
    near = a[None] + t[..., None] * ab[None]
    return np.sqrt(((p[:, None, :] - near) ** 2).sum(-1)).min(axis=1)


def remove_cells(labels, type_map, valid, outside_flags):
    """ti.py:2788-2791 on arrays: valid = 0 on the outside rows, 255 on their pixels"""
    valid = np.array(valid, copy=True)
    valid[np.asarray(outside_flags) != 0] = 0
    out = None
    if type_map is not None:
        out = np.array(type_map, copy=True)
        out[np.isin(labels, np.flatnonzero(outside_flags) + 1)] = 255
    return valid, out
