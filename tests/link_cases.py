"""Shared inputs of the linker tests (test_link_cases_host.py, test_gpu_link.py); not a test.  Everything is seeded; the host
linker's ids per case are computed once per process and handed out as copies' sources (do not write into them)."""
import functools

import numpy as np

from tissue_image_processing_amd import linking

# name: (seed, n, size, frames).  A: the general case.  B: everything within reach of everything, so every frame goes through
# many range reductions.  C: the 2048^2 headline density (about 0.25 s per host frame).
MOVIES = {"A": (1, 400, 600.0, 5), "B": (5, 64, 160.0, 6), "C": (2, 4660, 2048.0, 3)}
DRIFT = np.array([0.5, -0.3])


def movie(seed, n, size, frames, drop=0.03):
    """`frames` arrays of embedded features (N_t, 3).  Cells start uniform in [0, size)^2 with areas in [500, 1500]; before every
    later frame max(1, n // 50) fresh cells are appended, the rows are permuted, moved by N(0, 1) px + DRIFT and their areas
    scaled by U(0.98, 1.02); every frame shows each cell with probability 1 - drop (a hidden cell lives on: memory)."""
    rng = np.random.default_rng(seed)
    pts, area = rng.uniform(0, size, (n, 2)), rng.uniform(500, 1500, n)
    out = []
    for t in range(frames):
        if t:
            k = max(1, n // 50)
            pts = np.concatenate([pts, rng.uniform(0, size, (k, 2))])
            area = np.concatenate([area, rng.uniform(500, 1500, k)])
            perm = rng.permutation(pts.shape[0])
            pts = pts[perm] + rng.normal(0, 1.0, pts.shape) + DRIFT
            area = area[perm] * rng.uniform(0.98, 1.02, area.shape)
        seen = rng.random(pts.shape[0]) >= drop
        out.append(linking.embed(pts[seen, 0], pts[seen, 1], area[seen]))
    return out


@functools.lru_cache(maxsize=None)
def frames_of(name):
    return tuple(movie(*MOVIES[name]))


def run(linker, frames):
    """The ids of every frame."""
    return [linker.link(f) for f in frames]


@functools.lru_cache(maxsize=None)
def host_ids(name):
    return tuple(run(linking.FrameLinker(), frames_of(name)))


def shifted(frames, dy, dx):
    return [f + np.array([dy, dx, 0.0]) for f in frames]


@functools.lru_cache(maxsize=None)
def cluster_frames(k, with_a=True):
    """Two frames: movie A's first two (unless with_a is False), and far away from them a cluster of k cells drawn uniformly in
    a 40 x 40 square around (10000, 10000) -- k tracks in the first frame, the same k cells moved like a movie's in the second.
    Every pair of the cluster is within the search range of 100, so it is one subnet of k tracks and k features.  Seed 14: a
    cluster so dense splits only when a cell near a corner of the (y, x, sqrt(area / 2)) box loses its last neighbour; at this
    seed the host linker gets k = 31 there at range 15, at some others never above adaptive_stop = 10."""
    rng = np.random.default_rng(14)
    a = frames_of("A") if with_a else (np.zeros((0, 3)), np.zeros((0, 3)))
    pts = 10000.0 - 20.0 + rng.uniform(0, 40.0, (k, 2))
    area = rng.uniform(500, 1500, k)
    first = linking.embed(pts[:, 0], pts[:, 1], area)
    perm = rng.permutation(k)
    pts = pts[perm] + rng.normal(0, 1.0, pts.shape) + DRIFT
    area = area[perm] * rng.uniform(0.98, 1.02, k)
    second = linking.embed(pts[:, 0], pts[:, 1], area)
    return np.concatenate([a[0], first]), np.concatenate([second, a[1]])


@functools.lru_cache(maxsize=None)
def cluster_host_ids(k):
    return tuple(run(linking.FrameLinker(), cluster_frames(k)))


def oversize_frames():
    """test_linking.py's oversize case: 200 points in 300^2 with equal areas, everything within reach of everything."""
    rng = np.random.default_rng(3)
    pts = rng.uniform(0, 300, (200, 2))
    area = np.full(200, 900.0)
    return linking.embed(pts[:, 0], pts[:, 1], area), linking.embed(pts[:, 0] + 0.5, pts[:, 1], area)


class Recorder(object):
    """Wraps linking._solve_subnet (install with monkeypatch.setattr): records (tracks, features, null range) of every subnet
    solved and, with eps, multiplies every link cost's distance by 1 + eps u, u uniform in [-1, 1], seeded."""

    def __init__(self, eps=0.0):
        self.inner = linking._solve_subnet
        self.eps = eps
        self.rng = np.random.default_rng(9)
        self.solved = []

    def __call__(self, src, dst, es, ed, ev, null_range):
        self.solved.append((len(src), len(dst), float(null_range)))
        if self.eps:
            ev = ev * (1.0 + self.eps * self.rng.uniform(-1, 1, ev.shape))
        return self.inner(src, dst, es, ed, ev, null_range)

    def reductions(self, search_range=100.0, step=0.95):
        """How often the range was multiplied by `step` before the last subnet was solved."""
        return int(round(np.log(min(r for _, _, r in self.solved) / search_range) / np.log(step)))
