"""numpy restatement of the order kernels (csrc/tip_order.hip): the specification the GPU tests compare against, checked itself
against the reference's goldens (tests/golden/order_features.npz) and scipy by tests/test_order_features_host.py.

Delaunay rule, the same operations in the same order as the kernel's `cut` (every numpy operation below rounds once, to float64,
and numpy never contracts a multiply and an add): relative to p_i, a = p_j - p_i, b = p_k - p_i,
    s = a.x b.y - a.y b.x,   num = (b.x b.x + b.y b.y) - (a.x b.x + a.y b.y),   t = num / (2 s)
    hi = min t over s > 0 (+inf without one), lo = max t over s < 0 (-inf without one)
(i, j) is an edge iff lo < hi and no k has s == 0 and num < 0.  Here every k is visited (k = i and k = j give s = 0, num = 0
exactly), O(n^3): the kernel visits the ring it certified, which gives the same edges."""
import numpy as np


def delaunay_neighbors(py, px):
    """list of ascending int arrays: the 0-based positions of each point's neighbours"""
    py, px = np.asarray(py, np.float64).reshape(-1), np.asarray(px, np.float64).reshape(-1)
    n = py.size
    rows = []
    for i in range(n):
        bx, by = px - px[i], py - py[i]                      # also the a of every j
        ax, ay = bx[:, None], by[:, None]
        with np.errstate(all="ignore"):
            s = ax * by[None, :] - ay * bx[None, :]
            num = (bx * bx + by * by)[None, :] - (ax * bx[None, :] + ay * by[None, :])
            t = num / (2.0 * s)
        hi = np.fmin.reduce(np.where(s > 0, t, np.inf), axis=1)
        lo = np.fmax.reduce(np.where(s < 0, t, -np.inf), axis=1)
        blocked = ((s == 0) & (num < 0)).any(axis=1)
        edge = (lo < hi) & ~blocked
        edge[i] = False
        rows.append(np.flatnonzero(edge).astype(np.int32))
    return rows


def csr(rows, add=0):
    off = np.zeros(len(rows) + 1, np.int64)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows])
    mem = np.asarray([int(v) + add for r in rows for v in r], dtype=np.int32)
    return off, mem


def edges_of(rows):
    """the set of undirected edges (lo, hi) of a list of rows; asserts the rows are symmetric"""
    directed = {(q, int(v)) for q, r in enumerate(rows) for v in r}
    assert all((b, a) in directed for a, b in directed)
    return {(a, b) for a, b in directed if a < b}


def voronoi_edges(py, px):
    from scipy.spatial import Voronoi
    ridge = Voronoi(np.stack([np.asarray(px, np.float64), np.asarray(py, np.float64)], axis=1)).ridge_points
    return {(int(min(a, b)), int(max(a, b))) for a, b in ridge}


def psin(cy, cx, member_offsets, members, query=None, order=6):
    """hypot(sum cos(n theta), sum sin(n theta)) / count per row, the members (1-based labels) summed in the order given"""
    cy, cx = np.asarray(cy, np.float64), np.asarray(cx, np.float64)
    m = len(member_offsets) - 1
    out = np.zeros(m)
    for q in range(m):
        r = q if query is None else int(query[q])
        k = np.asarray(members[member_offsets[q]:member_offsets[q + 1]], dtype=np.int64) - 1
        if k.size == 0:
            continue
        th = float(order) * np.arctan2(cy[k] - cy[r], cx[k] - cx[r])
        sc = ss = 0.0
        for c, s in zip(np.cos(th), np.sin(th)):
            sc, ss = sc + c, ss + s
        out[q] = np.hypot(sc, ss) / k.size
    return out


def graph_neighbor_state(offsets, adj, member, state, query=None):
    """(nb_sum, nb_cnt): per query row the float64 sum, in row order, of state over the neighbours flagged in member"""
    n = len(offsets) - 1
    query = range(n) if query is None else query
    nb_sum, nb_cnt = np.zeros(len(query)), np.zeros(len(query), np.int64)
    for q, r in enumerate(query):
        acc = np.float64(0.0)
        for label in adj[offsets[r]:offsets[r + 1]]:
            if member[label - 1]:
                acc = acc + np.float64(state[label - 1])
                nb_cnt[q] += 1
        nb_sum[q] = acc
    return nb_sum, nb_cnt


def correlation(state, nb_sum, nb_cnt, method):
    """calculate_neighbors_correlation_function's value from the two columns (ti.py:811-840)"""
    state = np.asarray(state, np.float64)
    with np.errstate(all="ignore"):
        avg, var = np.average(state), np.var(state)
        if method == "neighbors":
            return np.sum((state - avg) * (nb_sum - nb_cnt * avg)) / (int(nb_cnt.sum()) * var)
        ns = np.zeros(state.size)
        has = nb_cnt > 0
        ns[has] = nb_sum[has] / nb_cnt[has]
        return np.sum((state - avg) * (ns - np.average(ns))) / (state.size * np.sqrt(var) * np.std(ns))
