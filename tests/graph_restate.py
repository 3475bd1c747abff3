"""numpy restatement of the neighbour-graph kernels (csrc/tip_graph.hip): the specification the GPU tests compare against, checked
itself against the reference's goldens (tests/golden/graph_features.npz) by tests/test_graph_features_host.py.

The graph is a CSR adjacency over table rows: offsets int32[n + 1], adj int32[...] of 1-based labels, ascending within a row."""
import numpy as np

ALL, VALID, INVALID, TYPE = 0, 1, 2, 3


def neighbor_pairs(labels):
    """unique (hi, lo) rows: a pixel labelled lo > 0 whose zero-padded 5x5 maximum is hi != lo (ti.py:1822-1835), sorted"""
    lab = np.asarray(labels, dtype=np.int64)
    Y, X = lab.shape
    pad = np.zeros((Y + 4, X + 4), np.int64)
    pad[2:-2, 2:-2] = lab
    mx = np.zeros_like(lab)
    for dy in range(5):
        for dx in range(5):
            mx = np.maximum(mx, pad[dy:dy + Y, dx:dx + X])
    keep = (lab > 0) & (mx != lab)
    pairs = np.unique(np.stack([mx[keep], lab[keep]], axis=1), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
    return pairs.astype(np.int32)


def contact_triples(labels):
    """(pairs (hi, lo) int32, counts int64): per pair hi > lo >= 1 the pixels whose cross-footprint maximum is hi and whose
    cross-footprint minimum, zeros replaced by max + 1 and the frame's outside 0, is lo (ti.py:1080-1085, 1871)"""
    lab = np.asarray(labels, dtype=np.int64)
    Y, X = lab.shape
    big = int(lab.max()) + 1 if lab.size else 1
    hi_pad = np.zeros((Y + 2, X + 2), np.int64)
    hi_pad[1:-1, 1:-1] = lab
    lo_pad = np.zeros((Y + 2, X + 2), np.int64)
    lo_pad[1:-1, 1:-1] = np.where(lab == 0, big, lab)
    shifts = ((0, 1), (2, 1), (1, 0), (1, 2))
    mx = np.max([hi_pad[dy:dy + Y, dx:dx + X] for dy, dx in shifts], axis=0)
    mn = np.min([lo_pad[dy:dy + Y, dx:dx + X] for dy, dx in shifts], axis=0)
    keep = (mx > mn) & (mn >= 1)
    if not keep.any():
        return np.zeros((0, 2), np.int32), np.zeros(0, np.int64)
    pairs, counts = np.unique(np.stack([mx[keep], mn[keep]], axis=1), axis=0, return_counts=True)
    return pairs.astype(np.int32), counts.astype(np.int64)


def csr_from_sets(neighbors):
    """the table's `neighbors` column (one set of labels per row) as CSR, rows ascending"""
    rows = [sorted(int(v) for v in s) for s in neighbors]
    offsets = np.zeros(len(rows) + 1, np.int32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    adj = np.asarray([v for r in rows for v in r], dtype=np.int32)
    return offsets, adj


def sets_from_csr(offsets, adj):
    return [set(int(v) for v in adj[offsets[r]:offsets[r + 1]]) for r in range(len(offsets) - 1)]


def neighbor_csr(pairs, n, working=None):
    """find_neighbors(only_for_labels=...) on a fresh table: pair (hi, lo) gives both directions when working[hi - 1] (or no working)"""
    rows = [set() for _ in range(n)]
    for hi, lo in np.asarray(pairs).reshape(-1, 2):
        hi, lo = int(hi), int(lo)
        if not (1 <= hi <= n and 1 <= lo <= n) or hi == lo:
            continue
        if working is None or working[hi - 1]:
            rows[hi - 1].add(lo)
            rows[lo - 1].add(hi)
    return csr_from_sets(rows)


def selected(type_byte, bit, positive):
    """is_positive_for_type on one byte (bit set and not 255), or its negation; bit None / < 0: everything"""
    if bit is None or bit < 0:
        return True
    pos = bool((int(type_byte) >> bit) & 1) and int(type_byte) != 255
    return pos if positive else not pos


def _row(offsets, adj, r):
    return [int(v) for v in adj[offsets[r]:offsets[r + 1]]]


def graph_counts(offsets, adj, valid, empty, type, query, mode, bit=-1, positive=True):
    out = np.zeros(len(query), np.int64)
    for q, r in enumerate(query):
        nb = _row(offsets, adj, r)
        if mode == ALL:
            out[q] = len(nb)
            continue
        for k in nb:
            if empty[k - 1] != 0:
                continue
            if mode == INVALID:
                out[q] += valid[k - 1] == 0
            elif mode == VALID:
                out[q] += valid[k - 1] == 1
            else:
                out[q] += valid[k - 1] == 1 and selected(type[k - 1], bit, positive)
    return out


def graph_second(offsets, adj, valid, type, query, bit=-1, positive=True):
    """find_second_order_neighbors: one set per query row"""
    out = []
    for r in query:
        found = set()
        for j in _row(offsets, adj, r):
            if valid[j - 1] != 1:
                continue
            for k in _row(offsets, adj, j - 1):
                if k != r + 1 and valid[k - 1] == 1 and selected(type[k - 1], bit, positive):
                    found.add(k)
        out.append(found)
    return out


def contact_sums(pairs, counts, offsets, adj, valid, type, query, mode, bit=-1, positive=True):
    """(sums int64[m], labels: list of arrays, values: list of arrays): per query row the selected neighbours ascending by label
    and the pixel counts of their contacts (0 without a triple)"""
    weight = {(int(h), int(l)): int(c) for (h, l), c in zip(np.asarray(pairs).reshape(-1, 2), counts)}
    sums = np.zeros(len(query), np.int64)
    labels, values = [], []
    for q, r in enumerate(query):
        lab, val = [], []
        for k in _row(offsets, adj, r):
            if mode == VALID and valid[k - 1] != 1:
                continue
            if mode == TYPE and not selected(type[k - 1], bit, positive):
                continue
            lab.append(k)
            val.append(weight.get((max(k, r + 1), min(k, r + 1)), 0))
        sums[q] = sum(val)
        labels.append(np.asarray(lab, dtype=np.int32))
        values.append(np.asarray(val, dtype=np.int64))
    return sums, labels, values
