"""numpy restatement of the event kernels (csrc/tip_events.hip): the specification the GPU tests compare against, checked itself
against the reference's find_events_iterator on the golden movies and their mutated copies (tests/test_events_host.py).  The three
functions take the arrays the C-ABI entries take and return what they write."""
import numpy as np

EVENT_OUTPUTS = (("delam", np.uint8), ("diff", np.uint8), ("division", np.uint8), ("n_match", np.int32), ("mother_row", np.int32))


def border_rows(labels, n=None):
    """tip_border_rows_i32: flags[r] = 1 when label r + 1 occurs in the first or last row or column."""
    labels = np.asarray(labels)
    if n is None:
        n = int(labels.max()) if labels.size else 0
    border = np.concatenate([labels[0, :], labels[-1, :], labels[:, 0], labels[:, -1]])
    flags = np.zeros(n, np.uint8)
    flags[border[(border >= 1) & (border <= n)] - 1] = 1
    return flags


def lookup_exact(labels, qy, qx):
    """tip_lookup_i32_dev: labels[qy, qx], -1 outside the frame."""
    labels = np.asarray(labels)
    qy, qx = np.asarray(qy, np.int64).reshape(-1), np.asarray(qx, np.int64).reshape(-1)
    ok = (qy >= 0) & (qy < labels.shape[0]) & (qx >= 0) & (qx < labels.shape[1])
    out = np.full(qy.size, -1, np.int32)
    out[ok] = labels[qy[ok], qx[ok]]
    return out


def _row(frame, r):
    return frame["adj"][frame["offsets"][r]:frame["offsets"][r + 1]]


def _passes(frame, n):
    """the row test: the neighbour LABEL n, read as a row index, is a selected row"""
    return 0 <= n < len(frame["id"]) and bool(frame["sel"][n])


def event_flags(prev, cur, first_edge_ids):
    """tip_event_flags_i32.  prev: dict(id, sel, pos, offsets, adj); cur: the same plus edge and under."""
    n_prev, n_cur = len(prev["id"]), len(cur["id"])
    P = set(int(i) for i, s in zip(prev["id"], prev["sel"]) if s)
    C = set(int(i) for i, s in zip(cur["id"], cur["sel"]) if s)
    F = set(int(i) for i in first_edge_ids)
    E = set(int(i) for i, e in zip(cur["id"], cur["edge"]) if e)
    cur_positive = set(int(i) for i, s, p in zip(cur["id"], cur["sel"], cur["pos"]) if s and p)
    out = {"delam": np.zeros(n_prev, np.uint8), "diff": np.zeros(n_prev, np.uint8), "division": np.zeros(n_cur, np.uint8),
           "n_match": np.zeros(n_cur, np.int32), "mother_row": np.full(n_cur, -1, np.int32)}

    def stays(r):
        for n in _row(prev, r):
            if not _passes(prev, n):
                return False
            nid = int(prev["id"][n])
            if nid not in C or nid in F:
                return False
        return True

    for r in range(n_prev):
        if not prev["sel"][r]:
            continue
        cid = int(prev["id"][r])
        if cid not in C and cid not in F and stays(r):
            out["delam"][r] = 1
        if cid in C and cid in cur_positive and not prev["pos"][r] and stays(r):
            out["diff"][r] = 1
    for r in range(n_cur):
        cid = int(cur["id"][r])
        if not cur["sel"][r] or cid in P or cid in E or cur["under"][r] == -1:
            continue
        matches, ok = [], True
        for n in _row(cur, r):
            if not _passes(cur, n):
                ok = False
                break
            nid = int(cur["id"][n])
            if nid in P and nid in C and nid not in E and cur["under"][n] != -1 and cur["under"][n] == cur["under"][r]:
                matches.append(int(n))
        if ok and matches:
            out["division"][r], out["n_match"][r], out["mother_row"][r] = 1, len(matches), max(matches)
    return out
