"""Event detection inside the sharded movie driver (movie.find_events): Tissue.find_events_iterator (ti.py:636-789) restated over
ROWS, so that one device pass per frame pair replaces the reference's pandas query per candidate cell and no label map leaves its
GPU.  DESIGN.md 5.11 has the rules and who computes what.

A frame's rows, as the kernels take them (csrc/tip_events.hip, _segmentation.event_flags): id (the track label per row), sel (valid
== 1 and empty_cell == 0), pos (positive for the differentiation type), the neighbour sets as a CSR, edge (the row's cell touches
the border of its own map) and under (the PREVIOUS map's label under the row's drift-shifted centroid).  This module holds what is
neither kernel nor backend: the CSR of the table's sets, the shifted positions, the choice of a division's mother where several
neighbours match, the field tuples of the three exchanges and rank 0's assembly of the events table through Tissue.add_event."""
import pickle

import numpy as np

from ._collectives import broadcast_varlen, gather_varlen, pack_records, unpack_records

BACKEND_METHODS = ("event_rows", "border_rows", "lookup_exact", "classify_pair")
# the three exchanges, as _collectives' records keyed by frame
MOVIE_FIELDS = (("drift", np.float64), ("id", np.int64), ("cy", np.float64), ("cx", np.float64))      # rank 0's hand-out
ROW_FIELDS = (("sel", np.uint8), ("pos", np.uint8), ("edge", np.uint8), ("offsets", np.int32), ("adj", np.int32),
              ("under_next", np.int32))      # an owner's frames; under_next: the frame's map under the NEXT frame's rows
FOUND_FIELDS = (("delam", np.int64), ("diff", np.int64), ("division", np.int64), ("mother", np.int64))      # an owner's pairs
_FAILED = -1      # key of the one record, its fields empty, that a rank sends when its owner step raised


def sets_to_csr(sets):
    """(offsets int32[n + 1], adj int32[...]) of a table's `neighbors` column: each row's labels ascending, tip_neighbor_csr_i32's
    layout -- built from the sets themselves, so it represents exactly what the archive's table will hold."""
    offsets = np.zeros(len(sets) + 1, np.int32)
    offsets[1:] = np.cumsum([len(s) for s in sets])
    adj = np.array([v for s in sets for v in sorted(s)], np.int32).reshape(-1)
    return offsets, adj


def as_archived(sets):
    """The sets in the iteration order they have once the frame's table went through the archive: a set's order depends on how it
    was built, and the table's pickle rebuilds each from its elements in their current order.  Upstream's division test keeps the
    LAST matching neighbour of list(set), so the mother is picked from what a reader of the archive will iterate."""
    return [pickle.loads(pickle.dumps(s, protocol=pickle.HIGHEST_PROTOCOL)) for s in sets]


def positive_rows(type_bytes, type_index=0):
    from .tissue_info import is_positive_for_type
    return np.asarray(is_positive_for_type(np.asarray(type_bytes, np.uint8), type_index), bool).astype(np.uint8)


def shifted_positions(cy, cx, drift):
    """(qy, qx) int64 where the reference reads the previous map for a row of the frame whose drift row is `drift`:
    int(np.round(cy)) + int(drift[0]), int(np.round(cx)) + int(drift[1]) -- the drift truncated BEFORE it is added (ti.py:745-752).
    A row without a finite centroid gets (-1, -1): outside every frame."""
    cy, cx = np.asarray(cy, np.float64), np.asarray(cx, np.float64)
    ok = np.isfinite(cy) & np.isfinite(cx)
    qy = np.where(ok, np.round(np.where(ok, cy, 0.0)).astype(np.int64) + int(drift[0]), -1)
    qx = np.where(ok, np.round(np.where(ok, cx, 0.0)).astype(np.int64) + int(drift[1]), -1)
    return qy.astype(np.int64), qx.astype(np.int64)


def check_unique_ids(ids, sel, t):
    chosen = np.asarray(ids)[np.asarray(sel) != 0]
    if np.unique(chosen).size != chosen.size:      # upstream prints a warning and takes the first such row
        raise ValueError("find_events: frame %d has a track id on two valid, non-empty rows" % t)


def pick_mothers(flags, prev, cur, sets):
    """mother row per current row (int64; -1 without a division).  One matching neighbour: the kernel's mother_row.  Several:
    upstream's loop keeps the last match in the iteration order of the row's neighbour SET, so that set (sets[r]) is walked."""
    mother = np.asarray(flags["mother_row"], np.int64).copy()
    several = np.flatnonzero((np.asarray(flags["division"]) != 0) & (np.asarray(flags["n_match"]) > 1))
    if several.size:
        ids, sel, under = np.asarray(cur["id"]), np.asarray(cur["sel"]), np.asarray(cur["under"])
        both = set(np.asarray(prev["id"])[np.asarray(prev["sel"]) != 0].tolist()) & set(ids[sel != 0].tolist())
        edge_ids = set(ids[np.asarray(cur["edge"]) != 0].tolist())
        for r in several:
            for n in list(sets[r]):
                if 0 <= n < ids.size and sel[n] and int(ids[n]) in both and int(ids[n]) not in edge_ids and under[n] != -1 \
                        and under[n] == under[r]:
                    mother[r] = n
    return mother


def found_rows(flags, prev, cur, sets):
    """A pair's flags as the four row lists that travel to rank 0: delaminations and differentiations (previous rows), divisions
    (current rows) and their mothers' rows."""
    mother = pick_mothers(flags, prev, cur, sets)
    division = np.flatnonzero(np.asarray(flags["division"]) != 0)
    return dict(delam=np.flatnonzero(np.asarray(flags["delam"]) != 0), diff=np.flatnonzero(np.asarray(flags["diff"]) != 0),
                division=division, mother=mother[division])


def _collect(step, fields, what, rank, world, dist, device, root=None):
    """Runs an owner step (-> {t: record of `fields`}) and the gather of every rank's records -> all of them in one dict ({} on a
    rank that receives nothing).  A step that raises still joins the gather, with the failure mark, and raises afterwards; the
    ranks that see another rank's mark raise RuntimeError -- no rank is left waiting in a collective."""
    error = None
    try:
        records = step()
    except Exception as e:
        error, records = e, {_FAILED: {name: () for name, _ in fields}}
    parts = gather_varlen(pack_records(records, fields), dist, rank, world, device, root=root)
    if error is not None:
        raise error
    parts = [unpack_records(part, fields) for part in parts or ()]
    bad = [r for r, part in enumerate(parts) if _FAILED in part]
    if bad:
        raise RuntimeError("find_events: %s failed on rank %d" % (what, bad[0]))
    return {t: record for part in parts for t, record in part.items()}


# ---- the collective -----------------------------------------------------------------------------------------------------------------
def find_events(n_frames, backend, tables, ids, rank=0, world=1, dist=None, device="cpu", drifts=None):
    """See movie.find_events."""
    from .pipeline import frames_for_rank
    if getattr(backend, "archive_frames", None) is None or not getattr(backend, "archive", None):
        raise ValueError("find_events needs a backend that kept its frames' archive parts: GpuFrameBackend(..., archive=True)")
    lacking = [m for m in BACKEND_METHODS if not hasattr(backend, m)]
    if lacking:
        raise ValueError("find_events needs a backend with %s" % ", ".join(lacking))
    # 1. rank 0 hands out ids, centroids and drift rows; every rank checks the same numbers
    movie = {}
    if rank == 0:
        movie = {t: dict(drift=tables[t]["drift"] if drifts is None else drifts[t], id=ids[t], cy=tables[t]["cy"], cx=tables[t]["cx"])
                 for t in range(n_frames)}
    movie = unpack_records(broadcast_varlen(pack_records(movie, MOVIE_FIELDS), dist, rank, world, device), MOVIE_FIELDS)
    for t in range(n_frames):
        sizes = set(movie[t][k].size for k in ("id", "cy", "cx")) if t in movie else {0}
        if sizes == {0}:
            raise ValueError("find_events: frame %d has no table" % t)
        if len(sizes) > 1:
            raise ValueError("find_events: frame %d's ids and table differ in length" % t)
        if not np.isfinite(movie[t]["drift"]).all():
            raise ValueError("find_events: the drift row of frame %d is not finite" % t)
    mine = list(frames_for_rank(n_frames, rank, world))

    # 2. every owner publishes its frames' rows and answers the exact look-ups of the NEXT frame's rows in its map
    def publish():
        rows = {}
        for t in mine:
            if t not in backend.archive_frames:
                raise ValueError("find_events: frame %d was not processed by this backend" % t)
            r = dict(backend.event_rows(t), edge=backend.border_rows(t))
            if r["sel"].size != movie[t]["id"].size:
                raise ValueError("find_events: frame %d has %d rows and %d ids" % (t, r["sel"].size, movie[t]["id"].size))
            check_unique_ids(movie[t]["id"], r["sel"], t)
            r["under_next"] = np.zeros(0, np.int32)
            if t + 1 < n_frames:
                nxt = movie[t + 1]
                r["under_next"] = backend.lookup_exact(t, *shifted_positions(nxt["cy"], nxt["cx"], nxt["drift"]))
            rows[t] = r
        return rows

    rows = _collect(publish, ROW_FIELDS, "a frame's rows", rank, world, dist, device)

    # 3. the owner of frame t classifies the pair (t - 1, t); the row lists travel to rank 0
    def classify():
        first_edge_ids = movie[0]["id"][rows[0]["edge"] != 0]
        found = {}
        for t in mine:
            if t >= 1:
                prev = dict(rows[t - 1], id=movie[t - 1]["id"])
                cur = dict(rows[t], id=movie[t]["id"], under=rows[t - 1]["under_next"])
                found[t] = backend.classify_pair(t, prev, cur, first_edge_ids)
        return found

    found = _collect(classify, FOUND_FIELDS, "a pair's classification", rank, world, dist, device, root=0)
    if rank != 0:
        return None
    return events_table(n_frames, tables, ids, [rows[t]["sel"] for t in range(n_frames)], found)


def events_table(n_frames, tables, ids, sel, found):
    """Rank 0's part: the events DataFrame find_events_iterator would leave, from the pairs' row lists.  The rows go through the
    reference route itself -- Tissue.add_event and find_event_frame on a Tissue that holds every frame's small table (label,
    valid = sel, empty_cell = 0, cx, cy, area, type) -- in upstream's order: per frame pair the delaminations, then the
    differentiations, then the divisions, each ascending by id.  Every frame is valid, so start and end are the ends of
    find_valid_frames(frame - 5, frame + 5); a division's end walks back to the daughter's last frame, with the list indexing
    (frame 0 is the last frame) upstream's walk has."""
    import pandas as pd
    from .tissue_info import Tissue
    tissue = Tissue(n_frames)
    for t in range(n_frames):
        tb = tables[t]
        n = np.asarray(ids[t]).size
        tissue.set_cells_info(t + 1, pd.DataFrame({
            "label": np.asarray(ids[t], np.int64), "valid": np.asarray(sel[t]).astype(np.int64), "empty_cell": np.zeros(n, np.int64),
            "cx": np.asarray(tb["cx"], np.float64), "cy": np.asarray(tb["cy"], np.float64), "area": np.asarray(tb["area"], np.int64),
            "type": np.asarray(tb["type"]).astype(np.int64) if "type" in tb else np.zeros(n, np.int64)}))
    for t in range(1, n_frames):
        frame, f = t + 1, found[t]
        around = tissue.find_valid_frames(frame - 5, frame + 5)
        start_frame, end_frame = np.min(around), np.max(around)
        prev_ids, cur_ids = np.asarray(ids[t - 1], np.int64), np.asarray(ids[t], np.int64)
        for cid in np.sort(prev_ids[f["delam"]]):
            tissue.add_event("delamination", start_frame, frame, start_cell_id=cid, source="automatic")
        for cid in np.sort(prev_ids[f["diff"]]):
            tissue.add_event("differentiation", start_frame, end_frame, start_cell_id=cid, source="automatic")
        for k in np.argsort(cur_ids[f["division"]], kind="stable"):
            cid, mother_id = cur_ids[f["division"][k]], cur_ids[f["mother"][k]]
            division_end, daughter_pos = end_frame + 1, None
            while daughter_pos is None:
                division_end -= 1
                if tissue.valid_frames[division_end - 1] == 1:
                    daughter_pos = tissue.get_cell_centroid_by_id(division_end, cid)
            tissue.add_event("division", start_frame, division_end, start_cell_id=mother_id, daughter_cell_id=cid,
                             second_end_pos=daughter_pos, source="automatic")
    return tissue.events
