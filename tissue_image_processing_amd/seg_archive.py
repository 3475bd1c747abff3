"""A finished movie as a `.seg` archive (movie.save_seg): the zip writer that takes members which are deflated already, the
per-frame cell table as the Tissue route leaves it, built from the tables the movie driver kept, and the collective that brings
every owner's members to rank 0.

The label maps and type maps never reach the host uncompressed: GpuFrameBackend(archive=...) has them deflated on their own GPU
(csrc/tip_deflate.hip) and keeps the streams; this module only wraps them (_deflate.npy_member) and writes the archive."""
import struct
import zlib

import numpy as np

from ._collectives import broadcast_varlen, gather_varlen, pack_records, unpack_records
from ._deflate import npy_header, npy_member

ZIP32_MAX = 0xFFFFFFFF          # a size or an offset of this value or above needs zip64
ZIP32_MAX_ENTRIES = 0xFFFF
_DOS_TIME, _DOS_DATE = 0, (1 << 5) | 1      # 1980-01-01 00:00: the archive's bytes depend on its members alone


def deflate_small(data, level=6):
    """(raw deflate stream, CRC-32, size) of a small host buffer through zlib (tables, names: kilobytes)."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush(), zlib.crc32(data), len(data)


def write_raw_zip(path, members):
    """Writes a zip archive of members that are ALREADY deflated -- (name, raw deflate stream, CRC-32 of the uncompressed bytes,
    uncompressed size), method 8, which the standard library's zipfile cannot take -- in the given order: local headers, the
    central directory, the end record.  An archive that would need zip64 (a size or an offset of 2^32 - 1 or more, 65535 or
    more members) raises ValueError, naming the limit, before anything is written."""
    members = [(name.encode("utf-8") if isinstance(name, str) else bytes(name), bytes(raw), int(crc) & 0xFFFFFFFF, int(size))
               for name, raw, crc, size in members]
    if len(members) >= ZIP32_MAX_ENTRIES:
        raise ValueError("%d members: a zip archive without zip64 holds fewer than %d" % (len(members), ZIP32_MAX_ENTRIES))
    offset, offsets = 0, []
    for name, raw, crc, size in members:
        if size >= ZIP32_MAX or len(raw) >= ZIP32_MAX:
            raise ValueError("member %s: %d bytes (%d deflated) need zip64; the limit is %d" % (name.decode(), size, len(raw), ZIP32_MAX - 1))
        offsets.append(offset)
        offset += 30 + len(name) + len(raw)
    central = sum(46 + len(name) for name, _, _, _ in members)
    if offset >= ZIP32_MAX or central >= ZIP32_MAX or offset + central >= ZIP32_MAX:
        raise ValueError("the archive's central directory would start at byte %d (%d bytes long): offsets of %d or more need zip64"
                         % (offset, central, ZIP32_MAX))
    with open(path, "wb") as fh:
        for name, raw, crc, size in members:
            fh.write(struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, 0, 8, _DOS_TIME, _DOS_DATE, crc, len(raw), size, len(name), 0))
            fh.write(name)
            fh.write(raw)
        for (name, raw, crc, size), at in zip(members, offsets):
            fh.write(struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 20, 20, 0, 8, _DOS_TIME, _DOS_DATE, crc, len(raw), size, len(name),
                                 0, 0, 0, 0, 0, at))
            fh.write(name)
        fh.write(struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, len(members), len(members), central, offset, 0))
    return path


# ---- the frame table -----------------------------------------------------------------------------------------------------
def _find_neighbors(neighbors, n_neighbors, by_hi, working_indices):
    """TissueHipMixin.find_neighbors on the kept pair list: a working cell's set becomes its lower-labelled partners, each of
    which gains the cell in turn."""
    for cell_index in working_indices:
        neighbors[cell_index] = set()
    for cell_index in working_indices:
        cell_label = int(cell_index) + 1
        nl = by_hi.get(cell_label)
        if nl:
            neighbors[cell_index] = neighbors[cell_index].union(nl)
            for nb in nl:
                neighbors[nb - 1].add(cell_label)
                n_neighbors[nb - 1] = len(neighbors[nb - 1])
    for cell_index in working_indices:
        n_neighbors[cell_index] = len(neighbors[cell_index])


def neighbor_sets(kept, typed, min_cell_area=0.1, max_cell_area=10):
    """The neighbour sets of one frame's rows as the Tissue route leaves them, from the kept parts (area, pairs and, typed, the row
    `valid`): calculate_frame_cellinfo's find_neighbors over the rows valid by the area rule, then -- typed -- calc_cell_types'
    second pass over the newly valid rows, which CLEARS their sets first.  -> (neighbors: object array of sets of 1-based labels,
    n_neighbors int64, valid by the area rule, valid in the end), what frame_table writes and movie.find_events classifies."""
    area = np.asarray(kept["area"], np.int64)
    n = area.size
    smallest, largest = min_cell_area * area.mean(), max_cell_area * area.mean()
    first_valid = (area > smallest) & (area < largest)
    pairs = np.asarray(kept["pairs"]).astype(np.int64).reshape(-1, 2)
    if pairs.size:
        pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]      # _segmentation.neighbor_pairs' order
    by_hi = {}
    for hi, lo in pairs:
        by_hi.setdefault(int(hi), []).append(int(lo))
    neighbors = np.empty(n, object)
    for i in range(n):
        neighbors[i] = set()
    n_neighbors = np.zeros(n, np.int64)
    _find_neighbors(neighbors, n_neighbors, by_hi, np.flatnonzero(first_valid))
    valid = first_valid
    if typed:
        valid = np.asarray(kept["valid"]) != 0
        _find_neighbors(neighbors, n_neighbors, by_hi, np.flatnonzero(valid & ~first_valid))
    return neighbors, n_neighbors, first_valid, valid


def frame_table(kept, ids, type_name=None, min_cell_area=0.1, max_cell_area=10):
    """The cells_info table of one frame as the Tissue route leaves it -- set_labels, calculate_frame_cellinfo, then
    calc_cell_types(plane, ..., type_name) when the frame was typed, then `label` set to the track ids -- from what the movie
    driver kept of the frame's device passes: area, bbox, sumy, sumx, pc (perimeter pixel counts), pairs (neighbour pairs) and,
    typed, the rows type / valid / mean_intensity.  No device work: perimeter and centroids are formed as
    _segmentation.regionprops_arrays forms them, validity and neighbour sets as calculate_frame_cellinfo / find_neighbors do."""
    import pandas as pd      # noqa: F401 (make_df needs it)
    from .tissue_info import CELL_INFO_SPECS, make_df
    area = np.asarray(kept["area"], np.int64)
    n = area.size
    if n == 0:
        return None                       # calculate_frame_cellinfo leaves no table for an empty label map
    pc = np.asarray(kept["pc"], np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cy = kept["sumy"] / area
        cx = kept["sumx"] / area
    sq2 = np.sqrt(2.0)
    perimeter = pc[:, 0] * 1.0 + pc[:, 1] * sq2 + pc[:, 2] * ((1 + sq2) / 2)
    present = area > 0
    columns = {"label": np.arange(1, n + 1), "area": area, "perimeter": perimeter, "cx": cx, "cy": cy}
    for j, edge in enumerate(("min_row", "min_col", "max_row", "max_col")):
        columns["bounding_box_" + edge] = np.asarray(kept["bbox"])[:, j]
    info = make_df(n, CELL_INFO_SPECS)
    for name, values in columns.items():
        full = np.zeros(n, dtype=np.float64 if name in ("perimeter", "cx", "cy") else np.int64)
        full[present] = np.asarray(values)[present]
        info[name] = full
    neighbors, n_neighbors, first_valid, valid = neighbor_sets(kept, type_name is not None, min_cell_area, max_cell_area)
    info["valid"] = first_valid.astype(int)
    if type_name is not None:             # calc_cell_types on a fresh table: the new type is bit 0
        rows = np.flatnonzero(present)
        info.loc[rows, "mean_intensity_" + type_name] = np.asarray(kept["mean_intensity"], np.float64)[rows]
        info.loc[:, "valid"] = valid.astype(int)
        info.loc[:, "type"] = np.asarray(kept["type"]).astype(np.int64)
    info["neighbors"] = list(neighbors)
    info["n_neighbors"] = n_neighbors
    info.loc[:, "label"] = np.asarray(ids, np.int64)
    return info


# ---- members and their way to rank 0 -------------------------------------------------------------------------------------
ID_FIELDS = (("ids", np.int64),)      # rank 0's hand-out, keyed by frame
MEMBER_FIELDS = (("name", np.uint8), ("stream", np.uint8), ("crc", np.int64), ("size", np.int64))      # keyed by the member's index


def members_as_records(members):
    """[(name, stream, CRC, size)] -> {index: record of MEMBER_FIELDS}, name and stream as their bytes."""
    return {k: dict(name=np.frombuffer(name.encode("utf-8"), np.uint8), stream=np.frombuffer(raw, np.uint8), crc=crc, size=size)
            for k, (name, raw, crc, size) in enumerate(members)}


def records_as_members(records):
    """members_as_records undone, `str` names and `bytes` streams."""
    return [(r["name"].tobytes().decode("utf-8"), r["stream"].tobytes(), int(r["crc"][0]), int(r["size"][0])) for r in records.values()]


def _ids_to_owners(ids, n_frames, rank, world, dist, device):
    """Rank 0 hands out the track ids in one broadcast (kilobytes per frame); every rank keeps its own frames'."""
    from .pipeline import frames_for_rank
    flat = pack_records({t: dict(ids=ids[t]) for t in range(n_frames)} if rank == 0 else {}, ID_FIELDS)
    every = unpack_records(broadcast_varlen(flat, dist, rank, world, device), ID_FIELDS)
    return {t: every[t]["ids"] for t in frames_for_rank(n_frames, rank, world)}


def frame_members(t, kept, ids, shape, type_name):
    """Frame t's archive members (names count frames from 1): labels, types when the frame was typed, the table."""
    Y, X = shape
    members = []
    stream, crc = kept["labels"]
    members.append(("frame_%d_labels.npy" % (t + 1),) + npy_member(npy_header((Y, X), np.int32), stream, crc, Y * X * 4))
    if kept.get("types") is not None:
        stream, crc = kept["types"]
        members.append(("frame_%d_types.npy" % (t + 1),) + npy_member(npy_header((Y, X), np.uint8), stream, crc, Y * X))
    table = frame_table(kept, ids, type_name if kept.get("types") is not None else None)
    if table is not None:
        import io
        buf = io.BytesIO()
        table.to_pickle(buf, compression=None)
        members.append(("frame_%d_data.pkl" % (t + 1),) + deflate_small(buf.getvalue()))
    return members


def save_seg(path, n_frames, backend, tables, ids, rank=0, world=1, dist=None, device="cpu", channel_names=(), events=None):
    """See movie.save_seg."""
    import io
    import json
    import pickle
    from .tissue_info import EVENTS_INFO_SPEC, make_df
    kept = getattr(backend, "archive_frames", None)
    if kept is None or not getattr(backend, "archive", None):
        raise ValueError("save_seg needs a backend that kept its frames' archive parts: GpuFrameBackend(..., archive=True)")
    type_name = backend.archive.get("type_name") if getattr(backend, "cell_types", None) is not None else None
    mine = _ids_to_owners(ids, n_frames, rank, world, dist, device)
    missing = [t for t in mine if t not in kept]
    if missing:
        raise ValueError("save_seg: frames %s were not processed by this backend" % missing)
    members = [m for t in sorted(mine) for m in frame_members(t, kept[t], mine[t], (backend.Y, backend.X), type_name)]
    parts = gather_varlen(pack_records(members_as_records(members), MEMBER_FIELDS), dist, rank, world, device, root=0)
    if rank != 0:
        return None
    members = [m for part in parts for m in records_as_members(unpack_records(part, MEMBER_FIELDS))]
    by_name = {m[0]: m for m in members}
    ordered = [by_name[name] for k in range(1, n_frames + 1)
               for name in ("frame_%d_labels.npy" % k, "frame_%d_types.npy" % k, "frame_%d_data.pkl" % k) if name in by_name]

    def small(name, write):
        buf = io.BytesIO()
        write(buf)
        ordered.append((name,) + deflate_small(buf.getvalue()))

    # the movie-wide members, in Tissue._archive_members' order
    small("events_data.pkl", lambda fh: (make_df(0, EVENTS_INFO_SPEC) if events is None else events).to_pickle(fh, compression=None))
    small("drifts.npy", lambda fh: np.save(fh, np.array([tables[t]["drift"] for t in range(n_frames)], np.float64).reshape(n_frames, 2)))
    small("valid_frames.npy", lambda fh: np.save(fh, np.ones((n_frames,)).astype(int)))
    small("shape_fitting_data.json", lambda fh: fh.write(json.dumps([dict() for _ in range(n_frames)]).encode()))
    small("cell_type_names.pkl", lambda fh: pickle.dump([type_name] if type_name is not None else [], fh))
    small("channel_names.pkl", lambda fh: pickle.dump(list(channel_names), fh))
    small("fake_channels.pkl", lambda fh: pickle.dump([], fh))
    return write_raw_zip(path.replace(".seg", "") + ".seg", ordered)
