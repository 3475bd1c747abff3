"""A finished movie as the TIFF of Tissue.export_segmentation_and_cell_types_to_tiff (ti.py:4040-4052) -- T x C x 1 x Y x X uint16,
channel 0 the tracking labels, channel 1 the type map with 0 -> 2 and 255 -> 0 -- written from maps that never leave their GPU
uncompressed: csrc/tip_export.hip turns a frame's resident label and type map into uint16 pages, csrc/tip_deflate.hip's strip
entry turns the pages into one zlib stream per TIFF strip, only the streams are downloaded, and
tiff.write_tiff_strips puts them behind their IFDs (movie.export_tiff, and the Tissue mixin's
compression="device")."""
import numpy as np

from ._collectives import gather_varlen, pack_records, unpack_records

STRIP_FIELDS = (("stream", np.uint8), ("sizes", np.int64))      # keyed by frame: its pages' strips end to end, and their sizes
MISSING_FIELDS = (("frames", np.int64), ("wide", np.int64))     # keyed by rank: frames without maps, frames with an id no uint16 holds


class PageEncoder(object):
    """The device side of one (Y, X) frame's export: a buffer for its uint16 pages and one for their streams, made on first use
    and kept.  It belongs to the thread that made it (the library's contexts are per thread)."""

    def __init__(self, Y, X):
        self.Y, self.X = int(Y), int(X)
        self._pages = self._streams = None

    def encode(self, labels_ptr, types_ptr, ids, rowsperstrip, codes):
        """DEVICE maps (int32 labels; uint8 types or None) -> per page -- tracking labels, then types when given -- the list of its
        strips' zlib streams.  ids: the track id of every label 1 .. len(ids) (int64).  ValueError for an id that no uint16
        holds and for a label the ids do not cover."""
        from . import _lib
        from ._deflate import deflate_strips_dev, export_maps_u16_dev, split_strips, strips_bound
        from .tiff import StripGeometry
        Y, X = self.Y, self.X
        n_pages = 1 if types_ptr is None else 2
        rps = StripGeometry(Y, rowsperstrip).rows_per_strip
        cap = strips_bound(2, Y, 2 * X, rps)
        if self._pages is None:
            self._pages = _lib.DeviceBuffer(2 * Y * X * 2)
        if self._streams is None or self._streams.nbytes < cap:
            self._streams = _lib.DeviceBuffer(cap)
        export_maps_u16_dev(labels_ptr, types_ptr, Y * X, ids, self._pages.ptr)
        table, total = deflate_strips_dev(self._pages.ptr, n_pages, Y, 2 * X, 2, rps, codes, self._streams.ptr, self._streams.nbytes)
        return split_strips(self._streams.download((total,), np.uint8), table, n_pages)


def strips_as_record(pages):
    """per page lists of streams -> a record of STRIP_FIELDS"""
    flat = [s for page in pages for s in page]
    return dict(stream=np.frombuffer(b"".join(flat), np.uint8), sizes=[len(s) for s in flat])


def record_as_strips(record, n_pages):
    """strips_as_record undone"""
    sizes = [int(n) for n in record["sizes"]]
    if n_pages < 1 or len(sizes) % n_pages:
        raise ValueError("a frame came with %d strips for %d pages" % (len(sizes), n_pages))
    stream, at, flat = record["stream"].tobytes(), 0, []
    for n in sizes:
        flat.append(stream[at:at + n])
        at += n
    per_page = len(sizes) // n_pages
    return [flat[k * per_page:(k + 1) * per_page] for k in range(n_pages)]


def export_tiff(path, n_frames, backend, ids, rank=0, world=1, dist=None, device="cpu", rowsperstrip=None, codes="dynamic", bigtiff=None):
    """See movie.export_tiff."""
    from ._deflate import strip_codes
    from .tiff import StripGeometry, default_rows_per_strip, write_tiff_strips
    from .seg_archive import _ids_to_owners
    Y, X = int(backend.Y), int(backend.X)
    channels = 2 if getattr(backend, "cell_types", None) is not None else 1
    rps = default_rows_per_strip(Y, 2 * X) if rowsperstrip is None else int(rowsperstrip)
    if rps < 1:
        raise ValueError("export_tiff: rowsperstrip %d" % rps)
    rps = StripGeometry(Y, rps).rows_per_strip
    strip_codes(codes)
    mine = _ids_to_owners(ids, n_frames, rank, world, dist, device)
    # a frame without its maps is every rank's error: the owners say which they lack before any of them encodes
    lacking = sorted(t for t in mine if t not in backend.labels or (channels == 2 and t not in backend.type_maps))
    wide = sorted(t for t in mine if mine[t].size and (mine[t].min() < 0 or mine[t].max() > 65535))
    said = gather_varlen(pack_records({rank: dict(frames=lacking, wide=wide)}, MISSING_FIELDS), dist, rank, world, device)
    said = [r for part in said for r in unpack_records(part, MISSING_FIELDS).values()]
    missing, wide = (sorted(int(t) for r in said for t in r[name]) for name in ("frames", "wide"))
    if missing:
        raise ValueError("export_tiff: frames %s were not processed by this backend" % missing)
    if wide:
        raise ValueError("export_tiff: frames %s hold a track id outside [0, 65535], which a uint16 page cannot hold" % wide)
    records = {t: strips_as_record(backend.export_page_strips(t, mine[t], rps, codes)) for t in sorted(mine)}
    parts = gather_varlen(pack_records(records, STRIP_FIELDS), dist, rank, world, device, root=0)
    if rank != 0:
        return None
    by_frame = {t: r for part in parts for t, r in unpack_records(part, STRIP_FIELDS).items()}
    pages = [page for t in range(n_frames) for page in record_as_strips(by_frame[t], channels)]
    return write_tiff_strips(path, (n_frames, channels, 1, Y, X), "TCZYX", np.uint16, rps, pages, bigtiff=bigtiff)
