"""A finished movie as the TIFF of Tissue.export_segmentation_and_cell_types_to_tiff (ti.py:4040-4052) -- T x C x 1 x Y x X uint16,
channel 0 the tracking labels, channel 1 the type map with 0 -> 2 and 255 -> 0 -- written from maps that never leave their GPU
uncompressed: csrc/tip_export.hip turns a frame's resident label and type map into uint16 pages, csrc/tip_deflate.hip's strip
entry turns the pages into one zlib stream per TIFF strip, only the streams are downloaded, and
tiff.write_tiff_strips puts them behind their IFDs (movie.export_tiff, and the Tissue mixin's
compression="device").

The projected movie goes the same way (movie.export_projection, and movie_surface_projection's compression="device"): the float64
projection planes become the uint16 pages of save_tiff(..., data_type="uint16") on the device (ProjectionEncoder), T x C x Y x X,
scaled by the whole movie's maximum."""
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


class ProjectionEncoder(object):
    """The device side of one (C, Y, X) frame of the projected movie (movie.export_projection): a buffer for its uint16 pages and
    one for their streams, made on first use and kept; owned like a PageEncoder, by the thread that made it."""

    def __init__(self, C, Y, X):
        self.C, self.Y, self.X = int(C), int(Y), int(X)
        self._pages = self._streams = None

    def encode(self, proj_ptr, scale_max, rowsperstrip, codes, predictor=1):
        """DEVICE float64 planes (C, Y, X) -> per channel the list of its strips' zlib streams: the uint16 page of
        tiff_normalise for a movie whose maximum is scale_max, differenced along x for predictor 2.  ValueError for a scale_max
        that is negative or not finite."""
        from ._deflate import projection_pages_u16_dev
        self._reserve(rowsperstrip)
        projection_pages_u16_dev(proj_ptr, self.C, self.Y, self.X, scale_max, predictor, self._pages.ptr)
        return self._deflate(rowsperstrip, codes)

    def encode_pages(self, pages, rowsperstrip, codes):
        """HOST uint16 pages (C, Y, X), written as they are -> per channel the list of its strips' zlib streams."""
        pages = np.ascontiguousarray(pages)
        if pages.dtype != np.uint16 or pages.shape != (self.C, self.Y, self.X):
            raise TypeError("encode_pages takes uint16 pages %s, not %s %s" % ((self.C, self.Y, self.X), pages.dtype, pages.shape))
        self._reserve(rowsperstrip)
        self._pages.upload(pages)
        return self._deflate(rowsperstrip, codes)

    def _reserve(self, rowsperstrip):
        from . import _lib
        from ._deflate import strips_bound
        from .tiff import StripGeometry
        cap = strips_bound(self.C, self.Y, 2 * self.X, StripGeometry(self.Y, rowsperstrip).rows_per_strip)
        if self._pages is None:
            self._pages = _lib.DeviceBuffer(self.C * self.Y * self.X * 2)
        if self._streams is None or self._streams.nbytes < cap:
            self._streams = _lib.DeviceBuffer(cap)

    def _deflate(self, rowsperstrip, codes):
        from ._deflate import deflate_strips_dev, split_strips
        from .tiff import StripGeometry
        rps = StripGeometry(self.Y, rowsperstrip).rows_per_strip
        table, total = deflate_strips_dev(self._pages.ptr, self.C, self.Y, 2 * self.X, 2, rps, codes, self._streams.ptr, self._streams.nbytes)
        return split_strips(self._streams.download((total,), np.uint8), table, self.C)


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


LACKING_FIELDS = (("frames", np.int64),)        # keyed by rank: its frames without a kept projection (or z-map)
MAXIMUM_FIELDS = (("maximum", np.float64),)     # keyed by frame: the maximum of its projection planes
ZMAP_FIELDS = (("zmap", np.uint16),)            # keyed by frame: its z-map as uint16, raw


def zmap_path_for(path):
    """`zmap_<name>.npy` beside `path`, <name> its basename without ".tif": where Tissue.load_height_map looks (ti.py:3568-3575)."""
    import os
    folder, name = os.path.split(path)
    return os.path.join(folder, "zmap_%s.npy" % (name[:-4] if name.lower().endswith(".tif") else name))


def export_projection(path, n_frames, backend, rank=0, world=1, dist=None, device="cpu", rowsperstrip=None, codes="dynamic", predictor=1,
                      bigtiff=None, zmap=True, metadata=None):
    """See movie.export_projection."""
    from ._deflate import strip_codes
    from .pipeline import frames_for_rank
    from .tiff import STRIP_BYTES, StripGeometry, default_rows_per_strip, metadata_xml, write_tiff_strips
    C, Y, X = int(backend.C), int(backend.Y), int(backend.X)
    if n_frames < 1:
        raise ValueError("export_projection: %d frames" % n_frames)
    if 2 * X > STRIP_BYTES:
        raise ValueError("export_projection: a row of %d uint16 samples is over %d bytes, and a strip is one chunk of the encoder" % (X, STRIP_BYTES))
    if predictor not in (1, 2):
        raise ValueError("export_projection: predictor %r (1: none, 2: horizontal differencing)" % (predictor,))
    rps = default_rows_per_strip(Y, 2 * X) if rowsperstrip is None else int(rowsperstrip)
    if rps < 1:
        raise ValueError("export_projection: rowsperstrip %d" % rps)
    rps = StripGeometry(Y, rps).rows_per_strip
    strip_codes(codes)
    mine = sorted(frames_for_rank(n_frames, rank, world))
    # a frame without its projection is every rank's error: the owners say which they lack before any of them encodes
    lacking = [t for t in mine if t not in backend.projections or (zmap and t not in backend.zmaps)]
    said = gather_varlen(pack_records({rank: dict(frames=lacking)}, LACKING_FIELDS), dist, rank, world, device)
    missing = sorted(int(t) for part in said for r in unpack_records(part, LACKING_FIELDS).values() for t in r["frames"])
    if missing:
        raise ValueError("export_projection: frames %s hold no projection on their owner's backend (GpuFrameBackend(..., keep_projection=True))"
                         % missing)
    # the normalisation is the whole movie's: every rank learns every frame's maximum and takes the largest
    maxima = pack_records({t: dict(maximum=[backend.projection_max(t)]) for t in mine}, MAXIMUM_FIELDS)
    maxima = [r["maximum"][0] for part in gather_varlen(maxima, dist, rank, world, device) for r in unpack_records(part, MAXIMUM_FIELDS).values()]
    scale_max = float(np.max(maxima))
    if not np.isfinite(scale_max) or scale_max < 0:
        raise ValueError("export_projection: the movie's maximum is %r; save_tiff's scaling needs one that is finite and not negative" % scale_max)
    records = {t: strips_as_record(backend.projection_page_strips(t, scale_max, rps, codes, predictor)) for t in mine}
    parts = gather_varlen(pack_records(records, STRIP_FIELDS), dist, rank, world, device, root=0)
    zparts = None
    if zmap:
        zparts = gather_varlen(pack_records({t: dict(zmap=backend.zmap_u16(t)) for t in mine}, ZMAP_FIELDS), dist, rank, world, device, root=0)
    if rank != 0:
        return None
    by_frame = {t: r for part in parts for t, r in unpack_records(part, STRIP_FIELDS).items()}
    pages = [page for t in range(n_frames) for page in record_as_strips(by_frame[t], C)]
    write_tiff_strips(path, (n_frames, C, Y, X), "TCYX", np.uint16, rps, pages, bigtiff=bigtiff, predictor=predictor,
                      xml=metadata_xml(metadata, "export_projection"))
    if not zmap:
        return path, None
    zmaps = {t: r["zmap"] for part in zparts for t, r in unpack_records(part, ZMAP_FIELDS).items()}
    zmap_path = zmap_path_for(path)
    np.save(zmap_path, np.stack([zmaps[t].reshape(Y, X) for t in range(n_frames)]).reshape(n_frames, 1, 1, Y, X))
    return path, zmap_path


def save_projection_tiff(path, movie, metadata=None, rowsperstrip=None, codes="dynamic", predictor=1, bigtiff=None):
    """save_tiff(path, movie, metadata, axes="TCYX", data_type="uint16") for a HOST movie (T, C, Y, X) with the strips deflated on
    the calling thread's GPU (movie_surface_projection's compression="device").  Every frame is uploaded and comes back as strips,
    which write_tiff_strips writes as they arrive.  A float64 movie becomes uint16 pages under its maximum on the device
    (ProjectionEncoder.encode: what tiff_normalise does on the host); a uint16 movie -- concatenate_time_points' -- is written as
    it is, as save_tiff writes it (encode_pages; predictor 1 only)."""
    from . import _lib
    from .tiff import STRIP_BYTES, default_rows_per_strip, metadata_xml, write_tiff_strips
    movie = np.asarray(movie)
    if movie.ndim != 4 or movie.dtype not in (np.float64, np.uint16) or movie.size == 0:
        raise TypeError("save_projection_tiff takes a float64 or uint16 movie (T, C, Y, X), not %s %s" % (movie.dtype, movie.shape))
    T, C, Y, X = movie.shape
    if 2 * X > STRIP_BYTES:
        raise ValueError("save_projection_tiff: a row of %d uint16 samples is over %d bytes, and a strip is one chunk of the encoder" % (X, STRIP_BYTES))
    rps = default_rows_per_strip(Y, 2 * X) if rowsperstrip is None else int(rowsperstrip)
    encoder = ProjectionEncoder(C, Y, X)
    if movie.dtype == np.uint16:
        if predictor != 1:
            raise ValueError("save_projection_tiff: predictor %r for a uint16 movie (its pages are written as they are: 1)" % (predictor,))
        pages = (page for t in range(T) for page in encoder.encode_pages(movie[t], rps, codes))
        return write_tiff_strips(path, movie.shape, "TCYX", np.uint16, rps, pages, bigtiff=bigtiff, xml=metadata_xml(metadata))
    scale_max, frame = float(np.max(movie)), _lib.DeviceBuffer(C * Y * X * 8)

    def normalised():
        for t in range(T):
            frame.upload(movie[t])
            for page in encoder.encode(frame.ptr, scale_max, rps, codes, predictor):
                yield page

    try:
        return write_tiff_strips(path, movie.shape, "TCYX", np.uint16, rps, normalised(), bigtiff=bigtiff, predictor=predictor,
                                 xml=metadata_xml(metadata))
    finally:
        frame.free()
