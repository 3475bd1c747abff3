"""The TIFF container, host side: the reader (page table, host decode, the lazy image source) and the writers behind read_tiff /
save_tiff (bim.py:28-51, 160-188), the deflate-strip exports and the streamed BigTIFF.  numpy and the standard library only; the
device's part -- inflating and deflating strips -- is _inflate.py / _deflate.py, and basic_image_manipulations re-exports the
public names.

What is read and written: little- or big-endian (written: little), classic (magic 42, 4-byte offsets) or BigTIFF (magic 43, 8-byte
offsets), strips of one sample per pixel, uncompressed or one zlib stream per strip, predictor 1 or 2."""
import struct

import numpy as np

TIFF_DEFLATE = (8, 32946)          # Compression: Adobe deflate and the legacy code; both are zlib streams (RFC 1950), one per strip

# 64 KB of raw rows: the default strip of every compressed writer here, and the most rows tip_deflate_strips takes as one strip
STRIP_BYTES = 65536


# ---- strip geometry --------------------------------------------------------------------------------------------------------
def default_rows_per_strip(rows, row_bytes):
    """As many rows as STRIP_BYTES hold, at least 1 and at most the page's."""
    return max(1, min(int(rows), STRIP_BYTES // max(1, int(row_bytes))))


class StripGeometry(object):
    """A page of `rows` rows cut into strips of `rowsperstrip`: rows_per_strip (clamped to the page, at least 1), the number of
    strips, and strip_rows(k) -- rows_per_strip but for a ragged last strip."""
    __slots__ = ("rows", "rows_per_strip", "strips")

    def __init__(self, rows, rowsperstrip):
        self.rows = int(rows)
        self.rows_per_strip = max(1, min(int(rowsperstrip), self.rows))
        self.strips = -(-self.rows // self.rows_per_strip)

    def strip_rows(self, k):
        return min(self.rows_per_strip, self.rows - k * self.rows_per_strip)


# ---- the reader ------------------------------------------------------------------------------------------------------------
def _tiff_axes_from_description(desc, npages, rows, cols):
    """(axes, shape) from the first page's ImageDescription: save_tiff's "axes=... shape=...", tifffile's own JSON
    {"shape": [...], "axes": "..."}, ImageJ's hyperstack keys, else a plain page stack."""
    import re
    if desc.startswith("{"):
        import json
        try:
            meta = json.loads(desc)
        except ValueError:
            meta = None
        if isinstance(meta, dict) and isinstance(meta.get("shape"), list) and all(isinstance(v, int) for v in meta["shape"]):
            shape, axes = tuple(meta["shape"]), meta.get("axes")
            if int(np.prod(shape)) == npages * rows * cols and shape[-2:] == (rows, cols):
                if not (isinstance(axes, str) and len(axes) == len(shape)):
                    axes = "Q" * (len(shape) - 2) + "YX"      # (tifffile's name for axes it was not told)
                return axes.upper(), shape
    m = re.search(r"axes=([A-Za-z]*) shape=([0-9x]+)", desc)
    if m and m.group(2):
        shape = tuple(int(v) for v in m.group(2).split("x"))
        if int(np.prod(shape)) == npages * rows * cols:
            return m.group(1).upper(), shape
    if desc.startswith("ImageJ="):
        keys = dict(line.split("=", 1) for line in desc.splitlines() if "=" in line)
        t, z, c = int(keys.get("frames", 1)), int(keys.get("slices", 1)), int(keys.get("channels", 1))
        if t * z * c == npages:
            axes, shape = "", ()
            for name, n in (("T", t), ("Z", z), ("C", c)):
                if n > 1:
                    axes += name
                    shape += (n,)
            return axes + "YX", shape + (rows, cols)
    if npages > 1:
        return "QYX", (npages, rows, cols)           # (tifffile's name for an unknown page axis)
    return "YX", (rows, cols)


class TiffPage(object):
    """One IFD of a strip-organised TIFF, as tiff_page_table reads it: no pixel data."""
    __slots__ = ("index", "cols", "rows", "bits", "sample_format", "samples", "compression", "predictor", "rows_per_strip",
                 "offsets", "counts", "tiled", "description")

    @property
    def strips(self):
        return StripGeometry(self.rows, self.rows_per_strip).strips

    def strip_rows(self, k):
        return StripGeometry(self.rows, self.rows_per_strip).strip_rows(k)


class TiffTable(object):
    """tiff_page_table's result: the pages, the file's byte order ("<" or ">"), classic or BigTIFF, and the memory map the
    offsets point into."""

    def __init__(self, path, buf, byte_order, big, pages):
        self.path, self.buf, self.byte_order, self.big, self.pages = path, buf, byte_order, big, pages

    @property
    def description(self):
        return self.pages[0].description if self.pages else ""


def tiff_page_table(path):
    """The IFDs of a TIFF / BigTIFF file through a memory map -- extents, bits, sample format, compression, predictor, rows per
    strip, strip offsets and byte counts per page; the file's byte order and flavour -- without touching pixel data."""
    import mmap
    with open(path, "rb") as fh:
        try:
            buf = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        except ValueError:
            buf = b""                         # (an empty file cannot be mapped)
    if len(buf) < 8 or buf[:2] not in (b"II", b"MM"):
        raise ValueError("%s is not a TIFF file" % path)
    bo = "<" if buf[:2] == b"II" else ">"
    magic, = struct.unpack(bo + "H", buf[2:4])
    if magic == 42:                       # classic: 4-byte offsets, 12-byte entries, 2-byte entry count
        big, ifd = False, struct.unpack(bo + "I", buf[4:8])[0]
    elif magic == 43:                     # BigTIFF: 8-byte offsets, 20-byte entries, 8-byte entry count
        big, ifd = True, struct.unpack(bo + "Q", buf[8:16])[0]
    else:
        raise ValueError("%s: not a TIFF / BigTIFF file (magic %d)" % (path, magic))
    sizes = {1: 1, 2: 1, 3: 2, 4: 4, 6: 1, 8: 2, 9: 4, 16: 8, 17: 8}
    codes = {1: "B", 3: "H", 4: "I", 6: "b", 8: "h", 9: "i", 16: "Q", 17: "q"}
    cnt_fmt, ent_size, inline, off_fmt = ("Q", 20, 8, "Q") if big else ("H", 12, 4, "I")
    pages = []
    while ifd:
        hdr = struct.calcsize(cnt_fmt)
        n, = struct.unpack(bo + cnt_fmt, buf[ifd:ifd + hdr])
        tags = {}
        for k in range(n):
            e = buf[ifd + hdr + ent_size * k: ifd + hdr + ent_size * (k + 1)]
            tag, typ = struct.unpack(bo + "HH", e[:4])
            cnt, = struct.unpack(bo + off_fmt, e[4:4 + inline])
            raw = e[4 + inline:]
            if typ not in sizes:
                continue
            nbytes = sizes[typ] * cnt
            at = struct.unpack(bo + off_fmt, raw)[0] if nbytes > inline else 0
            data = raw[:nbytes] if nbytes <= inline else buf[at:at + nbytes]
            tags[tag] = bytes(data) if typ == 2 else struct.unpack(bo + "%d%s" % (cnt, codes[typ]), data)
        ifd, = struct.unpack(bo + off_fmt, buf[ifd + hdr + ent_size * n: ifd + hdr + ent_size * n + inline])
        pg = TiffPage()
        pg.index = len(pages)
        pg.cols, pg.rows, pg.bits = tags[256][0], tags[257][0], tags.get(258, (1,))[0]
        pg.sample_format, pg.samples = tags.get(339, (1,))[0], tags.get(277, (1,))[0]
        pg.compression, pg.predictor = tags.get(259, (1,))[0], tags.get(317, (1,))[0]
        pg.tiled = 322 in tags or 324 in tags
        pg.rows_per_strip = StripGeometry(pg.rows, tags.get(278, (pg.rows,))[0]).rows_per_strip
        pg.offsets = tags.get(273, ())
        pg.counts = tags.get(279, (pg.rows * pg.cols * (pg.bits // 8),) if len(pg.offsets) == 1 else ())
        pg.description = tags[270].split(b"\0")[0].decode("latin-1") if 270 in tags else ""
        pages.append(pg)
    return TiffTable(path, buf, bo, big, pages)


def _tiff_check_page(path, pg):
    """What is read here: strips of one sample per pixel, uncompressed (any 8 / 16 / 32 / 64-bit type) or deflate (8- and 16-bit
    unsigned), predictor 1, or 2 on 8- and 16-bit unsigned.  Anything else raises with the tag value met."""
    where = "%s: page %d" % (path, pg.index)
    if pg.tiled:
        raise ValueError("%s is tiled (TileWidth / TileLength present); only strips are read here" % where)
    if pg.samples != 1:
        raise ValueError("%s: SamplesPerPixel %d; multi-sample pages are not read here" % (where, pg.samples))
    if pg.compression != 1 and pg.compression not in TIFF_DEFLATE:
        names = {5: "LZW", 6: "old JPEG", 7: "JPEG", 32773: "PackBits", 50000: "zstd", 34925: "LZMA"}
        raise ValueError("%s: compression %d%s; only uncompressed (1) and deflate (8, 32946) strips are read here"
                         % (where, pg.compression, " (%s)" % names[pg.compression] if pg.compression in names else ""))
    if pg.predictor not in (1, 2):
        raise ValueError("%s: predictor %d%s; only 1 (none) and 2 (horizontal differencing) are read here"
                         % (where, pg.predictor, " (floating point)" if pg.predictor == 3 else ""))
    plain = pg.compression == 1 and pg.predictor == 1
    if not plain and not (pg.sample_format == 1 and pg.bits in (8, 16)):
        raise ValueError("%s: compressed or differenced pages are read as 8- or 16-bit unsigned only (BitsPerSample %d, SampleFormat %d)"
                         % (where, pg.bits, pg.sample_format))
    if pg.sample_format not in (1, 2, 3) or pg.bits not in (8, 16, 32, 64):
        raise ValueError("%s: BitsPerSample %d, SampleFormat %d are not read here" % (where, pg.bits, pg.sample_format))
    if not plain and (len(pg.offsets) != pg.strips or len(pg.counts) != pg.strips):
        raise ValueError("%s: %d strip offsets and %d byte counts for %d strips" % (where, len(pg.offsets), len(pg.counts), pg.strips))


def _tiff_page_dtype(table, pg):
    return np.dtype("%s%s%d" % (table.byte_order, {1: "u", 2: "i", 3: "f"}[pg.sample_format], pg.bits // 8))


def _tiff_decode_page(table, pg):
    """Page pg as a (rows, cols) array in the FILE's byte order: strips joined (uncompressed) or inflated by zlib one by one, then
    the horizontal predictor undone on native-order samples (libtiff's order: byte swap, then accumulate)."""
    import zlib
    dtype, buf = _tiff_page_dtype(table, pg), table.buf
    if pg.compression == 1:
        raw = b"".join(buf[o:o + c] for o, c in zip(pg.offsets, pg.counts))
    else:
        parts = []
        for k, (o, c) in enumerate(zip(pg.offsets, pg.counts)):
            want = pg.strip_rows(k) * pg.cols * dtype.itemsize
            try:
                part = zlib.decompress(buf[o:o + c])
            except zlib.error as e:
                raise ValueError("%s: page %d strip %d does not inflate: %s" % (table.path, pg.index, k, e))
            if len(part) != want:
                raise ValueError("%s: page %d strip %d inflates to %d bytes, not %d" % (table.path, pg.index, k, len(part), want))
            parts.append(part)
        raw = b"".join(parts)
    plane = np.frombuffer(raw, dtype=dtype, count=pg.rows * pg.cols).reshape(pg.rows, pg.cols)
    if pg.predictor == 2:
        native = dtype.newbyteorder("=")
        plane = np.cumsum(plane.astype(native), axis=1, dtype=native).astype(dtype)
    return plane


def _tiff_checked_table(path):
    table = tiff_page_table(path)
    if not table.pages:
        raise ValueError("%s holds no image" % path)
    first = table.pages[0]
    for pg in table.pages:
        _tiff_check_page(path, pg)
        if (pg.rows, pg.cols, pg.bits, pg.sample_format) != (first.rows, first.cols, first.bits, first.sample_format):
            raise ValueError("%s: pages of different size or type" % path)
    return table


def read_tiff(path):
    """bim.py:28-51: (image, axes, shape, metadata) of a TIFF file.  Self-contained reader for what this package, ImageJ and
    tifffile's defaults write -- classic TIFF and BigTIFF, either byte order, strips of one sample per pixel: uncompressed 8 / 16 /
    32-bit unsigned, signed or float pages, or deflate (compression 8 / 32946, inflated with the standard library's zlib) 8- and
    16-bit unsigned pages, with predictor 1 or 2; pages of one size.  Anything else raises ValueError naming the tag value met."""
    table = _tiff_checked_table(path)
    pages = [_tiff_decode_page(table, pg) for pg in table.pages]
    rows, cols = pages[0].shape
    desc = table.description
    axes, shape = _tiff_axes_from_description(desc, len(pages), rows, cols)
    image = np.stack(pages).astype(pages[0].dtype.newbyteorder("=")).reshape(shape)
    metadata = dict(line.split("=", 1) for line in desc.splitlines() if "=" in line) if desc.startswith("ImageJ=") else None
    return image, axes, image.shape, metadata


class TiffSource(object):
    """A TIFF stack as a lazy image source: dims from the page table, block() decodes only the pages it is asked for.  The
    description's axes say which page holds which (t, c, z) -- TCZ, ImageJ's TZC or any other order of the page axes."""

    def __init__(self, path):
        self.table = _tiff_checked_table(path)
        first = self.table.pages[0]
        axes, shape = _tiff_axes_from_description(self.table.description, len(self.table.pages), first.rows, first.cols)
        axes = axes if axes else "TCZYX"[5 - len(shape):]
        if (len(axes) != len(shape) or any(a not in "TCZYX" for a in axes) or len(set(axes)) != len(axes) or axes[-2:] != "YX"):
            raise ValueError("axes %r do not describe an array of rank %d" % (axes, len(shape)))
        self.axes, self.shape = axes, tuple(int(v) for v in shape)
        self.page_axes, self.page_shape = axes[:-2], self.shape[:-2]
        self.dtype = _tiff_page_dtype(self.table, first).newbyteorder("=")
        self._decoded = {}            # the pages of the last block(): the chunk iterator asks for the same pages x by x, y by y

    def set_scene(self, series):
        if series != 0:
            raise IndexError("scene %d of 1" % series)

    @property
    def dims(self):
        from .basic_image_manipulations import ImageDims
        ext = dict(zip(self.axes, self.shape))
        return ImageDims(*[ext.get(a, 1) for a in "TCZYX"])

    def page_index(self, t, c, z):
        """the page that holds plane (t, c, z)"""
        at = dict(T=t, C=c, Z=z)
        k = 0
        for a, n in zip(self.page_axes, self.page_shape):
            k = k * n + at[a]
        return k

    def block(self, t, c, z, y, x):
        d = self.dims
        ts, cs, zs = (range(*s.indices(n)) if isinstance(s, slice) else [s] for s, n in zip((t, c, z), d[:3]))
        last, self._decoded = self._decoded, {}

        def plane(ti, ci, zi):
            k = self.page_index(ti, ci, zi)
            if k not in self._decoded:
                self._decoded[k] = last[k] if k in last else _tiff_decode_page(self.table, self.table.pages[k])
            return self._decoded[k]

        planes = [[[plane(ti, ci, zi)[y, x] for zi in zs] for ci in cs] for ti in ts]
        out = np.array(planes, dtype=self.dtype)
        for axis, s in reversed(list(enumerate((t, c, z)))):
            if not isinstance(s, slice):
                out = out.squeeze(axis)           # an integer index drops its axis, as on an array
        return out


# ---- the writers -----------------------------------------------------------------------------------------------------------
# An IFD is its entry count, the entries (tag, type, count, value) sorted by tag, and the offset of the next IFD (0: none).
# Per flavour, little-endian: the count's struct format, an entry's, an offset's, and the TIFF type of an offset or byte count
# (LONG, LONG8).
_CLASSIC, _BIGTIFF = ("<H", "<HHII", "<I", 4), ("<Q", "<HHQQ", "<Q", 16)


def _header(big, first_ifd):
    return struct.pack("<2sHHHQ", b"II", 43, 8, 0, first_ifd) if big else struct.pack("<2sHI", b"II", 42, first_ifd)


def _ifd_size(big, n_entries):
    count, entry, offset, _ = _BIGTIFF if big else _CLASSIC
    return struct.calcsize(count) + struct.calcsize(entry) * n_entries + struct.calcsize(offset)


def _pack_ifd(big, entries, next_ifd):
    count, entry, offset, _ = _BIGTIFF if big else _CLASSIC
    return (struct.pack(count, len(entries)) + b"".join(struct.pack(entry, *e) for e in sorted(entries))
            + struct.pack(offset, next_ifd))


def _page_tags(rows, cols, dtype, compression, rowsperstrip, predictor=1):
    """A page's entries but for where its data is (273, 279) and the description (270): min-is-black, one sample per pixel."""
    fmt = 3 if dtype.kind == "f" else (2 if dtype.kind == "i" else 1)
    tags = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, 1, dtype.itemsize * 8), (259, 3, 1, compression), (262, 3, 1, 1),
            (277, 3, 1, 1), (278, 4, 1, rowsperstrip), (339, 3, 1, fmt)]
    return tags + [(317, 3, 1, predictor)] if predictor != 1 else tags


def _description(axes, shape, xml=None):
    """Page 0's ImageDescription: "axes=... shape=...", the metadata's XML on a line of its own, NUL, padded to a word."""
    desc = ("axes=%s shape=%s" % (axes, "x".join(str(v) for v in shape))).encode("ascii")
    if xml is not None:
        desc += b"\n" + (xml if isinstance(xml, bytes) else xml.encode("utf-8", "replace"))
    desc += b"\0"
    return desc + b"\0" * (len(desc) & 1)                  # TIFF 6.0: every IFD starts on a word boundary


def _write_pages(path, big, tags, too_large, description, n_pages, pages):
    """The in-order layout of save_tiff and write_tiff_strips: the header; per page its IFD -- `tags` with 273, 279 and, on page 0,
    270 --, with more than one strip the table of strip offsets and then the table of byte counts (one strip: both inline), page
    0's description, and the strips, each padded to a word; the next IFD follows.  pages: per page the list of its finished
    strips, raw or compressed, as bytes-like objects.  A classic file that reaches 4 GiB raises ValueError(too_large)."""
    with open(path, "wb") as fh:
        at = fh.write(_header(big, 16 if big else 8))              # (the first IFD follows the header)
        for k, strips in enumerate(pages):
            at = _write_page(fh, at, big, tags, too_large, strips, description if k == 0 else b"", last=k + 1 == n_pages)


def _write_page(fh, ifd_at, big, tags, too_large, strips, description, last):
    """One page of _write_pages at file position ifd_at -> the position behind it.  Every strip is written as it is given: no copy,
    the pad byte a write of its own."""
    _, _, offset, off_type = _BIGTIFF if big else _CLASSIC
    word, n = struct.calcsize(offset), len(strips)
    sizes = [memoryview(s).nbytes for s in strips]
    tables_at = ifd_at + _ifd_size(big, len(tags) + 2 + (1 if description else 0))
    desc_at = tables_at + (2 * word * n if n > 1 else 0)
    starts, at = [], desc_at + len(description)
    for size in sizes:
        starts.append(at)
        at += size + (size & 1)
    if not big and at >= 2 ** 32:
        raise ValueError(too_large)
    entries = tags + [(273, off_type, n, tables_at if n > 1 else starts[0]), (279, off_type, n, tables_at + word * n if n > 1 else sizes[0])]
    if description:
        entries.append((270, 2, len(description), desc_at))
    fh.write(_pack_ifd(big, entries, 0 if last else at))
    if n > 1:
        fh.write(b"".join(struct.pack(offset, v) for v in starts + sizes))
    fh.write(description)
    for s, size in zip(strips, sizes):
        fh.write(s)
        if size & 1:
            fh.write(b"\0")
    return at


def tiff_normalise(image, data_type=""):
    """The conversion save_tiff applies before writing (bim.py:183-186): images that are not already of the requested
    unsigned type are scaled so that their maximum becomes the type's maximum, and rounded."""
    image = np.asarray(image)
    if data_type and image.dtype != data_type and data_type in ('uint8', 'uint16'):
        top = 255 if data_type == 'uint8' else 65535
        image = np.round((image / np.max(image)) * top).astype(data_type)
    return image


def metadata_xml(metadata, who="save_tiff"):
    """What of `metadata` rides in the description: upstream hands the OME metadata to aicsimageio's writer; here its XML (if it
    has one) or the string itself; other objects are reported once as not written."""
    if metadata is None:
        return None
    xml = metadata.to_xml() if hasattr(metadata, "to_xml") else (metadata if isinstance(metadata, (str, bytes)) else None)
    if xml is None:
        import warnings
        warnings.warn("%s: metadata of type %s is not written (no OME-XML writer here)" % (who, type(metadata).__name__))
    return xml


def save_tiff(path, image, metadata=None, axes="", data_type="", compression=None, predictor=1, rowsperstrip=None):
    """bim.py:160-188.  Upstream hands the array to aicsimageio's OME-TIFF writer; here a self-contained baseline TIFF
    writer stores every (Y, X) plane of the normalised array as one page (little-endian, uncompressed, min-is-black) with
    the axes string and shape in the first page's ImageDescription -- what ImageJ / tifffile / the reference's read_tiff
    open as a stack.  `metadata` with a to_xml() method (or a string) is appended to that description; other objects are
    reported once as not written.

    compression="zlib" (opt-in; uint8 / uint16 only) writes every page as deflate strips instead (Compression 8, host zlib, one
    stream per strip of `rowsperstrip` rows -- by default about 64 KB of raw data) with predictor 1 or 2 (horizontal
    differencing).  Without these arguments the file is byte for byte what it always was."""
    if compression not in (None, "zlib"):
        raise ValueError("save_tiff: compression %r (None or 'zlib')" % (compression,))
    if compression is None and (predictor != 1 or rowsperstrip is not None):
        raise ValueError("save_tiff: predictor and rowsperstrip belong to compression='zlib'")
    if predictor not in (1, 2):
        raise ValueError("save_tiff: predictor %r (1: none, 2: horizontal differencing)" % (predictor,))
    image = tiff_normalise(image, data_type)
    if image.dtype == np.float64:
        image = image.astype(np.float32)
    if image.dtype not in (np.uint8, np.uint16, np.float32, np.int32):
        raise TypeError("save_tiff writes uint8 / uint16 / int32 / float32 pages (got %s)" % image.dtype)
    if image.ndim < 2:
        raise ValueError("save_tiff needs at least a 2-D image")
    planes = np.ascontiguousarray(image).reshape((-1,) + image.shape[-2:]).astype(image.dtype.newbyteorder("<"))
    n_pages, rows, cols = planes.shape
    desc = _description(axes, image.shape, metadata_xml(metadata))
    too_large = "save_tiff: classic TIFF holds less than 4 GiB; split the movie"
    if compression == "zlib":
        if planes.dtype not in (np.uint8, np.uint16):
            raise TypeError("save_tiff: compression='zlib' writes uint8 / uint16 pages (got %s)" % planes.dtype)
        if rowsperstrip is None:
            rowsperstrip = default_rows_per_strip(rows, cols * planes.dtype.itemsize)
        if int(rowsperstrip) < 1:
            raise ValueError("save_tiff: rowsperstrip %d" % rowsperstrip)
        geometry = StripGeometry(rows, rowsperstrip)
        tags = _page_tags(rows, cols, planes.dtype, 8, geometry.rows_per_strip, predictor)
        return _write_pages(path, False, tags, too_large, desc, n_pages, _zlib_pages(planes, predictor, geometry))
    if planes.nbytes + n_pages * 256 + len(desc) >= 2 ** 32:      # (before the file is opened)
        raise ValueError(too_large)
    tags = _page_tags(rows, cols, planes.dtype, 1, rows)
    return _write_pages(path, False, tags, too_large, desc, n_pages, ([plane] for plane in planes))


def _zlib_pages(planes, predictor, geometry):
    """save_tiff's deflate form: per page the list of its strips' zlib streams (level 6), differenced first for predictor 2."""
    import os
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    n_pages, rows = planes.shape[:2]
    rps, n_strips = geometry.rows_per_strip, geometry.strips
    threads = max(1, min(16, os.cpu_count() or 1))
    ahead = max(1, threads // n_strips)

    def page_strips(k):
        plane = planes[k]
        if predictor == 2:
            plane = np.concatenate([plane[:, :1], np.diff(plane, axis=1)], axis=1).astype(planes.dtype)      # modulo 2^bits
        return [plane[r:r + rps] for r in range(0, rows, rps)]

    # (zlib releases the interpreter lock: the strips of a few pages are compressed side by side; the file does not depend on it)
    with ThreadPoolExecutor(threads) as pool:
        for k in range(0, n_pages, ahead):
            raw = [part for j in range(k, min(n_pages, k + ahead)) for part in page_strips(j)]
            out = list(pool.map(lambda part: zlib.compress(part.tobytes(), 6), raw))
            for i in range(0, len(out), n_strips):
                yield out[i:i + n_strips]


def write_tiff_strips(path, shape, axes, dtype, rowsperstrip, pages, bigtiff=None, predictor=1, xml=None):
    """A deflate-strip TIFF from strips that are compressed ALREADY (movie.export_tiff: zlib streams made on the GPUs).  shape: the
    whole array's, (..., Y, X), every leading index one page in C order; dtype uint8 or uint16; `pages` yields, per page, the list
    of its finished strip streams (one per `rowsperstrip` rows, the last strip the rows that are left).  Pages are written as they
    arrive; nothing but the current page is held.

    The layout is save_tiff(compression="zlib")'s: little-endian, Compression 8, no Predictor tag, per page the strip offsets and
    byte counts behind the IFD (inline for one strip), then the strips on word boundaries; "axes=... shape=..." in page 0's
    ImageDescription.  predictor=2: the strips hold rows differenced along x modulo 2^bits (the caller's work) and every page says so
    in tag 317; xml: a string that follows the description's first line, as save_tiff's metadata does.  bigtiff=True writes BigTIFF
    (magic 43, 8-byte offsets and counts); None chooses it when the classic form would reach 4 GiB -- from the strips themselves when `pages` is a list, otherwise, the sizes not being known before the first
    page is written, from the uncompressed size.  A classic file that reaches 4 GiB after all raises ValueError."""
    dtype = np.dtype(dtype)
    if dtype not in (np.uint8, np.uint16):
        raise TypeError("write_tiff_strips writes uint8 / uint16 pages (got %s)" % dtype)
    shape = tuple(int(v) for v in shape)
    if len(shape) < 2 or min(shape) < 1:
        raise ValueError("write_tiff_strips needs a shape (..., Y, X) of positive extents, not %r" % (shape,))
    rows, cols = shape[-2:]
    n_pages = int(np.prod(shape[:-2], dtype=np.int64))
    if int(rowsperstrip) < 1:
        raise ValueError("write_tiff_strips: rowsperstrip %d" % rowsperstrip)
    if predictor not in (1, 2):
        raise ValueError("write_tiff_strips: predictor %r (1: none, 2: horizontal differencing)" % (predictor,))
    geometry = StripGeometry(rows, rowsperstrip)
    n_strips = geometry.strips
    desc = _description(axes, shape, xml)
    if bigtiff is None:
        if isinstance(pages, (list, tuple)):
            payload = sum(len(s) + (len(s) & 1) for page in pages for s in page)
        else:
            payload = n_pages * rows * cols * dtype.itemsize
        bigtiff = payload + len(desc) + 16 + n_pages * (16 + 20 * (11 if predictor == 1 else 12) + 16 * n_strips) >= 2 ** 32      # (the larger form's tables)

    def checked():
        written = 0
        for k, strips in enumerate(pages):
            if k >= n_pages:
                raise ValueError("write_tiff_strips: more than the %d pages of shape %r" % (n_pages, shape))
            strips = list(strips)
            if len(strips) != n_strips:
                raise ValueError("write_tiff_strips: page %d came with %d strips, not %d" % (k, len(strips), n_strips))
            yield strips
            written += 1
        if written != n_pages:
            raise ValueError("write_tiff_strips: %d pages arrived for shape %r (%d pages)" % (written, shape, n_pages))

    _write_pages(path, bool(bigtiff), _page_tags(rows, cols, dtype, 8, geometry.rows_per_strip, predictor),
                 "write_tiff_strips: classic TIFF holds less than 4 GiB; pass bigtiff=True", desc, n_pages, checked())
    return path


class BigTiffAppender(object):
    """Streaming BigTIFF writer (magic 43, 8-byte offsets): every (Y, X) plane appended becomes one page -- uncompressed,
    min-is-black, one strip -- so a movie larger than memory (or than classic TIFF's 4 GiB) can be written frame by frame.  The
    number of pages is not known when a page is written: its data comes first, its IFD behind it, and the previous IFD's link
    (the header's, for page 0) is patched to point there."""

    def __init__(self, path):
        self.fh = open(path, "wb")
        self.fh.write(_header(True, 0))                                # the first-IFD offset (bytes 8..15) is patched later
        self.link = 8                                                  # file position of the pointer to the next IFD

    def write_plane(self, plane):
        plane = np.ascontiguousarray(plane)
        if plane.ndim != 2 or plane.dtype not in (np.uint8, np.uint16, np.float32, np.int32):
            raise TypeError("BigTIFF pages are 2-D uint8 / uint16 / int32 / float32 planes (got %s %s)" % (plane.dtype, plane.shape))
        rows, cols = plane.shape
        raw = plane.astype(plane.dtype.newbyteorder("<")).tobytes()
        at = self.fh.seek(0, 2)
        at += (-at) % 8
        self.fh.seek(at)
        self.fh.write(raw)
        ifd = at + len(raw)
        ifd += (-ifd) % 8
        entries = _page_tags(rows, cols, plane.dtype, 1, rows) + [(273, 16, 1, at), (279, 16, 1, len(raw))]
        self.fh.seek(ifd)
        self.fh.write(_pack_ifd(True, entries, 0))
        self.fh.seek(self.link)
        self.fh.write(struct.pack(_BIGTIFF[2], ifd))
        self.link = ifd + _ifd_size(True, len(entries)) - 8

    def close(self):
        self.fh.close()
