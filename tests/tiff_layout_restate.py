"""The TIFF files this package writes, restated from their documented layouts as flat functions that return a file's bytes.
Nothing of the package is imported: the tests compare what the writers put on disk with these, byte for byte.

Little-endian throughout.  An IFD entry is (tag, type, count, value): "<HHII" in a classic file (magic 42, 4-byte offsets), "<HHQQ"
in BigTIFF (magic 43, 8-byte offsets).  Types: 2 ASCII, 3 SHORT, 4 LONG, 16 LONG8."""
import struct


def _description(axes, shape):
    desc = ("axes=%s shape=%s" % (axes, "x".join(str(v) for v in shape))).encode("ascii") + b"\0"
    return desc + b"\0" * (len(desc) & 1)


def _sample_format(dtype):
    return {"u": 1, "i": 2, "f": 3}[dtype.kind]


def baseline_file(image, axes):
    """The uncompressed file save_tiff has always written: an 8-byte header; per (Y, X) plane an IFD of the sorted entries 256,
    257, 258, 259, 262, (270 on the first page,) 273, 277, 278, 279, 339, the next IFD's offset, the first page's description
    "axes=... shape=..." (NUL-terminated, padded to a word), the plane's little-endian samples as one strip, and a pad byte after
    an odd-sized plane."""
    planes = image.reshape((-1,) + image.shape[-2:]).astype(image.dtype.newbyteorder("<"))
    rows, cols = planes.shape[1:]
    item = planes.dtype.itemsize
    desc = _description(axes, image.shape)
    out, at = struct.pack("<2sHI", b"II", 42, 8), 8
    for k in range(len(planes)):
        extra = desc if k == 0 else b""
        n = 11 if extra else 10
        data_at = at + 2 + 12 * n + 4 + len(extra)
        size = rows * cols * item
        ent = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, 1, item * 8), (259, 3, 1, 1), (262, 3, 1, 1)]
        ent += [(270, 2, len(extra), at + 2 + 12 * n + 4)] if extra else []
        ent += [(273, 4, 1, data_at), (277, 3, 1, 1), (278, 4, 1, rows), (279, 4, 1, size), (339, 3, 1, _sample_format(planes.dtype))]
        nxt = data_at + size + (size & 1) if k + 1 < len(planes) else 0
        out += struct.pack("<H", n) + b"".join(struct.pack("<HHII", *e) for e in ent) + struct.pack("<I", nxt)
        out += extra + planes[k].tobytes() + b"\0" * (size & 1)
        at = nxt
    return out


def strip_file(shape, axes, dtype, rowsperstrip, pages, predictor=None, bigtiff=False):
    """A deflate-strip file (Compression 8) of write_tiff_strips / save_tiff(compression="zlib").  shape (..., Y, X), every leading
    index one page; pages: per page the list of its strips' bytes, taken as they are; predictor: the value of a Predictor entry
    (317), None for no entry.  Per page: the IFD -- sorted entries 256, 257, 258, 259, 262, (270 on page 0,) 273, 277, 278, 279,
    (317,) 339 --, the next IFD's offset; with more than one strip the table of strip offsets and then the table of byte counts
    (with one strip both values sit in their entries); page 0's description; the strips, a pad byte behind every odd-sized one.
    RowsPerStrip is clamped to the page's rows.  Offsets and counts are LONG in a classic file, LONG8 in BigTIFF."""
    rows, cols = shape[-2:]
    bits = 8 * dtype.itemsize
    rps = min(rowsperstrip, rows)
    if bigtiff:
        out, count, entry, word, off_type = struct.pack("<2sHHHQ", b"II", 43, 8, 0, 16), "<Q", "<HHQQ", "<Q", 16
    else:
        out, count, entry, word, off_type = struct.pack("<2sHI", b"II", 42, 8), "<H", "<HHII", "<I", 4
    w = struct.calcsize(word)
    desc = _description(axes, shape)
    for k, strips in enumerate(pages):
        n = len(strips)
        extra = desc if k == 0 else b""
        n_ent = 10 + (1 if extra else 0) + (0 if predictor is None else 1)
        ifd_at = len(out)
        tables_at = ifd_at + struct.calcsize(count) + struct.calcsize(entry) * n_ent + w
        extra_at = tables_at + (2 * w * n if n > 1 else 0)
        starts, at = [], extra_at + len(extra)
        for s in strips:
            starts.append(at)
            at += len(s) + (len(s) & 1)
        sizes = [len(s) for s in strips]
        ent = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, 1, bits), (259, 3, 1, 8), (262, 3, 1, 1)]
        ent += [(270, 2, len(extra), extra_at)] if extra else []
        ent += [(273, off_type, n, tables_at if n > 1 else starts[0]), (277, 3, 1, 1), (278, 4, 1, rps),
                (279, off_type, n, tables_at + w * n if n > 1 else sizes[0])]
        ent += [] if predictor is None else [(317, 3, 1, predictor)]
        ent += [(339, 3, 1, 1)]
        assert len(ent) == n_ent
        out += struct.pack(count, n_ent) + b"".join(struct.pack(entry, *e) for e in ent)
        out += struct.pack(word, at if k + 1 < len(pages) else 0)
        if n > 1:
            out += b"".join(struct.pack(word, v) for v in starts) + b"".join(struct.pack(word, v) for v in sizes)
        out += extra
        for s in strips:
            out += bytes(s) + b"\0" * (len(s) & 1)
        assert len(out) == at
    return out


def appended_bigtiff(planes):
    """The BigTIFF virtually_concatenate_time_points streams: a 16-byte header whose first-IFD offset points at page 0's IFD; per
    (Y, X) plane its little-endian samples as one uncompressed strip starting on an 8-byte boundary, then -- again on an 8-byte
    boundary -- the IFD: the entries 256, 257, 258, 259, 262, 273 (LONG8), 277, 278, 279 (LONG8), 339 and the next IFD's offset, 0 on
    the last page.  No description.  The gaps are zero bytes; nothing follows the last IFD."""
    ifds, body, at = [], b"", 16                                # (`at`: the file position behind the header and `body`)
    for p in planes:
        raw = p.astype(p.dtype.newbyteorder("<")).tobytes()
        body += b"\0" * ((-at) % 8)
        at += (-at) % 8
        data_at = at
        body += raw
        at += len(raw)
        body += b"\0" * ((-at) % 8)
        at += (-at) % 8
        ifds.append(at)
        rows, cols = p.shape
        ent = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, 1, 8 * p.dtype.itemsize), (259, 3, 1, 1), (262, 3, 1, 1),
               (273, 16, 1, data_at), (277, 3, 1, 1), (278, 4, 1, rows), (279, 16, 1, len(raw)), (339, 3, 1, _sample_format(p.dtype))]
        body += struct.pack("<Q", len(ent)) + b"".join(struct.pack("<HHQQ", *e) for e in ent) + struct.pack("<Q", 0)
        at += 8 + 20 * len(ent) + 8
    body = bytearray(body)
    for ifd_at, nxt in zip(ifds, ifds[1:]):                     # every IFD's last 8 bytes name the IFD behind it
        link = ifd_at - 16 + 8 + 20 * 10
        body[link:link + 8] = struct.pack("<Q", nxt)
    return struct.pack("<2sHHHQ", b"II", 43, 8, 0, ifds[0] if ifds else 0) + bytes(body)
