"""The deflate encoder of csrc/tip_deflate.hip (runs, or runs and matches to the row above; fixed or per-chunk dynamic codes) from Python, and what turns its output into a `.npy` archive member:
the CRC-32 of a concatenation from the parts' CRCs, and the member builder that puts the array header in front as a stored
block and closes the stream.  Nothing here inflates or deflates on the host."""
import ctypes
import zlib

import numpy as np

from . import _lib

CRC_POLY = 0xEDB88320            # the zip / zlib CRC-32's polynomial, reflected: bit 31 is x^0, bit 0 is x^31
FINAL_BLOCK = b"\x01\x00\x00\xff\xff"      # an empty stored block with BFINAL set: closes a stream of non-final blocks


def _gf_mul(a, b):
    """a * b in GF(2)[x] / P, reflected representation: for every term x^i of a add b * x^i; b * x shifts towards bit 0 and
    the x^32 that falls out is replaced by the polynomial's lower terms."""
    p = 0
    for i in range(32):
        if (a >> (31 - i)) & 1:
            p ^= b
        b = (b >> 1) ^ (CRC_POLY if b & 1 else 0)
    return p


def _x_pow_8n(n):
    """x^(8 n) by square and multiply"""
    p, sq = 1 << 31, 1 << 30          # x^0, x^1
    for _ in range(3):
        sq = _gf_mul(sq, sq)          # x^8
    while n:
        if n & 1:
            p = _gf_mul(sq, p)
        sq = _gf_mul(sq, sq)
        n >>= 1
    return p


def crc32_combine(crc_a, crc_b, len_b):
    """zlib.crc32(A + B) from zlib.crc32(A), zlib.crc32(B) and len(B).  From the definition, with J the all-ones word that is
    both the register's initial value and the final XOR: crc(M) = M(x) x^32 + J x^(8 |M|) + J (mod P).  Then
    crc(A) x^(8 |B|) + crc(B) = A(x) x^(32 + 8 |B|) + B(x) x^32 + J x^(8 |A| + 8 |B|) + J + (J + J) x^(8 |B|), and that is
    crc(A + B): A's CRC extended by |B| zero bytes, plus B's -- the two J x^(8 |B|) cancel because the two constants are equal."""
    return _gf_mul(int(crc_a) & 0xFFFFFFFF, _x_pow_8n(int(len_b))) ^ (int(crc_b) & 0xFFFFFFFF)


def runs_bound(nbytes):
    """tip_deflate_runs_bound: the most bytes the encoder writes for nbytes of input (no device needed)."""
    out = ctypes.c_int64(0)
    _lib.check(_lib.load().tip_deflate_runs_bound(int(nbytes), ctypes.byref(out)))
    return int(out.value)


def deflate_runs_dev(src_ptr, nbytes, elem_bytes, dst_ptr, cap):
    """tip_deflate_runs_dev on device addresses -> (stream bytes written at dst_ptr, CRC-32 of the input); waits once."""
    size, crc = ctypes.c_int64(0), ctypes.c_uint32(0)
    _lib.check(_lib.lib().tip_deflate_runs_dev(src_ptr, int(nbytes), int(elem_bytes), dst_ptr, int(cap), ctypes.byref(size),
                                               ctypes.byref(crc)))
    return int(size.value), int(crc.value)


def deflate_rows_dev(src_ptr, nbytes, elem_bytes, row_bytes, dst_ptr, cap):
    """tip_deflate_rows_dev on device addresses: deflate_runs_dev with matches to the row above, row_bytes the map's row length."""
    size, crc = ctypes.c_int64(0), ctypes.c_uint32(0)
    _lib.check(_lib.lib().tip_deflate_rows_dev(src_ptr, int(nbytes), int(elem_bytes), int(row_bytes), dst_ptr, int(cap),
                                               ctypes.byref(size), ctypes.byref(crc)))
    return int(size.value), int(crc.value)


def deflate_dynamic_dev(src_ptr, nbytes, elem_bytes, row_bytes, dst_ptr, cap):
    """tip_deflate_dynamic_dev on device addresses: the tokens of deflate_rows_dev (row_bytes > 0) or deflate_runs_dev (row_bytes 0 or
    None), every chunk in a dynamic-Huffman block of its own codes where that is fewer bytes than the fixed block."""
    size, crc = ctypes.c_int64(0), ctypes.c_uint32(0)
    _lib.check(_lib.lib().tip_deflate_dynamic_dev(src_ptr, int(nbytes), int(elem_bytes), int(row_bytes or 0), dst_ptr, int(cap),
                                                  ctypes.byref(size), ctypes.byref(crc)))
    return int(size.value), int(crc.value)


def _deflate_host(data, elem_bytes, row_bytes, dynamic=False):
    src = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).view(np.uint8).ravel()
    cap = runs_bound(src.size)
    dst = np.empty(max(cap, 1), np.uint8)
    keep = src if src.size else np.zeros(1, np.uint8)      # (an empty array has no address to hand over)
    size, crc = ctypes.c_int64(0), ctypes.c_uint32(0)
    if dynamic:
        rc = _lib.lib().tip_deflate_dynamic(_lib.ptr(keep), src.size, int(elem_bytes), int(row_bytes or 0), _lib.ptr(dst), cap,
                                            ctypes.byref(size), ctypes.byref(crc))
    elif row_bytes is None:
        rc = _lib.lib().tip_deflate_runs(_lib.ptr(keep), src.size, int(elem_bytes), _lib.ptr(dst), cap, ctypes.byref(size), ctypes.byref(crc))
    else:
        rc = _lib.lib().tip_deflate_rows(_lib.ptr(keep), src.size, int(elem_bytes), int(row_bytes), _lib.ptr(dst), cap, ctypes.byref(size),
                                         ctypes.byref(crc))
    _lib.check(rc)
    return dst[:size.value].tobytes(), int(crc.value)


def deflate_runs(data, elem_bytes):
    """tip_deflate_runs on a host buffer (bytes or a C-contiguous array) -> (stream, CRC-32 of the input)."""
    return _deflate_host(data, elem_bytes, None)


def deflate_rows(data, elem_bytes, row_bytes):
    """tip_deflate_rows on a host buffer: deflate_runs with matches to the row above, row_bytes the map's row length."""
    return _deflate_host(data, elem_bytes, row_bytes)


def deflate_dynamic(data, elem_bytes, row_bytes=None):
    """tip_deflate_dynamic on a host buffer: deflate_rows' tokens (deflate_runs' with row_bytes None or 0) under per-chunk dynamic codes."""
    return _deflate_host(data, elem_bytes, row_bytes, dynamic=True)


STRIP_CODES = {"fixed": 0, "dynamic": 1}      # tip_deflate_strips' `codes`


def strip_codes(codes):
    """"fixed" / "dynamic" (or 0 / 1) -> tip_deflate_strips' `codes`"""
    if codes in STRIP_CODES:
        return STRIP_CODES[codes]
    if codes in (0, 1) and not isinstance(codes, bool):
        return int(codes)
    raise ValueError("codes must be 'fixed' or 'dynamic', not %r" % (codes,))


def strips_bound(n_pages, rows, row_bytes, rows_per_strip):
    """tip_deflate_strips_bound: the most bytes the strip encoder writes for these pages (no device needed)."""
    out = ctypes.c_int64(0)
    _lib.check(_lib.load().tip_deflate_strips_bound(int(n_pages), int(rows), int(row_bytes), int(rows_per_strip), ctypes.byref(out)))
    return int(out.value)


def deflate_strips_dev(src_ptr, n_pages, rows, row_bytes, elem_bytes, rows_per_strip, codes, dst_ptr, cap):
    """tip_deflate_strips_dev on device addresses: every strip of every page as a zlib stream of its own, compacted at dst_ptr ->
    (table: int64 (strips, 2) of (offset, size) in page-major order, bytes written); waits once."""
    n_strips = int(n_pages) * -(-int(rows) // max(1, int(rows_per_strip)))
    table, total = np.zeros((max(n_strips, 1), 2), np.int64), ctypes.c_int64(0)
    _lib.check(_lib.lib().tip_deflate_strips_dev(src_ptr, int(n_pages), int(rows), int(row_bytes), int(elem_bytes), int(rows_per_strip),
                                                 strip_codes(codes), dst_ptr, int(cap), _lib.ptr(table), ctypes.byref(total)))
    return table[:n_strips], int(total.value)


def deflate_strips(pages, rows_per_strip, codes="dynamic"):
    """tip_deflate_strips on a host array of uint8 or uint16 pages (..., rows, cols) -> per page the list of its strips' zlib streams."""
    pages = np.ascontiguousarray(pages)
    if pages.ndim < 2 or pages.dtype.itemsize not in (1, 2):
        raise ValueError("deflate_strips takes 8- or 16-bit pages (..., rows, cols), not %s %s" % (pages.dtype, pages.shape))
    rows, cols = pages.shape[-2:]
    n_pages = int(np.prod(pages.shape[:-2], dtype=np.int64))
    item = pages.dtype.itemsize
    cap = strips_bound(n_pages, rows, cols * item, rows_per_strip)
    n_strips = n_pages * -(-rows // int(rows_per_strip))
    dst, table, total = np.empty(max(cap, 1), np.uint8), np.zeros((max(n_strips, 1), 2), np.int64), ctypes.c_int64(0)
    keep = pages if pages.size else np.zeros(1, np.uint8)      # (an empty array has no address to hand over)
    _lib.check(_lib.lib().tip_deflate_strips(_lib.ptr(keep), n_pages, rows, cols * item, item, int(rows_per_strip), strip_codes(codes),
                                             _lib.ptr(dst), cap, _lib.ptr(table), ctypes.byref(total)))
    return split_strips(dst[:total.value], table[:n_strips], n_pages)


def split_strips(stream, table, n_pages):
    """The compacted streams of deflate_strips_dev cut by its table -> per page the list of its strips' bytes."""
    per_page = len(table) // n_pages if n_pages else 0
    buf = memoryview(np.ascontiguousarray(stream, np.uint8)).cast("B")
    return [[bytes(buf[int(o):int(o) + int(n)]) for o, n in table[k * per_page:(k + 1) * per_page]] for k in range(n_pages)]


def export_maps_u16_dev(labels_ptr, types_ptr, n_pix, ids, out_ptr):
    """tip_export_maps_u16_dev on device addresses: the uint16 page of tracking labels ids[labels - 1] (0 on label 0) at out_ptr and,
    with types_ptr, the page of remapped types (0 -> 2, 255 -> 0) behind it.  ValueError for an id outside [0, 65535] and for a
    label outside [0, len(ids)]."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n_bad = ctypes.c_int32(0)
    keep = ids if ids.size else np.zeros(1, np.int64)
    _lib.check(_lib.lib().tip_export_maps_u16_dev(labels_ptr, types_ptr, int(n_pix), _lib.ptr(keep), ids.size, out_ptr, ctypes.byref(n_bad)))
    if n_bad.value:
        raise ValueError("%d pixels hold a label outside [0, %d]: the ids do not belong to this label map" % (n_bad.value, ids.size))
    return out_ptr


def max_f64_dev(src_ptr, n):
    """tip_max_f64_dev: the maximum of n float64 at a device address (waits once); a NaN is never taken."""
    out = ctypes.c_double(0.0)
    _lib.check(_lib.lib().tip_max_f64_dev(src_ptr, int(n), ctypes.byref(out)))
    return float(out.value)


def max_f64(values):
    """tip_max_f64, the host twin of max_f64_dev (no device needed)."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    out = ctypes.c_double(0.0)
    keep = values if values.size else np.zeros(1)
    _lib.check(_lib.load().tip_max_f64(_lib.ptr(keep), values.size, ctypes.byref(out)))
    return float(out.value)


def projection_pages_u16_dev(src_ptr, n_pages, rows, cols, scale_max, predictor, out_ptr):
    """tip_projection_pages_u16_dev on device addresses, asynchronous: float64 pages as the uint16 pages of
    tiff.tiff_normalise(movie, "uint16") when scale_max is the movie's maximum, differenced along x for predictor 2."""
    _lib.check(_lib.lib().tip_projection_pages_u16_dev(src_ptr, int(n_pages), int(rows), int(cols), float(scale_max), int(predictor), out_ptr))
    return out_ptr


def projection_pages_u16(planes, scale_max, predictor=1):
    """tip_projection_pages_u16, the host twin (no device needed), on a float64 array (..., rows, cols) -> uint16 of its shape."""
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    if planes.ndim < 2:
        raise ValueError("projection_pages_u16 takes pages (..., rows, cols), not %s" % (planes.shape,))
    rows, cols = planes.shape[-2:]
    out = np.zeros(planes.shape, np.uint16)
    keep, keep_out = (planes, out) if planes.size else (np.zeros(1), np.zeros(1, np.uint16))
    _lib.check(_lib.load().tip_projection_pages_u16(_lib.ptr(keep), int(np.prod(planes.shape[:-2], dtype=np.int64)), rows, cols,
                                                    float(scale_max), int(predictor), _lib.ptr(keep_out)))
    return out


def zmap_u16_dev(src_ptr, n, out_ptr):
    """tip_zmap_u16_dev on device addresses, asynchronous: n int64 as uint16, modulo 2^16."""
    _lib.check(_lib.lib().tip_zmap_u16_dev(src_ptr, int(n), out_ptr))
    return out_ptr


def zmap_u16(zmap):
    """tip_zmap_u16, the host twin (no device needed): an int64 array -> uint16 of its shape."""
    zmap = np.ascontiguousarray(zmap, dtype=np.int64)
    out = np.zeros(zmap.shape, np.uint16)
    if zmap.size:
        _lib.check(_lib.load().tip_zmap_u16(_lib.ptr(zmap), zmap.size, _lib.ptr(out)))
    return out


def npy_header(shape, dtype):
    """The bytes np.save writes in front of a C-contiguous array's data (format 1.0: magic, header length, dict, padding)."""
    import io
    buf = io.BytesIO()
    np.lib.format.write_array_header_1_0(buf, dict(shape=tuple(int(s) for s in shape), fortran_order=False,
                                                   descr=np.lib.format.dtype_to_descr(np.dtype(dtype))))
    return buf.getvalue()


def stored_block(payload):
    """A non-final stored block (BFINAL 0, BTYPE 00, padding, LEN, NLEN, the bytes): byte-aligned, so it goes in front of any
    byte-aligned stream."""
    n = len(payload)
    if n > 0xFFFF:
        raise ValueError("a stored block holds at most 65535 bytes (got %d)" % n)
    return b"\x00" + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + bytes(payload)


def npy_member(array_header_bytes, stream, crc, nbytes):
    """A whole `.npy` archive member from the encoder's output: (raw deflate stream, CRC-32, uncompressed size) of
    array_header_bytes + data, where `stream` is the encoder's stream of the nbytes of data and `crc` their CRC-32.  The header
    goes in front as a stored block, the final empty block behind; the CRCs are combined, no byte of the data is touched."""
    raw = stored_block(array_header_bytes) + bytes(stream) + FINAL_BLOCK
    return raw, crc32_combine(zlib.crc32(array_header_bytes), crc, nbytes), len(array_header_bytes) + int(nbytes)
