"""Restatement of tip_deflate_strips' framing in plain Python, for its tests: the pages of a TIFF cut into strips, every strip a
zlib stream (RFC 1950) of its own,

    78 01 || body || 01 00 00 FF FF || Adler-32 of the strip (most significant byte first)

with body = deflate_rows_restate.deflate_rows(strip alone, e, row_bytes) (codes "fixed") or
deflate_dynamic_restate.deflate_dynamic(strip alone, e, row_bytes) (codes "dynamic"): the strip is the WHOLE buffer of the body's
rule, so no match reaches before it, and the body ends in a byte-aligned non-final block, which the final empty stored block
closes.  78: deflate with a 32 KB window; 01: no dictionary, compression level 0, and 0x7801 is a multiple of 31.  A strip holds
at most 65536 bytes: one chunk of the body's rule.

Compacted (what the device entries write): the streams in page-major order, every one at an even offset -- one zero byte behind a
stream of odd size --, with the table of (offset, size) per strip, the size without the pad byte, and the total with the pads.
Bound: per strip of n bytes 2 + deflate_restate.chunk_bound(n) + 9, made even.
"""
import zlib

import numpy as np

import deflate_dynamic_restate as dd
import deflate_restate as dr
import deflate_rows_restate as rr

CODES = ("fixed", "dynamic")
HEAD = b"\x78\x01"
MAX_STRIP = dr.CHUNK


def strip_stream(strip, e, row_bytes, codes):
    strip = bytes(strip)
    assert codes in CODES and 0 < len(strip) <= MAX_STRIP
    body = rr.deflate_rows(strip, e, row_bytes) if codes == "fixed" else dd.deflate_dynamic(strip, e, row_bytes)
    return HEAD + body + dr.final_block() + zlib.adler32(strip).to_bytes(4, "big")


def raw_strips(pages, rows_per_strip):
    """pages: array (n_pages, rows, cols) of uint8 or uint16 -> per page the list of its strips' raw bytes"""
    pages = np.ascontiguousarray(pages)
    return [[page[r:r + rows_per_strip].tobytes() for r in range(0, pages.shape[1], rows_per_strip)] for page in pages]


def deflate_strips(pages, rows_per_strip, codes):
    """-> per page the list of its strips' zlib streams"""
    pages = np.ascontiguousarray(pages)
    e, row_bytes = pages.dtype.itemsize, pages.shape[2] * pages.dtype.itemsize
    return [[strip_stream(s, e, row_bytes, codes) for s in page] for page in raw_strips(pages, rows_per_strip)]


def compact(streams):
    """per page lists of streams -> (the compacted bytes, [(offset, size)] in page-major order)"""
    out, table = bytearray(), []
    for page in streams:
        for s in page:
            table.append((len(out), len(s)))
            out += s + b"\0" * (len(s) & 1)
    return bytes(out), table


def strip_bound(n):
    return (2 + dr.chunk_bound(n) + 9 + 1) & ~1


def bound(n_pages, rows, row_bytes, rows_per_strip):
    full, rest = divmod(rows, rows_per_strip)
    return n_pages * (full * strip_bound(rows_per_strip * row_bytes) + (strip_bound(rest * row_bytes) if rest else 0))
