"""Restatement of the "rows" token rule of csrc/tip_deflate.hip in plain Python, for its tests: the run-only rule of
tests/deflate_restate.py plus matches to the row above, written from RFC 1951 and the rule below, independent of the device
code.  deflate_rows(data, e, row_bytes) is byte for byte what tip_deflate_rows(_dev) must produce.

Framing, literal code, length code, bound: deflate_restate's, unchanged (chunks of 65536 bytes, one fixed-Huffman block and
one empty stored block each, segments of 256 bytes which no token crosses).

Token rule.  e = elem_bytes, P = row_bytes (a positive multiple of e, which need not divide the buffer); positions p are byte
offsets into the WHOLE buffer, multiples of e.

    R(p)      the element at p equals the element at p - e, and p is not the first byte of its chunk
    M_d(p)    p >= d and the element at p equals the element at p - d, for the candidate distances d = P, P + e, P - e (in this
              order) of which only those with e < d <= 32768 are kept; a match may reach into an earlier chunk, never before
              the buffer's first byte

At p, with lim bytes left in the segment: r = bytes of consecutive elements from p with R (at most lim), u_d the same for M_d,
(u, d*) the longest u_d, a tie going to the earlier candidate.

    u >= max(4, e) and u > r     one match (length u, distance d*), advance u
    else r >= max(3, e)          one match (length r, distance e), advance r
    else                         the element's e literals, advance e

A match is the length symbol and its extra bits, the 5-bit distance code (most significant bit first) and the distance code's
extra bits (least significant bit first): at most 8 + 5 + 5 + 13 = 31 bits for at least 4 bytes, so nine bits per input byte
stays the worst case.  With no candidate kept (P > 32768 + e) the rule is the run-only rule.
"""
import numpy as np

import deflate_restate as dr

_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def distance_bits(dist):
    """(value, bit count) of a distance 1 .. 32768: the 5-bit code (RFC 1951 3.2.5, packed from its most significant bit) and
    its extra bits behind it."""
    assert 1 <= dist <= 32768
    code = max(k for k in range(30) if _DIST_BASE[k] <= dist)
    return dr._rev(code, 5) | ((dist - _DIST_BASE[code]) << 5), 5 + _DIST_EXTRA[code]


def match_bits(length, dist):
    """(value, bit count) of a match at any distance: deflate_restate's length code (taken from its match at distance 1, whose
    distance code is five zero bits), then distance_bits."""
    val, n = dr.match_bits(length, 1)
    dv, dn = distance_bits(dist)
    return val | (dv << (n - 5)), n - 5 + dn


def candidates(e, row_bytes):
    return [d for d in (row_bytes, row_bytes + e, row_bytes - e) if e < d <= 32768]


def run_lengths(elems, k, e, floor_is_chunk_start):
    """For every element i of the buffer: the bytes of consecutive elements from i, up to its segment's end, that equal the
    element k before them -- from i >= k on (M_d: p >= d), or, for the run rule (floor_is_chunk_start), except at a chunk's first
    element.  (numpy only to keep the tests quick: next_false is, per segment, the first position at or behind i without the
    property.)"""
    n, per_seg = elems.size, dr.SEG // e
    eq = np.zeros(-(-n // per_seg) * per_seg, bool)           # padded to whole segments with False
    if k < n:
        eq[k:n] = elems[k:] == elems[:n - k]
    if floor_is_chunk_start:
        eq[::dr.CHUNK // e] = False
    eq = eq.reshape(-1, per_seg)
    at = np.arange(per_seg)
    next_false = np.minimum.accumulate(np.where(eq, per_seg, at)[:, ::-1], axis=1)[:, ::-1]
    return ((next_false - at) * e).ravel()


def tokens(data, e, row_bytes):
    """The rule on the whole buffer: ("lit", byte) and ("match", length, distance), and the index of every chunk's first token."""
    elems = np.frombuffer(data, {1: np.uint8, 2: np.uint16, 4: np.uint32}[e])
    cand = candidates(e, row_bytes)
    r_of = run_lengths(elems, 1, e, True)
    u_of = [run_lengths(elems, d // e, e, False) for d in cand]
    out, starts, p = [], [], 0
    while p < len(data):
        if p % dr.CHUNK == 0:
            starts.append(len(out))
        i = p // e
        r, u, best = int(r_of[i]), 0, None
        for d, u_d in zip(cand, u_of):
            if u_d[i] > u:                              # (a tie stays with the earlier candidate)
                u, best = int(u_d[i]), d
        if u >= max(4, e) and u > r:
            out.append(("match", u, best))
            p += u
        elif r >= max(3, e):
            out.append(("match", r, e))
            p += r
        else:
            out.extend(("lit", b) for b in data[p:p + e])
            p += e
    return out, starts + [len(out)]


def chunk_tokens(data, c0, e, row_bytes):
    """The tokens of the chunk that starts at byte c0 of data."""
    out, starts = tokens(bytes(data), e, row_bytes)
    return out[starts[c0 // dr.CHUNK]:starts[c0 // dr.CHUNK + 1]]


def encode_tokens(toks):
    out = bytearray()
    acc, n = 0b010, 3                      # BFINAL 0, BTYPE 01, as deflate_restate.encode_chunk
    for tok in toks:
        val, k = dr.literal_bits(tok[1]) if tok[0] == "lit" else match_bits(tok[1], tok[2])
        acc |= val << n
        n += k
        while n >= 8:                       # (whole bytes leave the accumulator at once: it stays a small integer)
            out.append(acc & 255)
            acc >>= 8
            n -= 8
    n += 7 + 3                              # end of block; the empty stored block's header bits, then the padding
    return bytes(out) + acc.to_bytes((n + 7) // 8, "little") + dr.EMPTY_STORED


def deflate_rows(data, e, row_bytes):
    data = bytes(data)
    assert e in (1, 2, 4) and len(data) % e == 0 and row_bytes > 0 and row_bytes % e == 0
    out, starts = tokens(data, e, row_bytes)
    return b"".join(encode_tokens(out[a:b]) for a, b in zip(starts[:-1], starts[1:]))
