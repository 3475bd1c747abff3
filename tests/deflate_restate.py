"""Restatement of the run-only deflate encoder of csrc/tip_deflate.hip in plain Python, for its tests: the token rule, the
fixed-Huffman bit layout of RFC 1951 and the size bound, written from the format's definition and independent of the device
code.  deflate_runs(data, e) is byte for byte what tip_deflate_runs(_dev) must produce; zlib.decompressobj(-15) inflates it
(after final_block()) to `data`.

Stream.  The input is cut into chunks of CHUNK = 65536 bytes; every chunk becomes

    one fixed-Huffman block (BFINAL 0, BTYPE 01): tokens, end-of-block code
    one empty stored block  (BFINAL 0, BTYPE 00): the header bits 000, THEN zero bits up to the byte boundary, then
                                                  LEN = 0x0000, NLEN = 0xFFFF (zlib's sync flush marker)

so the chunks are whole bytes and concatenate; an empty input is an empty stream.  No block is final: the caller puts
final_block() behind the last one (and may put stored_block(...) in front).

Token rule.  An ELEMENT is e bytes (e in 1, 2, 4).  An element "repeats" when it equals the element before it IN THE SAME
CHUNK (the chunk's first element never repeats).  The chunk is cut into SEGMENTS of SEG = 256 bytes.  Inside a segment, a
maximal group of consecutive repeating elements of R bytes becomes

    ONE match (length R, distance e)      if R >= max(3, e)
    R literal bytes                       otherwise (e = 1: R in 1, 2; e = 2: R = 2),

and every element that does not repeat becomes e literals.  A segment's first element may repeat its predecessor in the
segment before, so a run that crosses a segment edge continues as a new match there; R <= 256 < 258 needs no splitting, and
no match reaches before its chunk's start.
"""
import zlib

CHUNK = 65536
SEG = 256
EMPTY_STORED = b"\x00\x00\xff\xff"      # LEN, NLEN of an empty stored block (after its header bits and the padding)


def _rev(code, nbits):
    """Huffman codes are packed starting from their most significant bit (RFC 1951 3.1.1): the code, bit-reversed, goes into
    the stream least significant bit first like everything else."""
    out = 0
    for _ in range(nbits):
        out = (out << 1) | (code & 1)
        code >>= 1
    return out


def literal_bits(v):
    """(value to append LSB first, bit count) of literal byte v in the fixed code (RFC 1951 3.2.6)."""
    if v < 144:
        return _rev(0x30 + v, 8), 8
    return _rev(0x190 + (v - 144), 9), 9


_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_CODE = {1: 0, 2: 1, 4: 3}          # distances 1..4 are codes 0..3 without extra bits


def match_bits(length, dist):
    """(value, bit count) of a match: length symbol (fixed code), its extra bits, the 5-bit distance code."""
    assert 3 <= length <= 258 and dist in _DIST_CODE
    i = max(k for k in range(29) if _LEN_BASE[k] <= length)
    sym = 257 + i
    if sym < 280:
        val, n = _rev(sym - 256, 7), 7
    else:
        val, n = _rev(0xC0 + (sym - 280), 8), 8
    val |= (length - _LEN_BASE[i]) << n
    n += _LEN_EXTRA[i]
    val |= _rev(_DIST_CODE[dist], 5) << n
    return val, n + 5


def chunk_tokens(chunk, e):
    """The rule above on one chunk: a list of ("lit", byte) and ("match", length)."""
    assert len(chunk) <= CHUNK and len(chunk) % e == 0
    tokens = []
    for s0 in range(0, len(chunk), SEG):
        seg_end = min(s0 + SEG, len(chunk))
        run = 0

        def flush(run, at):
            if run >= max(3, e):
                tokens.append(("match", run))
            else:
                tokens.extend(("lit", b) for b in chunk[at - run:at])

        for p in range(s0, seg_end, e):
            if p >= e and chunk[p:p + e] == chunk[p - e:p]:
                run += e
            else:
                flush(run, p)
                run = 0
                tokens.extend(("lit", b) for b in chunk[p:p + e])
        flush(run, seg_end)
    return tokens


def encode_chunk(chunk, e):
    acc, n = 0b010, 3                      # BFINAL 0, BTYPE 01 (two bits, least significant first)
    for kind, v in chunk_tokens(chunk, e):
        val, k = literal_bits(v) if kind == "lit" else match_bits(v, e)
        acc |= val << n
        n += k
    n += 7                                  # end of block: symbol 256, seven zero bits
    n += 3                                  # the empty stored block's header bits 000 come BEFORE the padding
    return acc.to_bytes((n + 7) // 8, "little") + EMPTY_STORED


def deflate_runs(data, e):
    data = bytes(data)
    assert e in (1, 2, 4) and len(data) % e == 0
    return b"".join(encode_chunk(data[i:i + CHUNK], e) for i in range(0, len(data), CHUNK))


def chunk_bound(n):
    """Most bytes a chunk of n input bytes can take: 3 header bits, at most 9 bits per input byte (the longest literal; a
    match of R >= 3 bytes takes at most 8 + 5 + 5 = 18 bits, fewer than its bytes as literals), 7 bits of end-of-block, 3 header
    bits of the stored block, padding to a byte, LEN and NLEN."""
    return (3 + 9 * n + 7 + 3 + 7) // 8 + 4


def bound(nbytes):
    full, rest = divmod(nbytes, CHUNK)
    return full * chunk_bound(CHUNK) + (chunk_bound(rest) if rest else 0)


def stored_block(payload):
    """A non-final stored block holding `payload` (at most 65535 bytes), byte-aligned in front of a stream."""
    assert len(payload) <= 0xFFFF
    n = len(payload)
    return b"\x00" + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + bytes(payload)


def final_block():
    return b"\x01" + EMPTY_STORED


def inflate(stream):
    """zlib's reading of stream + final_block() as a raw deflate stream."""
    d = zlib.decompressobj(-15)
    out = d.decompress(stream + final_block()) + d.flush()
    assert d.eof and not d.unused_data
    return out
