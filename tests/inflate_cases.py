"""Named deflate streams for the inflate tests (tip_inflate_strips*): valid ones built with the standard library's zlib -- or
by hand where zlib never writes the token (a distance of 32768) -- each in its raw (RFC 1951) and zlib-wrapped (RFC 1950) form,
and hand-made invalid ones, one per status word.  A case is (name, stream, wrapper, expected bytes or None, dst_len, status
name).  `walk` is a small inflate of the tests' own that reports what a stream contains: its block types and its longest code.
`dump` writes the list as the binary case file tools/inflate_hostcheck.cpp reads."""
import struct
import zlib

import numpy as np


# ---- bits ------------------------------------------------------------------------------------------------------------------
class BitWriter(object):
    """RFC 1951's packing: values least-significant bit first, Huffman codes most-significant bit first."""

    def __init__(self):
        self.bits = []

    def value(self, v, n):
        self.bits += [(v >> i) & 1 for i in range(n)]
        return self

    def code(self, c, n):
        self.bits += [(c >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)
        return self

    def raw(self, data):
        assert len(self.bits) % 8 == 0
        for b in data:
            self.value(b, 8)
        return self

    def bytes(self):
        bits = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(bits[i + k] << k for k in range(8)) for i in range(0, len(bits), 8))


def fixed_lit(w, s):
    """literal/length symbol s under the fixed code (RFC 1951 3.2.6)"""
    if s < 144:
        return w.code(0x30 + s, 8)
    if s < 256:
        return w.code(0x190 + s - 144, 9)
    if s < 280:
        return w.code(s - 256, 7)
    return w.code(0xC0 + s - 280, 8)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def fixed_match(w, length, dist):
    ls = max(i for i in range(29) if LEN_BASE[i] <= length and (i < 28 or length == 258))
    fixed_lit(w, 257 + ls).value(length - LEN_BASE[ls], LEN_EXTRA[ls])
    ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return w.code(ds, 5).value(dist - DIST_BASE[ds], DIST_EXTRA[ds])


# ---- the tests' own inflate: what a stream contains ---------------------------------------------------------------------------
class WalkError(Exception):
    pass


def _canonical(lens):
    """{(length, code): symbol}"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[(l, code)] = s
                code += 1
        code <<= 1
    return out


def walk(stream, wrapper):
    """(output bytes, set of block types met, longest literal/length or distance code length USED by a symbol)"""
    pos = [16 if wrapper else 0]
    nbits = len(stream) * 8

    def bits(n):
        if pos[0] + n > nbits:
            raise WalkError("input exhausted")
        v = 0
        for i in range(n):
            v |= ((stream[(pos[0] + i) >> 3] >> ((pos[0] + i) & 7)) & 1) << i
        pos[0] += n
        return v

    def sym(table):
        code = 0
        for l in range(1, 16):
            code = (code << 1) | bits(1)
            if (l, code) in table:
                return table[(l, code)], l
        raise WalkError("no such code")

    out, types, longest = bytearray(), set(), 0
    fixed = (_canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _canonical([5] * 32))
    while True:
        last, typ = bits(1), bits(2)
        types.add(typ)
        if typ == 0:
            pos[0] += -pos[0] % 8
            n, nn = bits(16), bits(16)
            if n ^ 0xFFFF != nn:
                raise WalkError("LEN/NLEN")
            if pos[0] + 8 * n > nbits:
                raise WalkError("input exhausted")
            out += stream[pos[0] >> 3:(pos[0] >> 3) + n]
            pos[0] += 8 * n
        elif typ in (1, 2):
            if typ == 1:
                lit, dist = fixed
            else:
                nl, nd, nc = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(nc):
                    cl[CL_ORDER[i]] = bits(3)
                clt, lens = _canonical(cl), []
                while len(lens) < nl + nd:
                    s, _ = sym(clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * ((3 + bits(3)) if s == 17 else (11 + bits(7)))
                if len(lens) != nl + nd:
                    raise WalkError("repeat past the end")
                lit, dist = _canonical(lens[:nl]), _canonical(lens[nl:])
            while True:
                s, l = sym(lit)
                longest = max(longest, l)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    length = LEN_BASE[s - 257] + bits(LEN_EXTRA[s - 257])
                    d, l = sym(dist)
                    longest = max(longest, l)
                    distance = DIST_BASE[d] + bits(DIST_EXTRA[d])
                    if distance > len(out):
                        raise WalkError("distance")
                    for _ in range(length):
                        out.append(out[-distance])
        else:
            raise WalkError("BTYPE 3")
        if last:
            return bytes(out), types, longest


# ---- valid cases ----------------------------------------------------------------------------------------------------------------
def _deflate(data, wrapper, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 15 if wrapper else -15, 9, strategy)
    return co.compress(data) + co.flush()


def _wrap(raw, data):
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data))


def _rng(seed):
    return np.random.default_rng(seed)


def _fibonacci_bytes():
    """Symbol counts 1, 1, 2, 3, 5, ... over 22 symbols (46 367 bytes, more than one block): the Huffman tree of a block is a
    chain, and zlib's length limit of 15 is reached"""
    counts, a, b = [], 1, 1
    for _ in range(22):
        counts.append(a)
        a, b = b, a + b
    data = np.repeat(np.arange(len(counts), dtype=np.uint8) + 40, counts)
    _rng(15).shuffle(data)
    return data.tobytes()


def _smooth_u16(differenced):
    yy, xx = np.mgrid[0:48, 0:64]
    img = (3000 + 900 * np.sin(yy / 7.0) * np.cos(xx / 9.0) + _rng(16).integers(0, 6, (48, 64))).astype("<u2")
    if differenced:
        img = np.concatenate([img[:, :1], np.diff(img, axis=1)], axis=1).astype("<u2")      # modulo 2^16: TIFF predictor 2
    return img.tobytes()


def _three_parts(wrapper):
    parts = [bytes(_rng(17).integers(0, 5, 3000, dtype=np.uint8)), b"sync and full flush " * 90, bytes(_rng(18).integers(0, 200, 2500, dtype=np.uint8))]
    co = zlib.compressobj(6, zlib.DEFLATED, 15 if wrapper else -15)
    s = co.compress(parts[0]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(parts[1]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(parts[2]) + co.flush()
    return s, b"".join(parts)


def _distance_32768():
    """zlib's own matcher stops at 32768 - 262, so the largest distance is written by hand: the bytes in one stored block, then
    their first 300 as two matches of a fixed block."""
    r = bytes(_rng(19).integers(0, 256, 32768, dtype=np.uint8))
    w = BitWriter().value(0, 1).value(0, 2).align().value(32768, 16).value(32768 ^ 0xFFFF, 16).raw(r)
    w.value(1, 1).value(1, 2)
    fixed_match(w, 258, 32768)
    fixed_match(w, 42, 32768)
    fixed_lit(w, 256)
    return w.bytes(), r + r[:300]


def _valid():
    text = (b"the strips of a compressed page are independent streams; " * 40)[:2000]
    skew = bytes(np.minimum(_rng(11).geometric(0.08, 20000), 255).astype(np.uint8))
    built = [
        ("empty", b"", dict()),
        ("one_byte", b"\x5a", dict()),
        ("stored", bytes(_rng(12).integers(0, 256, 1000, dtype=np.uint8)), dict(level=0)),
        ("stored_many", bytes(_rng(13).integers(0, 256, 70000, dtype=np.uint8)), dict(level=0)),
        ("fixed", text, dict(strategy=zlib.Z_FIXED)),
        ("literals_only", skew[:6000], dict(strategy=zlib.Z_HUFFMAN_ONLY)),
        ("distance_1", b"a" * 262 + b"tail", dict(strategy=zlib.Z_RLE)),       # a, a match of 258, a match of 3
        ("dynamic", skew, dict(level=9)),
        ("codes_15_bits", _fibonacci_bytes(), dict(strategy=zlib.Z_HUFFMAN_ONLY)),
        ("smooth_u16", _smooth_u16(False), dict(level=6)),
        ("smooth_u16_differenced", _smooth_u16(True), dict(level=6)),
    ]
    cases = []
    for wrapper in (0, 1):
        form = "zlib" if wrapper else "raw"
        for name, data, kw in built:
            cases.append(("%s_%s" % (name, form), _deflate(data, wrapper, **kw), wrapper, data, len(data), "OK"))
        s, data = _three_parts(wrapper)
        cases.append(("three_parts_flushed_%s" % form, s, wrapper, data, len(data), "OK"))
        s, data = _distance_32768()
        cases.append(("distance_32768_%s" % form, _wrap(s, data) if wrapper else s, wrapper, data, len(data), "OK"))
    return cases


# ---- invalid cases, by hand --------------------------------------------------------------------------------------------------
def _invalid():
    skew = bytes(np.minimum(_rng(11).geometric(0.08, 20000), 255).astype(np.uint8))
    dyn = _deflate(skew[:4000], 0, level=9)              # one dynamic block: its header is 14 bits, its code table tens of bytes
    cases = [
        ("truncated_at_header", dyn[:1], 0, None, 4000, "INPUT_END"),
        ("truncated_at_code_table", dyn[:10], 0, None, 4000, "INPUT_END"),
    ]
    # a, then a match of 258 at distance 24577 + 13 extra bits: 37 bits, cut after 32 -- inside the distance's extra bits
    w = BitWriter().value(1, 1).value(1, 2)
    fixed_lit(w, ord("a"))
    fixed_lit(w, 285).code(29, 5).value(0, 13)
    cases.append(("truncated_inside_match", w.bytes()[:4], 0, None, 259, "INPUT_END"))
    cases.append(("btype_3", BitWriter().value(1, 1).value(3, 2).bytes(), 0, None, 0, "BAD_BLOCK_TYPE"))
    cases.append(("len_nlen_mismatch", b"\x01\x05\x00\x00\x00hello", 0, None, 5, "BAD_STORED"))
    # dynamic header, HCLEN 4: the code-length codes 16, 17, 18 all of length 1 -- three codes where two fit
    w = BitWriter().value(1, 1).value(2, 2).value(0, 5).value(0, 5).value(0, 4).value(1, 3).value(1, 3).value(1, 3).value(0, 3)
    cases.append(("oversubscribed_lengths", w.bytes() + b"\0" * 4, 0, None, 0, "BAD_LENGTHS"))
    # code-length code {16: 1 bit, 0: 1 bit}: complete; canonical codes 0 -> "0", 16 -> "1"; the first symbol sent is 16
    w = BitWriter().value(1, 1).value(2, 2).value(0, 5).value(0, 5).value(0, 4).value(1, 3).value(0, 3).value(0, 3).value(1, 3)
    w.code(1, 1).value(0, 2)
    cases.append(("repeat_16_first", w.bytes() + b"\0" * 4, 0, None, 0, "BAD_LENGTHS"))
    w = BitWriter().value(1, 1).value(1, 2)
    fixed_lit(w, 286)
    cases.append(("symbol_286", w.bytes() + b"\0" * 2, 0, None, 0, "BAD_SYMBOL"))
    w = BitWriter().value(1, 1).value(1, 2)
    fixed_lit(w, ord("a"))
    fixed_lit(w, 257).code(30, 5)
    cases.append(("distance_code_30", w.bytes() + b"\0" * 2, 0, None, 4, "BAD_SYMBOL"))
    w = BitWriter().value(1, 1).value(1, 2)
    fixed_lit(w, ord("a"))
    fixed_lit(w, ord("b"))
    fixed_match(w, 3, 3)
    fixed_lit(w, 256)
    cases.append(("distance_beyond_output", w.bytes(), 0, None, 5, "BAD_DISTANCE"))
    data = bytes(_rng(14).integers(0, 9, 500, dtype=np.uint8))
    cases.append(("one_byte_too_many", _deflate(data + b"\x01", 0), 0, None, 500, "OUTPUT_FULL"))
    cases.append(("one_byte_too_few", _deflate(data[:-1], 0), 0, None, 500, "OUTPUT_SHORT"))
    z = bytearray(_deflate(data, 1))
    z[-1] ^= 1
    cases.append(("wrong_adler", bytes(z), 1, None, 500, "BAD_ADLER"))
    cases.append(("fdict_set", b"\x78\x20" + _deflate(data, 0) + struct.pack(">I", zlib.adler32(data)), 1, None, 500, "BAD_HEADER"))
    return cases


VALID = _valid()
INVALID = _invalid()
CASES = VALID + INVALID
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

GUARD = 64            # bytes of a fixed pattern before, between and after the destinations


def guard_pattern(n):
    return (np.arange(n, dtype=np.int64) * 37 + 11).astype(np.uint8)


def pack(cases):
    """The cases of one wrapper as one call: (src, strips (n, 4) int64, dst filled with the guard pattern)."""
    src = b"".join(c[1] for c in cases)
    strips, s_off, d_off = [], 0, GUARD
    for c in cases:
        strips.append((s_off, len(c[1]), d_off, c[4]))
        s_off += len(c[1])
        d_off += c[4] + GUARD
    return np.frombuffer(src, np.uint8).copy(), np.array(strips, np.int64).reshape(-1, 4), guard_pattern(d_off)


def check_packed(cases, strips, dst, status, status_code):
    """every case's bytes (valid) and status, and every guard byte of dst"""
    pattern = guard_pattern(dst.size)
    inside = np.zeros(dst.size, bool)
    for c, (_, _, d_off, d_len), st in zip(cases, strips, status):
        assert int(st) == status_code[c[5]], (c[0], int(st), c[5])
        if c[3] is not None:
            assert dst[d_off:d_off + d_len].tobytes() == c[3], c[0]
        inside[d_off:d_off + d_len] = True
    assert np.array_equal(dst[~inside], pattern[~inside]), "a byte outside every strip's destination changed"


def dump(path, cases=None):
    """The case file of tools/inflate_hostcheck.cpp: int32 count, then per case int32 wrapper, status (-1: any), valid flag,
    int64 src_len, dst_len, the stream, and for a valid case the expected bytes."""
    from tissue_image_processing_amd._inflate import STATUS
    cases = CASES if cases is None else cases
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for name, stream, wrapper, expected, dst_len, status in cases:
            fh.write(struct.pack("<iiiqq", wrapper, STATUS[status], int(expected is not None), len(stream), dst_len))
            fh.write(stream)
            if expected is not None:
                fh.write(expected)
