"""Restatement of the dynamic-code deflate encoder of csrc/tip_deflate.hip (tip_deflate_dynamic, tip_deflate_dynamic_dev) in plain
Python, for its tests, written from RFC 1951 and the rules below, independent of the device code.  deflate_dynamic(data, e,
row_bytes) is byte for byte what the device must produce; this file is the specification.

Unchanged from deflate_restate / deflate_rows_restate: chunks of 65536 bytes, segments of 256, the token rule (the rows rule
when row_bytes is given -- which is the run-only rule when no candidate distance is kept --, the run-only rule for
row_bytes=None), the empty stored block behind every chunk, the bound.  New is how a chunk's tokens become bits:

    fixed form      one fixed-Huffman block (BTYPE 01), exactly the bytes of deflate_rows / deflate_runs
    dynamic form    one dynamic-Huffman block (BFINAL 0, BTYPE 10) with the chunk's own codes

whichever gives FEWER BYTES for the chunk, stored block included; a tie goes to the fixed form.  So no chunk is longer than
its fixed form and deflate_restate.bound stays the bound.  Both sizes are known exactly, in bits, before anything is written.

Alphabets.  Literal/length symbols 0 .. 285, the end of block (256) counted once; distance symbols 0 .. 29.  The literal/length
alphabet always has two used symbols or more (256, and the chunk's first element is literals).  A call has at most four
distinct distances -- e, P, P + e, P - e --, so a chunk uses at most four distance symbols and its distance code is at most 3
bits deep: the 15-bit limit can never bind there (asserted in chunk_info).

Code lengths of one alphabet, from its counts c[s]; n is the number of used symbols (c[s] > 0).
    n = 0   (distances only) no length; HDIST is 1 and the one length written is 0.
    n = 1   the symbol gets length 1 (the one incomplete code zlib's inflater accepts).
    n >= 2  1. The used symbols are sorted by (count, symbol), ascending: "rank" 0 .. n - 1.
            2. Huffman's tree by the two-queue method: queue A holds the leaves in rank order, queue B the internal nodes in the
               order they are made (their weights never decrease).  n - 1 times, take the two lightest heads -- each time the
               lighter of A's and B's head, and A's ON EQUAL WEIGHTS -- and append a node of their summed weight to B.
            3. bl[d] = number of leaves at depth d, depths above 15 counted at 15 ("the limit was applied").
            4. Only when the limit was applied, the repair: K = sum of bl[d] 2^(15 - d); while K > 2^15: bl[15] -= 1; for the
               largest d < 15 with bl[d] > 0: bl[d] -= 1, bl[d + 1] += 2; K -= 1.  The loop ends at K = 2^15: a complete code.
            5. The lengths go to the symbols BY RANK, longest first: ranks 0 .. bl[15] - 1 get 15, the next bl[14] get 14, and
               so on.  Without the repair this costs what the tree costs (the same depths, the longer ones on the lighter
               symbols), so the code is optimal; it is complete (Kraft sum 1) in either case.
Codes are canonical (RFC 1951 3.2.2): within a length, in symbol order.

Header.  HLIT = max(257, last used literal/length symbol + 1), HDIST = max(1, last used distance symbol + 1).  The HLIT + HDIST
lengths are ONE sequence (a run of zeros may cross from one alphabet into the other).  A maximal run of n zeros: while n >= 11,
symbol 18 for m = min(n, 138) (7 extra bits m - 11), n -= m; then, if n >= 3, symbol 17 (3 extra bits n - 3); else n plain
zeros.  Symbol 16 is never used.  The code-length code is the same in every block: 4 bits for the symbols 0 .. 11, 17, 18,
5 bits for 12 .. 15, none for 16 (Kraft sum 14/16 + 4/32 = 1); canonical, so 0 .. 11 are the 4-bit codes 0 .. 11, 17 and 18 are
12 and 13, and 12 .. 15 are the 5-bit codes 28 .. 31.  In the permuted order of RFC 1951 3.2.7 the last symbol is 15: HCLEN is 19.
"""
import deflate_restate as dr
import deflate_rows_restate as rr

MAX_BITS = 15
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_LENGTHS = [4] * 12 + [5] * 4 + [0, 4, 4]


def code_lengths(counts):
    """(lengths, limit applied) of one alphabet: the construction of this file's head."""
    used = sorted((c, s) for s, c in enumerate(counts) if c > 0)
    lengths, n = [0] * len(counts), len(used)
    if n == 0:
        return lengths, False
    if n == 1:
        lengths[used[0][1]] = 1
        return lengths, False
    weight = [c for c, _ in used]                 # nodes 0 .. n - 1: the leaves by rank; n ..: the internal nodes as made
    parent = [None] * (2 * n - 1)
    a, b = 0, n                                   # the heads of queue A (leaves) and queue B (internal nodes)
    for _ in range(n - 1):
        pair = []
        for _ in range(2):
            if a < n and (b >= len(weight) or weight[a] <= weight[b]):       # (equal weights: the leaf)
                pair.append(a)
                a += 1
            else:
                pair.append(b)
                b += 1
        for node in pair:
            parent[node] = len(weight)
        weight.append(weight[pair[0]] + weight[pair[1]])
    bl, limited = [0] * (MAX_BITS + 1), False
    for leaf in range(n):
        depth, node = 0, leaf
        while parent[node] is not None:
            node, depth = parent[node], depth + 1
        limited |= depth > MAX_BITS
        bl[min(depth, MAX_BITS)] += 1
    if limited:
        kraft = sum(bl[d] << (MAX_BITS - d) for d in range(1, MAX_BITS + 1))
        while kraft > 1 << MAX_BITS:
            bl[MAX_BITS] -= 1
            d = max(d for d in range(1, MAX_BITS) if bl[d])
            bl[d] -= 1
            bl[d + 1] += 2
            kraft -= 1
    rank = 0
    for d in range(MAX_BITS, 0, -1):
        for _, s in used[rank:rank + bl[d]]:
            lengths[s] = d
        rank += bl[d]
    assert rank == n
    return lengths, limited


def canonical(lengths):
    """RFC 1951 3.2.2: the code of every symbol with a length (None for the others)."""
    bl = [0] * (max(lengths) + 2)
    for n in lengths:
        bl[n] += n > 0
    code, first = 0, [0] * len(bl)
    for bits in range(1, len(bl)):
        code = (code + bl[bits - 1]) << 1
        first[bits] = code
    out = []
    for n in lengths:
        out.append(first[n] if n else None)
        first[n] += 1
    return out


_CL_CODES = canonical(CL_LENGTHS)


def length_symbol(length):
    """(symbol, extra bits, their count) of a match length 3 .. 258"""
    i = max(k for k in range(29) if dr._LEN_BASE[k] <= length)
    return 257 + i, length - dr._LEN_BASE[i], dr._LEN_EXTRA[i]


def distance_symbol(dist):
    code = max(k for k in range(30) if rr._DIST_BASE[k] <= dist)
    return code, dist - rr._DIST_BASE[code], rr._DIST_EXTRA[code]


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, val, k):                         # least significant bit first
        self.acc |= val << self.n
        self.n += k
        self.total += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, k):                       # a Huffman code: from its most significant bit
        self.put(dr._rev(code, k), k)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def _header(w, lit_len, dist_len):
    hlit = max(257, max(s for s in range(286) if lit_len[s]) + 1)
    hdist = max([1] + [s + 1 for s in range(30) if dist_len[s]])
    w.put(0b100, 3)                                # BFINAL 0, BTYPE 10 (two bits, least significant first)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(CL_LENGTHS[s], 3)
    seq = lit_len[:hlit] + dist_len[:hdist]
    i = 0
    while i < len(seq):
        if seq[i]:
            w.huff(_CL_CODES[seq[i]], CL_LENGTHS[seq[i]])
            i += 1
            continue
        n = 0
        while i + n < len(seq) and seq[i + n] == 0:
            n += 1
        i += n
        while n >= 11:
            m = min(n, 138)
            w.huff(_CL_CODES[18], CL_LENGTHS[18])
            w.put(m - 11, 7)
            n -= m
        if n >= 3:
            w.huff(_CL_CODES[17], CL_LENGTHS[17])
            w.put(n - 3, 3)
        else:
            for _ in range(n):
                w.huff(_CL_CODES[0], CL_LENGTHS[0])


def _dynamic_block(toks, lit_len, dist_len):
    """(bytes of the dynamic block up to and including its end-of-block code, its bits)"""
    lit_code, dist_code = canonical(lit_len), canonical(dist_len)
    w = _Bits()
    _header(w, lit_len, dist_len)
    for tok in toks:
        if tok[0] == "lit":
            w.huff(lit_code[tok[1]], lit_len[tok[1]])
        else:
            s, x, k = length_symbol(tok[1])
            w.huff(lit_code[s], lit_len[s])
            w.put(x, k)
            s, x, k = distance_symbol(tok[2])
            w.huff(dist_code[s], dist_len[s])
            w.put(x, k)
    w.huff(lit_code[256], lit_len[256])
    return w, w.total


def _chunks_of_tokens(data, e, row_bytes):
    if row_bytes is None:
        return [[t if t[0] == "lit" else ("match", t[1], e) for t in dr.chunk_tokens(data[i:i + dr.CHUNK], e)]
                for i in range(0, len(data), dr.CHUNK)]
    toks, starts = rr.tokens(data, e, row_bytes)
    return [toks[a:b] for a, b in zip(starts[:-1], starts[1:])]


def _encode(data, e, row_bytes):
    data = bytes(data)
    assert e in (1, 2, 4) and len(data) % e == 0 and (row_bytes is None or (row_bytes > 0 and row_bytes % e == 0))
    out, info = [], []
    for toks in _chunks_of_tokens(data, e, row_bytes):
        fixed = rr.encode_tokens(toks)
        lit, dist = [0] * 286, [0] * 30
        lit[256] = 1
        for tok in toks:
            if tok[0] == "lit":
                lit[tok[1]] += 1
            else:
                lit[length_symbol(tok[1])[0]] += 1
                dist[distance_symbol(tok[2])[0]] += 1
        assert sum(c > 0 for c in lit) >= 2 and sum(c > 0 for c in dist) <= 4
        (lit_len, lit_limited), (dist_len, dist_limited) = code_lengths(lit), code_lengths(dist)
        assert not dist_limited and max(dist_len) <= 3          # four symbols at the most: the limit cannot bind
        w, bits = _dynamic_block(toks, lit_len, dist_len)
        dynamic_bytes = (bits + 3 + 7) // 8 + 4                 # the stored block's header bits, the padding, LEN and NLEN
        form = "dynamic" if dynamic_bytes < len(fixed) else "fixed"
        if form == "dynamic":
            w.put(0, 3)
            chunk = w.bytes() + dr.EMPTY_STORED
            assert len(chunk) == dynamic_bytes
        else:
            chunk = fixed
        out.append(chunk)
        info.append(dict(form=form, fixed_bytes=len(fixed), dynamic_bytes=dynamic_bytes, size=len(chunk), lit_lengths=lit_len,
                         dist_lengths=dist_len, lit_counts=lit, dist_counts=dist, limit_applied=lit_limited))
    return b"".join(out), info


def deflate_dynamic(data, e, row_bytes=None):
    return _encode(data, e, row_bytes)[0]


def chunk_info(data, e, row_bytes=None):
    """Per chunk: form ("fixed" or "dynamic"), fixed_bytes, dynamic_bytes, size (the chosen form's), lit_lengths, dist_lengths (the
    dynamic form's two tables, whichever form was chosen), lit_counts, dist_counts, limit_applied."""
    return _encode(data, e, row_bytes)[1]
