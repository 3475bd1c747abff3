// tip_inflate_core.h -- one inflate (RFC 1950 zlib-wrapped / RFC 1951 raw) of one strip, compiled as device code by
// tip_inflate.hip and as plain host C++ by the same unit (tip_inflate_strips_host) and by tools/inflate_hostcheck.cpp.
//
// The stream contract: `src` points at the strip's first compressed byte and holds src_len of them; the output is the
// strip's own dst_len bytes and nothing else.  The window is the output written so far: a match never reaches before
// byte 0 of the strip, so strips decode independently.  Status words: tip_inflate_status in include/tissue_hip.h.
//
// What is bounds-checked, and where (the only places that touch memory):
//   * Bits::refill is the only reader of src.  Its word path loads 8 bytes only when p + 8 <= end, its byte path only
//     while p < end; bits beyond the last byte are never counted in `n`, and every consumer tests `n` before it takes
//     bits (need / the decoders), so a truncated stream ends in TIP_INFLATE_INPUT_END.
//   * inflate_stream is the only caller of Out::lit / Out::match / Out::adler, and tests pos < dst_len (a literal),
//     pos + length <= dst_len and distance <= pos (a match) before the call.  An Out therefore only ever sees positions
//     inside [0, dst_len) and match sources inside [0, pos).
//   * The tables are indexed by masked bits (fast tables), by symbols below the table's own size, and by lengths 0..15.
//
// The Huffman decoder: a fast table indexed by the next LIT_FAST / DIST_FAST bits (entry = symbol << 4 | length, 0: not
// there) and, for the longer codes, the canonical walk over count[] / sym[] one bit at a time (the second level).
#pragma once
#include <stdint.h>
#include "../../include/tissue_hip.h"

#if defined(__HIPCC__)
#define TIP_INF_HD __host__ __device__ __forceinline__
#else
#define TIP_INF_HD inline
#endif

namespace tip_inflate {

constexpr int LIT_FAST = 10, DIST_FAST = 8, MAX_BITS = 15;
constexpr int MAX_LIT = 288, MAX_DIST = 32, MAX_LENS = 320;    // 288 + 32: what the fixed codes use; a dynamic header gives at most 286 + 30

struct Tables {
    uint16_t lit_fast[1 << LIT_FAST];
    uint16_t dist_fast[1 << DIST_FAST];      // (also the code-length code's table while a dynamic header is read)
    uint16_t lit_sym[MAX_LIT], dist_sym[MAX_DIST];
    uint16_t lit_count[MAX_BITS + 1], dist_count[MAX_BITS + 1];
    uint16_t offs[2 * (MAX_BITS + 2)];       // scratch of build(): where each length's symbols go, and each length's next code
    uint8_t lens[MAX_LENS];
    int fixed_ready;                         // the lit / dist tables hold the fixed codes (kept from block to block, strip to strip)
};

struct Bits {
    const uint8_t *src;
    int64_t p, end;
    uint64_t buf;
    int n;                                   // valid bits in buf; bits above them are zero or the stream's own next bits

    TIP_INF_HD void refill()
    {
        if (p + 8 <= end) {
            uint64_t w;
            __builtin_memcpy(&w, src + p, 8);
            buf |= w << n;
            const int adv = (63 - n) >> 3;
            p += adv;
            n += adv * 8;
        } else {
            while (n <= 56 && p < end) {
                buf |= (uint64_t)src[p++] << n;
                n += 8;
            }
        }
    }
    TIP_INF_HD bool need(int k)              // k <= 32
    {
        if (n < k) refill();
        return n >= k;
    }
    TIP_INF_HD uint32_t take(int k)          // after need(k)
    {
        const uint32_t v = (uint32_t)(buf & ((1ull << k) - 1ull));
        buf >>= k;
        n -= k;
        return v;
    }
};

// The canonical code of lens[0, nsym): count[], sym[] (symbols by length, then value) and the fast table of `fast_bits`.
// Returns 0, or TIP_INFLATE_BAD_LENGTHS: over-subscribed, or incomplete unless allow_single and the set is empty or one
// code of length 1 (the distance code of a block with one distance, which zlib accepts).
TIP_INF_HD int build(const uint8_t *lens, int nsym, uint16_t *count, uint16_t *sym, uint16_t *fast, int fast_bits, uint16_t *offs,
                     bool allow_single)
{
    for (int l = 0; l <= MAX_BITS; ++l) count[l] = 0;
    for (int s = 0; s < nsym; ++s) count[lens[s]] = (uint16_t)(count[lens[s]] + 1);
    int left = 1, maxlen = 0;
    for (int l = 1; l <= MAX_BITS; ++l) {
        left = (left << 1) - (int)count[l];
        if (left < 0) return TIP_INFLATE_BAD_LENGTHS;
        if (count[l]) maxlen = l;
    }
    if (left > 0 && !(allow_single && maxlen <= 1)) return TIP_INFLATE_BAD_LENGTHS;
    count[0] = 0;
    offs[1] = 0;
    for (int l = 1; l <= MAX_BITS; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int i = 0; i < (1 << fast_bits); ++i) fast[i] = 0;
    // first code of each length, kept in `left`-style arithmetic: code(l) = (code(l - 1) + count[l - 1]) << 1
    uint16_t *next = offs + MAX_BITS + 2;
    uint32_t code = 0;
    for (int l = 1; l <= MAX_BITS; ++l) {
        code = (code + (l > 1 ? count[l - 1] : 0u)) << 1;
        next[l] = (uint16_t)code;           // (a used length's first code is below 2^l)
    }
    for (int s = 0; s < nsym; ++s) {
        const int l = lens[s];
        if (!l) continue;
        sym[offs[l]] = (uint16_t)s;
        offs[l] = (uint16_t)(offs[l] + 1);
        const uint32_t c = next[l];
        next[l] = (uint16_t)(c + 1);
        if (l <= fast_bits) {
            uint32_t rev = 0;
            for (int b = 0; b < l; ++b) rev |= ((c >> b) & 1u) << (l - 1 - b);
            for (uint32_t i = rev; i < (1u << fast_bits); i += 1u << l) fast[i] = (uint16_t)((s << 4) | l);
        }
    }
    return 0;
}

// One symbol.  0 and *out, TIP_INFLATE_INPUT_END when the stream ends inside the code, TIP_INFLATE_BAD_SYMBOL for bits that are
// no code of an incomplete set.
TIP_INF_HD int decode(Bits &b, const uint16_t *fast, int fast_bits, const uint16_t *count, const uint16_t *sym, int *out)
{
    if (b.n < MAX_BITS) b.refill();
    const uint32_t e = fast[b.buf & ((1u << fast_bits) - 1u)];
    const int len = (int)(e & 15u);
    if (len) {
        if (len > b.n) return TIP_INFLATE_INPUT_END;
        b.buf >>= len;
        b.n -= len;
        *out = (int)(e >> 4);
        return 0;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= MAX_BITS; ++l) {
        if (l > b.n) return TIP_INFLATE_INPUT_END;
        code |= (int)((b.buf >> (l - 1)) & 1u);
        const int cnt = count[l];
        if (code - cnt < first) {
            *out = sym[index + (code - first)];
            b.buf >>= l;
            b.n -= l;
            return 0;
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return TIP_INFLATE_BAD_SYMBOL;
}

TIP_INF_HD void fixed_lengths(uint8_t *lens)
{
    for (int s = 0; s < 144; ++s) lens[s] = 8;
    for (int s = 144; s < 256; ++s) lens[s] = 9;
    for (int s = 256; s < 280; ++s) lens[s] = 7;
    for (int s = 280; s < 288; ++s) lens[s] = 8;
    for (int s = 0; s < 32; ++s) lens[288 + s] = 5;
}

// the order of the code-length code's lengths in a dynamic header (RFC 1951 3.2.7), five bits each
TIP_INF_HD int cl_order(int i)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)(((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12)))) & 31u);
}

// The header of a dynamic block: the two codes into T.  0 or a status.
TIP_INF_HD int dynamic_header(Bits &b, Tables &T)
{
    if (!b.need(14)) return TIP_INFLATE_INPUT_END;
    const int nlen = (int)b.take(5) + 257, ndist = (int)b.take(5) + 1, ncode = (int)b.take(4) + 4;
    if (nlen > 286 || ndist > 30) return TIP_INFLATE_BAD_LENGTHS;
    T.fixed_ready = 0;
    for (int i = 0; i < 19; ++i) T.lens[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        if (!b.need(3)) return TIP_INFLATE_INPUT_END;
        T.lens[cl_order(i)] = (uint8_t)b.take(3);
    }
    // the code-length code: 19 symbols, at most 7 bits, all in the fast table (dist_fast and dist_count / dist_sym borrowed)
    if (build(T.lens, 19, T.dist_count, T.dist_sym, T.dist_fast, 7, T.offs, false)) return TIP_INFLATE_BAD_LENGTHS;
    int i = 0;
    while (i < nlen + ndist) {
        int s;
        if (int rc = decode(b, T.dist_fast, 7, T.dist_count, T.dist_sym, &s)) return rc == TIP_INFLATE_BAD_SYMBOL ? TIP_INFLATE_BAD_LENGTHS : rc;
        if (s < 16) {
            T.lens[i++] = (uint8_t)s;
            continue;
        }
        int rep, val = 0;
        if (s == 16) {
            if (i == 0) return TIP_INFLATE_BAD_LENGTHS;
            if (!b.need(2)) return TIP_INFLATE_INPUT_END;
            val = T.lens[i - 1];
            rep = 3 + (int)b.take(2);
        } else if (s == 17) {
            if (!b.need(3)) return TIP_INFLATE_INPUT_END;
            rep = 3 + (int)b.take(3);
        } else {
            if (!b.need(7)) return TIP_INFLATE_INPUT_END;
            rep = 11 + (int)b.take(7);
        }
        if (i + rep > nlen + ndist) return TIP_INFLATE_BAD_LENGTHS;
        while (rep--) T.lens[i++] = (uint8_t)val;
    }
    if (T.lens[256] == 0) return TIP_INFLATE_BAD_LENGTHS;
    // the distance lengths first: building the literal/length code reuses nothing of lens, but the distance build must not
    // read lengths the literal build has moved -- neither moves any, both only read
    if (build(T.lens + nlen, ndist, T.dist_count, T.dist_sym, T.dist_fast, DIST_FAST, T.offs, true)) return TIP_INFLATE_BAD_LENGTHS;
    if (build(T.lens, nlen, T.lit_count, T.lit_sym, T.lit_fast, LIT_FAST, T.offs, false)) return TIP_INFLATE_BAD_LENGTHS;
    return 0;
}

TIP_INF_HD void fixed_tables(Tables &T)
{
    if (T.fixed_ready) return;
    fixed_lengths(T.lens);
    build(T.lens, 288, T.lit_count, T.lit_sym, T.lit_fast, LIT_FAST, T.offs, false);
    build(T.lens + 288, 32, T.dist_count, T.dist_sym, T.dist_fast, DIST_FAST, T.offs, false);
    T.fixed_ready = 1;
}

// An Out carries out what the stream says, inside the strip's own dst_len bytes:
//   void lit(int64_t pos, uint32_t byte);  void match(int64_t pos, int length, int distance);  uint32_t adler(int64_t n);
// called with checked arguments only (see the head).  wrapper: 0 raw, 1 zlib.
template <class Out>
TIP_INF_HD int inflate_stream(const uint8_t *src, int64_t src_len, int64_t dst_len, int wrapper, Tables &T, Out &out)
{
    Bits b{src, 0, src_len, 0, 0};
    if (wrapper) {
        if (!b.need(16)) return TIP_INFLATE_INPUT_END;
        const uint32_t cmf = b.take(8), flg = b.take(8);
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u || (flg & 32u)) return TIP_INFLATE_BAD_HEADER;
    }
    int64_t pos = 0;
    for (;;) {
        if (!b.need(3)) return TIP_INFLATE_INPUT_END;
        const uint32_t last = b.take(1), type = b.take(2);
        if (type == 3) return TIP_INFLATE_BAD_BLOCK_TYPE;
        if (type == 0) {
            b.take(b.n & 7);                     // to the byte boundary: n counts whole bytes beyond it
            if (!b.need(32)) return TIP_INFLATE_INPUT_END;
            const uint32_t len = b.take(16), nlen = b.take(16);
            if ((len ^ 0xFFFFu) != nlen) return TIP_INFLATE_BAD_STORED;
            for (uint32_t i = 0; i < len; ++i) {
                if (!b.need(8)) return TIP_INFLATE_INPUT_END;
                if (pos >= dst_len) return TIP_INFLATE_OUTPUT_FULL;
                out.lit(pos++, b.take(8));
            }
        } else {
            if (type == 1) fixed_tables(T);
            else if (int rc = dynamic_header(b, T)) return rc;
            for (;;) {
                int s;
                if (int rc = decode(b, T.lit_fast, LIT_FAST, T.lit_count, T.lit_sym, &s)) return rc;
                if (s < 256) {
                    if (pos >= dst_len) return TIP_INFLATE_OUTPUT_FULL;
                    out.lit(pos++, (uint32_t)s);
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return TIP_INFLATE_BAD_SYMBOL;
                s -= 257;                        // lengths (RFC 1951 3.2.5): 3..10 plain, then four codes per extra bit, 258 last
                int length;
                if (s < 8) length = 3 + s;
                else if (s == 28) length = 258;
                else {
                    const int e = (s >> 2) - 1;
                    if (!b.need(e)) return TIP_INFLATE_INPUT_END;
                    length = 3 + ((4 + (s & 3)) << e) + (int)b.take(e);
                }
                int d;
                if (int rc = decode(b, T.dist_fast, DIST_FAST, T.dist_count, T.dist_sym, &d)) return rc;
                if (d > 29) return TIP_INFLATE_BAD_SYMBOL;
                int distance;                    // distances: 1..4 plain, then two codes per extra bit
                if (d < 4) distance = d + 1;
                else {
                    const int e = (d >> 1) - 1;
                    if (!b.need(e)) return TIP_INFLATE_INPUT_END;
                    distance = 1 + ((2 + (d & 1)) << e) + (int)b.take(e);
                }
                if ((int64_t)distance > pos) return TIP_INFLATE_BAD_DISTANCE;
                if (pos + length > dst_len) return TIP_INFLATE_OUTPUT_FULL;
                out.match(pos, length, distance);
                pos += length;
            }
        }
        if (last) break;
    }
    if (pos != dst_len) return TIP_INFLATE_OUTPUT_SHORT;
    if (wrapper) {
        b.take(b.n & 7);
        if (!b.need(32)) return TIP_INFLATE_INPUT_END;
        uint32_t want = 0;
        for (int i = 0; i < 4; ++i) want = (want << 8) | b.take(8);
        if (out.adler(dst_len) != want) return TIP_INFLATE_BAD_ADLER;
    }
    return TIP_INFLATE_OK;
}

// Adler-32 from partial sums: s1 = sum d[i], s2 = sum ((n - i) mod 65521) d[i] over all i < n, both already reduced mod 65521
TIP_INF_HD uint32_t adler_from_sums(uint32_t s1, uint32_t s2, int64_t n)
{
    const uint32_t a = (1u + s1) % 65521u, b = (uint32_t)((uint64_t)(n % 65521) + s2) % 65521u;
    return (b << 16) | a;
}

// the serial Out: plain host C++
struct SerialOut {
    uint8_t *dst;
    TIP_INF_HD void lit(int64_t pos, uint32_t byte) { dst[pos] = (uint8_t)byte; }
    TIP_INF_HD void match(int64_t pos, int length, int distance)
    {
        for (int i = 0; i < length; ++i) dst[pos + i] = dst[pos + i - distance];     // ascending: an overlapping match repeats
    }
    TIP_INF_HD uint32_t adler(int64_t n)
    {
        uint64_t s1 = 0, s2 = 0;
        int64_t w = n % 65521;               // (n - i) mod 65521
        for (int64_t i = 0; i < n; ++i) {
            s1 += dst[i];
            s2 += (uint64_t)w * dst[i];
            if (--w < 0) w += 65521;
        }
        return adler_from_sums((uint32_t)(s1 % 65521u), (uint32_t)(s2 % 65521u), n);
    }
};

// One strip on the host.  strip: src_off, src_len, dst_off, dst_len, already checked against the buffers.
inline int inflate_strip_serial(const uint8_t *src, const int64_t *strip, int wrapper, uint8_t *dst, Tables &T)
{
    SerialOut out{dst + strip[2]};
    return inflate_stream(src + strip[0], strip[1], strip[3], wrapper, T, out);
}

}  // namespace tip_inflate
