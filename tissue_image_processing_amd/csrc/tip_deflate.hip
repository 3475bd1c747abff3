// tip_deflate.hip -- deflate (RFC 1951) by runs, or by runs and matches to the row above, and CRC-32 of a device buffer, so that a label map or a type map leaves its
// GPU as the few kilobytes a `.seg` archive member holds instead of as 16 MB for the host's zlib (movie.save_seg).
//
// Stream (tests/deflate_restate.py is the same rule in Python, byte for byte).  The input is cut into chunks of 65536 bytes.
// A chunk becomes one fixed-Huffman block (BFINAL 0, BTYPE 01) and one empty stored block (header bits 000, then the padding to
// the byte boundary, then 00 00 FF FF: zlib's sync-flush marker), so chunks are whole bytes and concatenate; no block is
// final, the caller closes the stream (and may put a stored block in front).  Tokens: an element (elem_bytes = 1, 2 or 4)
// REPEATS when it equals the element before it in the same chunk.  The chunk is cut into segments of 256 bytes; inside a
// segment a maximal group of R bytes of repeating elements is ONE match (length R <= 256, distance elem_bytes) when
// R >= max(3, elem_bytes) and R literals otherwise; an element that does not repeat is elem_bytes literals.  A segment's
// first element may repeat the last one of the segment before, so a long run is a chain of 256-byte matches; the chunk's
// first element never repeats: no match reaches before its chunk.
//
// The ROWS rule (tip_deflate_rows; tests/deflate_rows_restate.py) keeps stream, chunks and segments and adds matches to the row
// above of a map whose rows are P = row_bytes long.  With e = elem_bytes and p a byte offset into the WHOLE buffer: R(p) is
// "repeats" as above; M_d(p), for the candidate distances d = P, P + e, P - e in this order, each kept only when e < d <= 32768,
// is p >= d and the element at p equals the one at p - d -- in an earlier chunk too, never before the buffer.  At p, with r and
// u_d the bytes of consecutive elements from p on, up to the segment's end, with R and with M_d, and (u, d*) the longest u_d (a
// tie goes to the earlier candidate): u >= max(4, e) and u > r gives one match (u, d*); else r >= max(3, e) one match (r, e);
// else the element's e literals.  A match is the length code, the 5-bit distance code and its extra bits, at most 8 + 5 + 5 + 13
// = 31 bits for at least 4 bytes: the bound is unchanged.  Without a kept candidate (P > 32768 + e) it is the run-only rule,
// and the run-only kernel runs.
//
// k_deflate_runs, k_deflate_rows: one workgroup (256 threads) per chunk, one thread per segment; they differ in the token rule
// alone (RunsRule: a byte walk with look-behind; RowsRule: bit masks of R and the M_d in registers, see there).
// k_deflate_dynamic (tip_deflate_dynamic) is either rule with another CODING of its tokens: per chunk a dynamic-Huffman block of
// the chunk's own codes where that is fewer bytes ("the dynamic coding", below); the steps here are shared.
//   stage    the chunk into LDS, segment t at dword 65 t: the threads then walk their segments in step, lane l reading dword
//            65 l + w -- bank (l + w) mod 32, all distinct within a 32-lane half (ds_read_b32), where the plain layout (stride
//            64 dwords) would put all 64 lanes on one bank.  The global reads are consecutive dwords.
//   count    every thread walks its segment once and adds up its tokens' bit lengths; a block scan gives its bit offset.
//   emit     the same walk again, tokens shifted into a 64-bit accumulator and OR-ed (LDS atomics) into the zeroed output
//            words 32 bits at a time -- neighbours share their boundary words, the OR merges them.
//   CRC      every thread takes the CRC-32 (zip / zlib: reflected polynomial 0xEDB88320, initial value and final XOR all
//            ones) of its segment from a 256-entry table built in LDS, then extends it by the zero bytes that stand for the
//            rest of the WHOLE buffer behind the segment: crc(A || B) = crc(A) * x^(8 |B|) + crc(B) over GF(2)[x] / P, and so
//            the buffer's CRC is the XOR of every segment's extended CRC.  One XOR per wave into LDS, one atomic per
//            workgroup into the result word.  x^(8 n) by square and multiply over the 32 constants x^(2^k) (df_powers).
//   store    the chunk's bytes go to its slot of a chunk-strided workspace (consecutive dwords), its size to sizes[chunk].
//   LDS: 16640 + 18435 + 264 dwords = 138 KiB of the CU's 160: one workgroup -- one wave per SIMD -- per CU, which a 2048^2
//   int32 map (256 chunks on 256 CUs) fills once.  Two workgroups per CU would need the output words to reuse the input's
//   space; measured on an MI355X (HIP events) the three launches take 0.09 ms for a 2048^2 int32 label map and
//   0.12 ms for its uint8 type map (64 chunks: a quarter of the CUs) beside a frame of 13 ms and more, so the plain layout stays.
// k_deflate_offsets: one workgroup scans the chunk sizes (exclusive, 64-bit) and leaves the total next to the CRC.
// k_deflate_compact: workgroup c copies chunk c's bytes from its slot to dst + offset[c] (byte offsets: byte copies).
// The entry then copies {total, crc} to pinned memory and waits for the stream once.
// k_deflate_strips (tip_deflate_strips; the strips section below): the same chunk encoder on every strip of a TIFF page as a
// buffer of its own, framed as a zlib stream with the strip's Adler-32 in place of the CRC (movie.export_tiff).
#include "tip_internal.h"

namespace tip {

constexpr int DF_CHUNK = 65536, DF_SEG = 256, DF_THREADS = DF_CHUNK / DF_SEG;
constexpr int DF_SEG_LD = DF_SEG / 4 + 1;                       // dwords between two segments in LDS
constexpr uint32_t DF_POLY = 0xEDB88320u;

// The most bytes a chunk of n input bytes takes: 3 header bits, at most 9 bits per byte (the longest literal; a match of
// R >= 3 bytes takes at most 8 + 5 + 5 bits, fewer than R literals), 7 bits of end-of-block, the 3 header bits of the
// stored block, the padding, LEN and NLEN.
__host__ __device__ constexpr long chunk_bound(long n) { return (3 + 9 * n + 7 + 3 + 7) / 8 + 4; }

// A strip's zlib stream (the strips section below) is a chunk with 78 01 in front and the final block and the Adler-32 behind.
constexpr int ZL_LEAD = 2, ZL_TAIL = 5 + 4;
__host__ __device__ constexpr long strip_bound(long n) { return (ZL_LEAD + chunk_bound(n) + ZL_TAIL + 1) & ~1L; }      // (even: strips start on words)

constexpr int DF_OUT_WORDS = (int)((ZL_LEAD + chunk_bound(DF_CHUNK) + ZL_TAIL + 3) / 4) + 1;      // LDS output words (+1: the accumulator's last flush)
constexpr int DF_IN_WORDS = DF_THREADS * DF_SEG_LD;
constexpr int DF_LDS_WORDS = DF_IN_WORDS + DF_OUT_WORDS + 256 + 8;

static long stream_bound(long nbytes)
{
    const long full = nbytes / DF_CHUNK, rest = nbytes % DF_CHUNK;
    return full * chunk_bound(DF_CHUNK) + (rest ? chunk_bound(rest) : 0);
}

// ---- GF(2)[x] / P in the CRC's reflected representation: bit 31 is x^0, bit 0 is x^31 ------------------------------------
// a * b: for every term x^i of a, add b * x^i; b * x is a shift towards bit 0, and the x^32 that falls out is replaced by
// P - x^32 (DF_POLY).
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if ((a >> (31 - i)) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? DF_POLY : 0u);
    }
    return p;
}

struct CrcPowers { uint32_t p[32]; };      // p[k] = x^(2^k); x^(2^32) = x, so the exponents' index wraps at 32

constexpr CrcPowers crc_powers()
{
    CrcPowers t{};
    t.p[0] = 1u << 30;                      // x^1
    for (int k = 1; k < 32; ++k) t.p[k] = gf_mul(t.p[k - 1], t.p[k - 1]);
    return t;
}

__device__ const CrcPowers df_powers = crc_powers();      // (worked out by the compiler)

// x^(8 n): the bits of n select the factors x^(2^(k + 3))
__device__ static inline uint32_t gf_x_pow_8n(unsigned long n)
{
    uint32_t p = 1u << 31;                  // x^0
    for (int k = 3; n; n >>= 1, ++k)
        if (n & 1ul) p = gf_mul(df_powers.p[k & 31], p);
    return p;
}

// ---- tokens ----------------------------------------------------------------------------------------------------------------
struct CountSink {
    uint32_t bits = 0;
    __device__ void put(uint32_t, int n) { bits += n; }
};

struct WordSink {                           // appends at a bit position of zeroed LDS words, least significant bit first
    uint32_t *words;
    uint64_t acc = 0;
    int nacc;
    uint32_t word;
    __device__ WordSink(uint32_t *w, uint32_t bitpos) : words(w), nacc((int)(bitpos & 31u)), word(bitpos >> 5) {}
    __device__ void put(uint32_t v, int n)  // n <= 31 (a row match) and nacc < 32: the accumulator never passes 63 bits
    {
        acc |= (uint64_t)v << nacc;
        nacc += n;
        if (nacc >= 32) {
            atomicOr(&words[word++], (uint32_t)acc);
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ void flush()
    {
        if (nacc > 0) atomicOr(&words[word], (uint32_t)acc);
    }
};

// Huffman codes enter the stream from their most significant bit: bit-reversed, then least significant bit first like the rest
template <class Sink> __device__ static inline void put_literal(Sink &s, uint32_t v)
{
    if (v < 144u) s.put(__brev(0x30u + v) >> 24, 8);
    else s.put(__brev(0x190u + (v - 144u)) >> 23, 9);
}

// the length symbol of a match of 3 <= len <= 256 bytes; eb, extra: its extra bits' count and value
__device__ static inline uint32_t length_symbol(int len, int &eb, uint32_t &extra)
{
    const uint32_t n = (uint32_t)len - 3u;
    eb = n < 8u ? 0 : (31 - __clz((int)n)) - 2;
    extra = n & ((1u << eb) - 1u);
    return n < 8u ? 257u + n : 261u + 4u * eb + ((n >> eb) & 3u);
}

// the length symbol in the fixed code and its extra bits; nb: their bit count (7 .. 13)
__device__ static inline uint32_t length_code(int len, int &nb)
{
    int eb;
    uint32_t extra, v;
    const uint32_t sym = length_symbol(len, eb, extra);
    if (sym < 280u) { v = __brev(sym - 256u) >> 25; nb = 7; }
    else { v = __brev(0xC0u + (sym - 280u)) >> 24; nb = 8; }
    v |= extra << nb;
    nb += eb;
    return v;
}

// ---- codings: what a token becomes.  A token rule hands its tokens to a coding: literal(sink, byte) and match(sink, len, k), k the
// match's distance -- 0, 1, 2: the rows rule's candidates in its order; 3: elem_bytes (a run).
// A candidate distance: d bytes (0: not kept), its fixed code -- five bits reversed, the extra bits behind them --, the bit count,
// and its distance symbol.
struct RowDist {
    int d;
    uint32_t code;
    int nbits;
    int sym;
};
struct RowDists {                           // P, P + E, P - E in the rule's order, at least one kept (row_bytes 0 on the host: none)
    RowDist c[3];
    long row_bytes;
};

template <int E> struct FixedCode {         // RFC 1951's fixed code: what the run-only and the rows kernel write
    const RowDists *dist = nullptr;           // the rows rule's candidates (k = 0, 1, 2); the run-only rule has none
    template <class Sink> __device__ __forceinline__ void literal(Sink &s, uint32_t v) const { put_literal(s, v); }
    template <class Sink> __device__ __forceinline__ void match(Sink &s, int len, int k) const
    {
        int nb;
        uint32_t v = length_code(len, nb);
        if (k == 3) {
            constexpr uint32_t dist_rev5 = E == 1 ? 0u : E == 2 ? 16u : 24u;   // distance codes 0, 1, 3 (distances 1, 2, 4), five bits reversed
            s.put(v | (dist_rev5 << nb), nb + 5);
        } else {
            const uint32_t code0 = dist->c[0].code, code1 = dist->c[1].code, code2 = dist->c[2].code;
            const int nbits0 = dist->c[0].nbits, nbits1 = dist->c[1].nbits, nbits2 = dist->c[2].nbits;
            v |= (k == 0 ? code0 : k == 1 ? code1 : code2) << nb;
            s.put(v, nb + (k == 0 ? nbits0 : k == 1 ? nbits1 : nbits2));      // at most 13 + 18
        }
    }
};

template <int E, class Code, class Sink> __device__ static inline void put_run(const Code &code, Sink &s, int run, uint32_t elem)
{
    if (run == 0) return;
    if (run >= (E > 3 ? E : 3)) { code.match(s, run, 3); return; }
    for (int i = 0; i < run; ++i) code.literal(s, (elem >> (8 * (i % E))) & 255u);      // (E = 1: run 1, 2; E = 2: run 2)
}

// one thread's segment: nb valid bytes (a multiple of E) at seg[0 ..]; prev: the element before it, when has_prev
template <int E, class Code, class Sink>
__device__ static inline void encode_segment(const Code &code, Sink &s, const uint32_t *seg, int nb, bool has_prev, uint32_t prev)
{
    constexpr uint32_t mask = E == 4 ? 0xFFFFFFFFu : (1u << (8 * (E & 3))) - 1u;
    int run = 0;
    for (int w = 0; 4 * w < nb; ++w) {
        const uint32_t d = seg[w];
#pragma unroll
        for (int k = 0; k < 4 / E; ++k) {
            if (4 * w + k * E < nb) {
                const uint32_t x = (d >> (8 * E * k % 32)) & mask;
                if (has_prev && x == prev) {
                    run += E;
                } else {
                    put_run<E>(code, s, run, prev);
                    run = 0;
#pragma unroll
                    for (int b = 0; b < E; ++b) code.literal(s, (x >> (8 * b)) & 255u);
                }
                prev = x;
                has_prev = true;
            }
        }
    }
    put_run<E>(code, s, run, prev);
}

template <int E> struct RunsRule {          // the run-only rule: nothing to prepare, the segment is walked byte by byte
    __device__ void set(const RowDists &) {}
    __device__ FixedCode<E> fixed_code() const { return FixedCode<E>(); }
    __device__ void prepare(const uint8_t *, long, long, const uint32_t *, int, bool, uint32_t) {}
    template <class Code, class Sink>
    __device__ void encode(const Code &code, Sink &s, const uint32_t *seg, int nb, bool has_prev, uint32_t prev) const
    {
        encode_segment<E>(code, s, seg, nb, has_prev, prev);
    }
};

// ---- the rows rule ---------------------------------------------------------------------------------------------------------
// one bit per element of the dword x: the element is zero (x: the XOR of two dwords -- their elements are equal)
template <int E> __device__ static inline uint32_t zero_elems(uint32_t x)
{
    if constexpr (E == 4) return x == 0u ? 1u : 0u;
    else if constexpr (E == 2) return ((x & 0xFFFFu) == 0u ? 1u : 0u) | ((x >> 16) == 0u ? 2u : 0u);
    else {
        // bit 7 of every byte that is not zero (the sum does not carry between bytes), inverted, then the four flags -- bits
        // 0, 8, 16, 24 -- gathered in bits 28 .. 31 by one product whose sixteen terms land on distinct bits
        const uint32_t nz = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
        return (((nz ^ 0x80808080u) >> 7) * 0x10204080u) >> 28;
    }
}

// the dword that starts E bytes before hi's first byte (lo: the dword before hi) and the one that starts E bytes behind lo's
template <int E> __device__ static inline uint32_t elem_before(uint32_t lo, uint32_t hi)
{
    if constexpr (E == 4) return lo;
    else return (lo >> (32 - 8 * E)) | (hi << (8 * E));
}
template <int E> __device__ static inline uint32_t elem_behind(uint32_t lo, uint32_t hi)
{
    if constexpr (E == 4) return hi;
    else return (lo >> (8 * E)) | (hi << (32 - 8 * E));
}

// the one bits of the mask m (W words, bit i: element i) in a row from bit pos on
template <int W> __device__ static inline int ones_from(const uint64_t (&m)[W], int pos)
{
    int n = 0;
    bool go = true;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int b = pos - 64 * k;           // the first bit of word k that counts (below 0: all of it)
        if (go && b < 64) {
            const int from = b > 0 ? b : 0, room = 64 - from;
            const uint64_t inv = ~m[k] >> from;      // (zeros enter at the top: the count is capped at the word's end)
            int c = inv ? __builtin_ctzll(inv) : 64;
            c = c < room ? c : room;
            n += c;
            go = c == room;
        }
    }
    return n;
}

// clears the bits of m outside [lo, hi)
template <int W> __device__ static inline void keep_bits(uint64_t (&m)[W], int lo, int hi)
{
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int l = lo - 64 * k, h = hi - 64 * k;
        const uint64_t below_h = h >= 64 ? ~0ul : h <= 0 ? 0ul : (1ul << h) - 1ul;
        const uint64_t below_l = l >= 64 ? ~0ul : l <= 0 ? 0ul : (1ul << l) - 1ul;
        m[k] &= below_h & ~below_l;
    }
}

// Eighteen dwords of the buffer from byte offset `off` on (any sign, any alignment); bytes outside the buffer read as zero.
__device__ static inline void load_above(const uint8_t *src, long nbytes, long off, uint32_t (&a)[18])
{
    if (off >= 0 && off + 72 <= nbytes && (((uintptr_t)src + (uintptr_t)off) & 3u) == 0) {
        const uint32_t *p = (const uint32_t *)(src + off);
#pragma unroll
        for (int i = 0; i < 18; ++i) a[i] = p[i];
    } else {
#pragma unroll
        for (int i = 0; i < 18; ++i) {
            uint32_t d = 0;
            for (int b = 0; b < 4; ++b) {
                const long o = off + 4 * i + b;
                if (o >= 0 && o < nbytes) d |= (uint32_t)src[o] << (8 * b);
            }
            a[i] = d;
        }
    }
}

// The rows rule (this file's head): per thread one bit per element of its segment for R -- the element repeats -- and for each
// candidate distance -- the element equals the one d bytes before it in the BUFFER -- kept in registers (64 bits each for
// int32, 256 for uint8); the walk is then count-the-ones arithmetic on the four masks, the same for both sinks.
// The masks are built sixteen dwords at a time.  The three distances differ by one element, so ONE span of the row above --
// the sixteen dwords at p - P and one dword either side -- serves all three: plain dword loads when the span lies inside the
// buffer and is dword-aligned (an int32 map; a uint8 map whose row is a multiple of 4), byte loads otherwise.  The guard
// p >= d is applied to the finished masks, so whatever the loads return before the buffer's first byte (zero) never counts.
template <int E> struct RowsRule {
    static constexpr int W = 4 / E;          // 64-bit words of a mask: 256 / E elements
    static constexpr int NE = 4 / E;         // elements of a dword
    RowDists dist;
    uint64_t r[W], m[3][W];

    __device__ void set(const RowDists &d) { dist = d; }
    __device__ FixedCode<E> fixed_code() const
    {
        FixedCode<E> f;
        f.dist = &dist;
        return f;
    }

    __device__ __forceinline__ void prepare(const uint8_t *src, long nbytes, long at, const uint32_t *seg, int nb, bool has_prev, uint32_t prev)
    {
#pragma unroll
        for (int j = 0; j < W; ++j) r[j] = m[0][j] = m[1][j] = m[2][j] = 0;
        if (nb <= 0) return;
        uint32_t before = prev << (32 - 8 * E);               // (a dword whose last element is the one before the segment)
#pragma unroll 1
        for (int g = 0; 64 * g < nb; ++g) {
            uint32_t a[18];                                     // the row above: dwords -1 .. 16 of this group's
            load_above(src, nbytes, at - dist.row_bytes + 64 * g - 4, a);
            uint64_t br = 0, b0 = 0, b1 = 0, b2 = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t x = seg[16 * g + i];
                br |= (uint64_t)zero_elems<E>(x ^ elem_before<E>(before, x)) << (NE * i);
                before = x;
                b0 |= (uint64_t)zero_elems<E>(x ^ a[i + 1]) << (NE * i);
                b1 |= (uint64_t)zero_elems<E>(x ^ elem_before<E>(a[i], a[i + 1])) << (NE * i);
                b2 |= (uint64_t)zero_elems<E>(x ^ elem_behind<E>(a[i + 1], a[i + 2])) << (NE * i);
            }
            const int bit = 16 * NE * g;                        // the group's first element
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (j == (bit >> 6)) {
                    r[j] |= br << (bit & 63);
                    m[0][j] |= b0 << (bit & 63);
                    m[1][j] |= b1 << (bit & 63);
                    m[2][j] |= b2 << (bit & 63);
                }
        }
        keep_bits(r, has_prev ? 0 : 1, nb / E);                 // the chunk's first element never repeats
        keep_from(m[0], dist.c[0].d, at, nb);                   // M_d needs p >= d, and a distance that is kept
        keep_from(m[1], dist.c[1].d, at, nb);
        keep_from(m[2], dist.c[2].d, at, nb);
    }

    // clears, in the mask of distance d, the elements before byte d of the buffer (all when d is 0: not kept)
    __device__ static __forceinline__ void keep_from(uint64_t (&mk)[W], int d, long at, int nb)
    {
        const long first = (long)d - at;                        // the segment's first byte with p >= d
        keep_bits(mk, d == 0 || first >= nb ? nb / E : first > 0 ? (int)first / E : 0, nb / E);
    }

    template <class Code, class Sink>
    __device__ __forceinline__ void encode(const Code &code, Sink &s, const uint32_t *seg, int nb, bool, uint32_t) const
    {
        constexpr uint32_t mask = E == 4 ? 0xFFFFFFFFu : (1u << (8 * (E & 3))) - 1u;
        for (int pos = 0; pos < nb / E;) {
            const int run = ones_from(r, pos), u1 = ones_from(m[1], pos), u2 = ones_from(m[2], pos);
            int u = ones_from(m[0], pos), k = 0;                // the longest; a tie stays with the earlier distance
            if (u1 > u) { u = u1; k = 1; }
            if (u2 > u) { u = u2; k = 2; }
            if (u * E >= 4 && u > run) {
                code.match(s, u * E, k);
                pos += u;
            } else if (run * E >= (E > 3 ? E : 3)) {
                code.match(s, run * E, 3);
                pos += run;
            } else {
                const uint32_t x = (seg[(pos * E) >> 2] >> (8 * ((pos * E) & 3))) & mask;
#pragma unroll
                for (int b = 0; b < E; ++b) code.literal(s, (x >> (8 * b)) & 255u);
                pos += 1;
            }
        }
    }
};

// ---- the dynamic coding (tip_deflate_dynamic; tests/deflate_dynamic_restate.py is its specification) -------------------------
// Per chunk the tokens -- the rule's, unchanged -- are written either as above or as one dynamic-Huffman block (BTYPE 10) with the
// chunk's own literal/length and distance codes, whichever gives fewer bytes (a tie: the fixed form), so no chunk grows and the
// bound stays.  Code lengths: the used symbols ranked by (count, symbol); Huffman's tree by two queues (leaves in rank order,
// internal nodes as made; the leaf on equal weights); the leaves counted per depth, depths above 15 at 15 and then repaired
// (bl[15] -= 1, the deepest d < 15 with leaves: bl[d] -= 1, bl[d + 1] += 2, until Kraft's sum is 1); lengths handed out by rank,
// longest first; one used symbol gets length 1; canonical codes.  Header: HLIT, HDIST trimmed, the lengths as one sequence, zero
// runs as symbols 18 (while 11 or more remain) and 17 (3 .. 10), never 16, under a CONSTANT code-length code (4 bits for 0 .. 11,
// 17, 18; 5 bits for 12 .. 15), so HCLEN is 19 and the first 17 + 57 bits differ between blocks in HLIT and HDIST alone.
// Steps of k_deflate_dynamic behind the staging: walk 1 counts every thread's symbols into LDS and its fixed bits; the counters
// add up; lengths, codes, header and both sizes; the choice; then the fixed kernels' scan and emitting walk -- with, for a
// dynamic chunk, one more counting walk in between, whose bits and the emitting walk's come from the code table.
// Histogram: a map's few dominant symbols would put a wave's lanes on one LDS counter (same-address atomics serialise), so there
// are 32 copies of the 316 counters, copy (lane mod 32) at word 32 symbol + copy: the lanes of a 32-lane half hit 32 distinct
// banks whatever their symbols, and a counter is shared by two lanes of each wave.  The copies, the sort and the tree live in the
// output words, which are zeroed again before anything is emitted; only the code table (288 words), the four distances' codes,
// the header (64 words) and a few counters are kept beside them: 1.5 KB more LDS than the fixed kernels.
// The tree's merge (at most 285 steps), the repair and the header's run-length walk (at most 316 steps) are one lane's work.
constexpr int DY_LIT = 286, DY_SYMS = DY_LIT + 30, DY_REPS = 32;
constexpr int DY_CNT = DY_SYMS * DY_REPS, DY_LEN = DY_CNT + 320, DY_SORT = DY_LEN + 320;      // scratch, in the output words
constexpr int DY_SORT_WORDS = 288 + 288 + 288 + 576 + 64;                                       // sw, ssym, iw, parent, bl
constexpr int DY_DTAB = DY_SORT + DY_SORT_WORDS, DY_SCRATCH = DY_DTAB + 32;
static_assert(DY_SCRATCH <= DF_OUT_WORDS, "the dynamic coding's scratch lies in the output words");
constexpr int DY_TAB = 0, DY_DIST = 288, DY_HDR = 296, DY_MISC = 360, DY_WORDS = 376;         // kept, behind misc
enum { DM_HLIT = 0, DM_HDIST, DM_BITS, DM_HDR_BITS, DM_LIMITED };

// the code-length code's constant table: symbol -> code, reversed, in bits 0 .. 4, its length in bits 8 ..
__device__ static inline uint32_t cl_code(uint32_t sym)
{
    if (sym < 12u) return (__brev(sym) >> 28) | (4u << 8);
    if (sym < 16u) return (__brev(28u + (sym - 12u)) >> 27) | (5u << 8);
    return (__brev(sym - 5u) >> 28) | (4u << 8);                 // 17, 18: the 4-bit codes 12, 13
}

// The lengths of one alphabet from its counts (this section's head), and its table: tab[s] = the canonical code, reversed, with
// the length in bits 16 ..; 0 for an unused symbol.  All 256 threads call it; scr: DY_SORT_WORDS of scratch.
__device__ static void code_lengths(const uint32_t *cnt, int nsym, uint32_t *len, uint32_t *tab, uint32_t *scr, uint32_t *limited)
{
    uint32_t *sw = scr, *ssym = scr + 288, *iw = scr + 576, *parent = scr + 864, *bl = scr + 1440, *lstart = bl + 16, *first = bl + 32,
             *over = bl + 48;
    const int t = threadIdx.x;
    int n = 0;
    for (int s = t; s == t || s < nsym; s += DF_THREADS) {      // (every thread runs the first round: it learns n)
        const uint32_t c = s < nsym ? cnt[s] : 0u;
        int r = 0, used = 0;
        for (int j = 0; j < nsym; ++j) {
            const uint32_t cj = cnt[j];
            used += cj != 0u;
            r += cj != 0u && (cj < c || (cj == c && j < s));
        }
        n = used;
        if (s < nsym) {
            len[s] = 0;
            if (c) { sw[r] = c; ssym[r] = (uint32_t)s; }
        }
    }
    if (t < 64) bl[t] = 0;
    __syncthreads();
    if (n == 1 && t == 0) bl[1] = 1;
    if (n >= 2) {
        if (t == 0) {                         // two queues: A the leaves 0 .. n - 1, B the internal nodes n .. as they are made
            int a = 0, b = 0;
            uint32_t wa = sw[0], wb = ~0u;
            for (int made = 0; made < n - 1; ++made) {
                uint32_t sum = 0;
                for (int k = 0; k < 2; ++k) {
                    if (wa <= wb) {
                        sum += wa;
                        parent[a] = (uint32_t)(n + made);
                        ++a;
                        wa = a < n ? sw[a] : ~0u;
                    } else {
                        sum += wb;
                        parent[n + b] = (uint32_t)(n + made);
                        ++b;
                        wb = b < made ? iw[b] : ~0u;
                    }
                }
                iw[made] = sum;
                if (b == made) wb = sum;      // (B was empty: the new node is its head)
            }
        }
        __syncthreads();
        for (int r = t; r < n; r += DF_THREADS) {
            int d = 0;
            for (uint32_t x = (uint32_t)r; x != (uint32_t)(2 * n - 2); x = parent[x]) ++d;
            if (d > 15) { *over = 1u; d = 15; }
            atomicAdd(&bl[d], 1u);
        }
        __syncthreads();
        if (t == 0 && *over) {
            *limited = 1u;
            uint32_t kraft = 0;
            for (int d = 1; d <= 15; ++d) kraft += bl[d] << (15 - d);
            for (; kraft > (1u << 15); --kraft) {
                bl[15] -= 1u;
                for (int d = 14; d >= 1; --d)
                    if (bl[d]) { bl[d] -= 1u; bl[d + 1] += 2u; break; }
            }
        }
    }
    if (t == 0) {
        uint32_t rank = 0, code = 0;
        for (int d = 15; d >= 1; --d) { lstart[d] = rank; rank += bl[d]; }
        for (int d = 1; d <= 15; ++d) { code = (code + bl[d - 1]) << 1; first[d] = code; }      // (bl[0] is 0)
    }
    __syncthreads();
    for (int r = t; r < n; r += DF_THREADS)
        for (int d = 15; d >= 1; --d)
            if ((uint32_t)r - lstart[d] < bl[d]) len[ssym[r]] = (uint32_t)d;
    __syncthreads();
    for (int s = t; s < nsym; s += DF_THREADS) {
        const uint32_t l = len[s];
        uint32_t e = 0;
        if (l) {
            uint32_t k = 0;
            for (int j = 0; j < s; ++j) k += len[j] == l;
            e = (__brev(first[l] + k) >> (32 - l)) | (l << 16);
        }
        tab[s] = e;
    }
    __syncthreads();
}

// the header of a dynamic block into the zeroed words hdr; returns its bits.  One lane's work.
__device__ static uint32_t dynamic_header(uint32_t *hdr, const uint32_t *len, int hlit, int hdist)
{
    // the code-length code's lengths in the order 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 -- 0, eleven
    // times 4, then 5, 4, 5, 4, 5, 4, 5 --, three bits each, the first in the lowest bits: octal, read from the right
    constexpr uint32_t order_lo = 04444444440u, order_hi = 0545454544u;      // ten and nine of them
    WordSink s(hdr, 0u);
    uint32_t bits = 0;
    auto put = [&](uint32_t v, int n) { s.put(v, n); bits += (uint32_t)n; };
    put(4u, 3);                               // BFINAL 0, then BTYPE 10 least significant bit first
    put((uint32_t)(hlit - 257), 5);
    put((uint32_t)(hdist - 1), 5);
    put(19u - 4u, 4);
    put(order_lo, 30);
    put(order_hi, 27);
    const int total = hlit + hdist;
    auto at = [&](int i) { return i < hlit ? len[i] : len[DY_LIT + (i - hlit)]; };
    for (int i = 0; i < total;) {
        const uint32_t l = at(i);
        if (l) {
            const uint32_t c = cl_code(l);
            put(c & 31u, (int)(c >> 8));
            ++i;
            continue;
        }
        int n = 1;
        while (i + n < total && at(i + n) == 0u) ++n;
        i += n;
        while (n >= 11) {
            const int m = n < 138 ? n : 138;
            put((cl_code(18u) & 31u) | ((uint32_t)(m - 11) << 4), 4 + 7);
            n -= m;
        }
        if (n >= 3) {
            put((cl_code(17u) & 31u) | ((uint32_t)(n - 3) << 4), 4 + 3);
        } else {
            for (; n > 0; --n) put(cl_code(0u) & 31u, 4);
        }
    }
    s.flush();
    return bits;
}

// the extra bits of a literal/length symbol (s < DY_LIT) or of the distance symbol s - DY_LIT
__device__ static inline uint32_t symbol_extra_bits(int s)
{
    if (s < DY_LIT) return s < 265 || s == 285 ? 0u : (uint32_t)(s - 261) >> 2;
    const int d = s - DY_LIT;
    return d < 4 ? 0u : (uint32_t)(d >> 1) - 1u;
}

template <int E> struct HistCode {          // walk 1: counts the symbols in this lane's copy, and the fixed form's bits
    FixedCode<E> fixed;
    uint32_t *hist;                           // this lane's copy: symbol s at hist[DY_REPS s]
    const RowDists *dist;                     // the candidates: their distance symbols
    template <class Sink> __device__ __forceinline__ void literal(Sink &s, uint32_t v) const
    {
        atomicAdd(&hist[DY_REPS * v], 1u);
        fixed.literal(s, v);
    }
    template <class Sink> __device__ __forceinline__ void match(Sink &s, int len, int k) const
    {
        int eb;
        uint32_t extra;
        atomicAdd(&hist[DY_REPS * length_symbol(len, eb, extra)], 1u);
        const int sym0 = dist->c[0].sym, sym1 = dist->c[1].sym, sym2 = dist->c[2].sym;
        atomicAdd(&hist[DY_REPS * (DY_LIT + (k == 0 ? sym0 : k == 1 ? sym1 : k == 2 ? sym2 : E - 1))], 1u);
        fixed.match(s, len, k);
    }
};

struct DynCode {                            // the chunk's own codes, in LDS
    const uint32_t *tab;                      // symbol -> code, reversed, and its length in bits 16 ..
    const uint32_t *dist;                     // [k]: distance k's code, reversed, with its extra bits behind it; [4 + k]: the bit count
    template <class Sink> __device__ __forceinline__ void literal(Sink &s, uint32_t v) const
    {
        const uint32_t e = tab[v];
        s.put(e & 0xFFFFu, (int)(e >> 16));
    }
    template <class Sink> __device__ __forceinline__ void match(Sink &s, int len, int k) const
    {
        int eb;
        uint32_t extra;
        const uint32_t e = tab[length_symbol(len, eb, extra)];
        s.put((e & 0xFFFFu) | (extra << (e >> 16)), (int)(e >> 16) + eb);                      // at most 15 + 5
        s.put(dist[k], (int)dist[4 + k]);                                                      // at most 15 + 13
    }
};

// One chunk by one workgroup (this file's head): what all the kernels are, but for the token rule and the coding (DYN: the
// dynamic coding's section above; dists: the rule's candidates once more, or zeros).  The chunk is the DF_CHUNK bytes from
// `base` on of the buffer (src, nbytes) -- the bytes the rule's matches may reach into; its stream goes to `slot`, the stream's size
// to *size_out.  ZLIB false: the buffer's CRC-32 is folded into *sum_out.  ZLIB true (the strips section below: the buffer IS the
// chunk): the stream is a whole zlib stream -- 78 01 in front, which shifts every bit by ZL_LEAD bytes, the final empty stored block
// and the chunk's Adler-32 behind -- and sum_out is not used.
template <int E, bool DYN, bool ZLIB, class Rule>
__device__ static __forceinline__ void deflate_chunk(Rule &rule, const RowDists &dists, const uint8_t *__restrict__ src, long nbytes, long base,
                                                     int aligned, uint32_t *__restrict__ slot, uint32_t *__restrict__ size_out,
                                                     uint32_t *__restrict__ sum_out)
{
    extern __shared__ uint32_t df_lds[];
    uint32_t *in = df_lds, *out = df_lds + DF_IN_WORDS, *crctab = out + DF_OUT_WORDS, *misc = crctab + 256;
    [[maybe_unused]] uint32_t *kept = misc + 8, *dm = kept + DY_MISC;      // (DYN only: DY_WORDS more)
    const int t = threadIdx.x;
    const int L = (int)(nbytes - base < DF_CHUNK ? nbytes - base : DF_CHUNK);      // 1 .. 65536, a multiple of E
    const uint8_t *chunk = src + base;
    constexpr uint32_t lead = ZLIB ? 8u * ZL_LEAD : 0u;      // the bits in front of the first block

    for (int i = t; 4 * i < L; i += DF_THREADS) {
        uint32_t d;
        if (aligned && 4 * i + 4 <= L) {
            d = ((const uint32_t *)chunk)[i];
        } else {                              // an unaligned buffer, or the bytes behind the last whole dword
            d = 0;
            for (int b = 0; b < 4 && 4 * i + b < L; ++b) d |= (uint32_t)chunk[4 * i + b] << (8 * b);
        }
        in[(i >> 6) * DF_SEG_LD + (i & 63)] = d;
    }
    const int out_words = (int)((chunk_bound(L) + (ZLIB ? ZL_LEAD + ZL_TAIL : 0) + 3) / 4) + 1;
    const int zero_words = DYN && out_words < DY_SCRATCH ? DY_SCRATCH : out_words;      // (DYN: its scratch starts from zeros too)
    for (int i = t; i < zero_words; i += DF_THREADS) out[i] = 0;
    if constexpr (!ZLIB) {
        uint32_t c = (uint32_t)t;             // the CRC of the one byte t: eight steps of the bitwise definition
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? DF_POLY : 0u);
        crctab[t] = c;
    }
    if (t < 8) misc[t] = 0;                   // [0..3] the waves' bit totals, [4] the workgroup's CRC (ZLIB: [4], [5] the Adler sums)
    if constexpr (DYN) {
        for (int i = t; i < DY_WORDS; i += DF_THREADS) kept[i] = 0;
    }
    __syncthreads();

    const int first = t * DF_SEG;
    const int nb = L - first < 0 ? 0 : (L - first < DF_SEG ? L - first : DF_SEG);
    const uint32_t *seg = in + t * DF_SEG_LD;
    const bool has_prev = t > 0 && nb > 0;
    const uint32_t prev = has_prev ? in[(t - 1) * DF_SEG_LD + 63] >> (32 - 8 * E) : 0u;      // the segment before is full
    const int lane = t & 63, wave = t >> 6;
    // exclusive block scan of the bit counts: within the wave by shuffles, across the four waves through LDS.  (This function keeps
    // its scan and its three reductions by hand: with tip_wave.h's block_exclusive_scan and wave_reduce the compiler orders the
    // code of the kernels around it differently, and these kernels are the archive's time.)
    auto scan = [&](uint32_t bits, uint32_t &before, uint32_t &total) {
        uint32_t incl = bits;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) misc[wave] = incl;
        __syncthreads();
        before = incl - bits;
        total = 0;
        for (int w = 0; w < DF_THREADS / 64; ++w) {
            if (w < wave) before += misc[w];
            total += misc[w];
        }
    };

    rule.prepare(src, nbytes, base + first, seg, nb, has_prev, prev);
    CountSink cs;
    uint32_t before, total, head = lead + 3u, eob_bits = 7u;      // head: the bits in front of the first token; the fixed end of block: seven zeros
    bool dynamic = false;
    DynCode dyn{};
    if constexpr (DYN) {
        HistCode<E> hc{rule.fixed_code(), out + (t & (DY_REPS - 1)), &dists};
        rule.encode(hc, cs, seg, nb, has_prev, prev);
        scan(cs.bits, before, total);         // (its barrier: the counters are complete)
        uint32_t *cnt = out + DY_CNT, *len = out + DY_LEN, *dtab = out + DY_DTAB;
        for (int s = t; s < DY_SYMS; s += DF_THREADS) {
            uint32_t c = 0;
            for (int j = 0; j < DY_REPS; ++j) c += out[DY_REPS * s + ((j + s) & (DY_REPS - 1))];      // (rotated: distinct banks)
            cnt[s] = s == 256 ? 1u : c;       // the end of block, once
        }
        __syncthreads();
#ifndef DF_TIME_SKIP_CODES                    // (a timing build leaves the construction and the header out: tools/deflate_dynamic_time.py --lib)
        code_lengths(cnt, DY_LIT, len, kept + DY_TAB, out + DY_SORT, &dm[DM_LIMITED]);
        code_lengths(cnt + DY_LIT, DY_SYMS - DY_LIT, len + DY_LIT, dtab, out + DY_SORT, &dm[DM_LIMITED]);
#endif
        uint32_t bits = 0;
        for (int s = t; s < DY_SYMS; s += DF_THREADS) {
            if (len[s]) atomicMax(&dm[s < DY_LIT ? DM_HLIT : DM_HDIST], (uint32_t)(s < DY_LIT ? s : s - DY_LIT) + 1u);
            bits += cnt[s] * (len[s] + symbol_extra_bits(s));
        }
        for (int d = 32; d >= 1; d >>= 1) bits += __shfl_xor(bits, d, 64);
        if (lane == 0) atomicAdd(&dm[DM_BITS], bits);
        if (t < 4) {                          // the four distances' codes: the rule's candidates, then elem_bytes
            const RowDist rd = t < 3 ? dists.c[t] : RowDist{E, 0u, 5, E - 1};
            const uint32_t e = rd.d ? dtab[rd.sym] : 0u;
            kept[DY_DIST + t] = (e & 0xFFFFu) | ((rd.code >> 5) << (e >> 16));
            kept[DY_DIST + 4 + t] = (e >> 16) + (uint32_t)(rd.nbits - 5);
        }
        __syncthreads();
#ifndef DF_TIME_SKIP_CODES
        if (t == 0) {
            const uint32_t hlit = dm[DM_HLIT] < 257u ? 257u : dm[DM_HLIT], hdist = dm[DM_HDIST] < 1u ? 1u : dm[DM_HDIST];
            dm[DM_HDR_BITS] = dynamic_header(kept + DY_HDR, len, (int)hlit, (int)hdist);
        }
#endif
        __syncthreads();
        // both forms' bytes, the stored block included (DM_BITS counts the end-of-block code too); a tie goes to the fixed form
        const uint32_t fixed_bytes = (3u + total + 7u + 3u + 7u) / 8u + 4u, dynamic_bytes = (dm[DM_HDR_BITS] + dm[DM_BITS] + 3u + 7u) / 8u + 4u;
        dynamic = dynamic_bytes < fixed_bytes;
        dyn = DynCode{kept + DY_TAB, kept + DY_DIST};
        __syncthreads();                      // (everyone has read the scratch)
        for (int i = t; i < (out_words < DY_SCRATCH ? out_words : DY_SCRATCH); i += DF_THREADS) out[i] = 0;
        if (dynamic) {
            cs.bits = 0;
            rule.encode(dyn, cs, seg, nb, has_prev, prev);
            scan(cs.bits, before, total);
            head = lead + dm[DM_HDR_BITS];
            eob_bits = kept[DY_TAB + 256] >> 16;
        } else {
            __syncthreads();                  // the output words are zero again
        }
    } else {
        rule.encode(rule.fixed_code(), cs, seg, nb, has_prev, prev);
        scan(cs.bits, before, total);
    }

    WordSink ws(out, dynamic || t > 0 ? head + before : lead);
    if constexpr (ZLIB) {
        if (t == 0) atomicOr(&out[0], 0x0178u);      // CMF 78: deflate, a 32 KB window; FLG 01: no dictionary, level 0, and 0x7801 a multiple of 31
    }
    if (dynamic) {
        if (t < 64 && kept[DY_HDR + t]) {
            const uint64_t h = (uint64_t)kept[DY_HDR + t] << lead;      // (the header's words, moved behind the lead)
            atomicOr(&out[t], (uint32_t)h);
            if (lead && (uint32_t)(h >> 32)) atomicOr(&out[t + 1], (uint32_t)(h >> 32));
        }
        rule.encode(dyn, ws, seg, nb, has_prev, prev);
        if (t == 0) {
            ws.flush();
            ws = WordSink(out, head + total);
            ws.put(kept[DY_TAB + 256] & 0xFFFFu, (int)eob_bits);
        }
    } else {
        if (t == 0) ws.put(2u, 3);            // BFINAL 0, then BTYPE 01 least significant bit first
        rule.encode(rule.fixed_code(), ws, seg, nb, has_prev, prev);
    }
    ws.flush();
    // the fixed end of block (seven zero bits) and the stored block's header (three) are zeros already; behind the padding LEN = 0, NLEN = FFFF
    const uint32_t body = (head + total + eob_bits + 3u + 7u) / 8u, size = body + 4u;
    if (t == 0) {
        atomicOr(&out[(body + 2u) >> 2], 0xFFu << (8u * ((body + 2u) & 3u)));
        atomicOr(&out[(body + 3u) >> 2], 0xFFu << (8u * ((body + 3u) & 3u)));
    }

    if constexpr (ZLIB) {
        // Adler-32 (RFC 1950) of the L bytes x_0 ..: s1 = 1 + sum x_i, s2 = L + sum (L - i) x_i, both modulo 65521.  A thread's
        // share is its segment's two sums with the weights counted from the segment's end, moved to the chunk's end by
        // (bytes behind the segment) * (its plain sum); one add per wave into LDS.
        uint32_t s1 = 0;
        uint64_t s2 = 0;
        for (int w = 0; 4 * w < nb; ++w) {
            const uint32_t d = seg[w];
            for (int b = 0; b < 4 && 4 * w + b < nb; ++b) {
                const uint32_t x = (d >> (8 * b)) & 255u;
                s1 += x;
                s2 += (uint32_t)(nb - (4 * w + b)) * x;
            }
        }
        if (nb > 0) s2 += (uint64_t)(uint32_t)(L - (first + nb)) * s1;      // below 2^33
        uint32_t a = s1 % 65521u, b = (uint32_t)(s2 % 65521u);
        for (int d = 32; d >= 1; d >>= 1) {
            a += __shfl_xor(a, d, 64);
            b += __shfl_xor(b, d, 64);
        }
        if (lane == 0) {
            atomicAdd(&misc[4], a);
            atomicAdd(&misc[5], b);
        }
        __syncthreads();                      // the output words and the sums are complete
        if (t == 0) {                         // the final block 01 00 00 FF FF and the Adler-32, most significant byte first
            const uint32_t adler = (((uint32_t)L + misc[5]) % 65521u) << 16 | ((1u + misc[4]) % 65521u);
            const uint32_t tail[ZL_TAIL] = {1u, 0u, 0u, 0xFFu, 0xFFu, adler >> 24, (adler >> 16) & 255u, (adler >> 8) & 255u, adler & 255u};
            for (uint32_t i = 0; i < (uint32_t)ZL_TAIL; ++i) out[(size + i) >> 2] |= tail[i] << (8u * ((size + i) & 3u));
        }
        __syncthreads();
        const uint32_t whole = size + (uint32_t)ZL_TAIL;
        for (uint32_t i = t; 4u * i < whole; i += DF_THREADS) slot[i] = out[i];
        if (t == 0) *size_out = whole;
    } else {
        uint32_t part = 0;
        if (nb > 0) {
            uint32_t c = 0xFFFFFFFFu;
            for (int w = 0; 4 * w < nb; ++w) {
                const uint32_t d = seg[w];
                for (int b = 0; b < 4 && 4 * w + b < nb; ++b) c = crctab[(c ^ (d >> (8 * b))) & 255u] ^ (c >> 8);
            }
            part = gf_mul(~c, gf_x_pow_8n((unsigned long)(nbytes - (base + first + nb))));
        }
        for (int d = 32; d >= 1; d >>= 1) part ^= __shfl_xor(part, d, 64);
        if (lane == 0) atomicXor(&misc[4], part);
        __syncthreads();                      // the output words and the CRC are complete

        for (uint32_t i = t; 4u * i < size; i += DF_THREADS) slot[i] = out[i];
        if (t == 0) {
            *size_out = size;
            atomicXor(sum_out, misc[4]);
        }
    }
}

// the chunk of workgroup blockIdx.x of a whole buffer, into its slot of the chunk-strided workspace
template <int E, bool DYN, class Rule>
__device__ static __forceinline__ void deflate_own_chunk(Rule &rule, const RowDists &dists, const uint8_t *__restrict__ src, long nbytes, int aligned,
                                                         uint32_t *__restrict__ slots, uint32_t *__restrict__ sizes,
                                                         uint32_t *__restrict__ crc_out)
{
    deflate_chunk<E, DYN, false>(rule, dists, src, nbytes, (long)blockIdx.x * DF_CHUNK, aligned, slots + (size_t)blockIdx.x * DF_OUT_WORDS,
                                 sizes + blockIdx.x, crc_out);
}

template <int E>
__global__ __launch_bounds__(DF_THREADS) void k_deflate_runs(const uint8_t *__restrict__ src, long nbytes, int aligned,
                                                             uint32_t *__restrict__ slots, uint32_t *__restrict__ sizes,
                                                             uint32_t *__restrict__ crc_out)
{
    RunsRule<E> rule;
    deflate_own_chunk<E, false>(rule, RowDists{}, src, nbytes, aligned, slots, sizes, crc_out);
}

template <int E>
__global__ __launch_bounds__(DF_THREADS) void k_deflate_rows(const uint8_t *__restrict__ src, long nbytes, int aligned, RowDists dist,
                                                             uint32_t *__restrict__ slots, uint32_t *__restrict__ sizes,
                                                             uint32_t *__restrict__ crc_out)
{
    RowsRule<E> rule;
    rule.set(dist);
    deflate_own_chunk<E, false>(rule, dist, src, nbytes, aligned, slots, sizes, crc_out);
}

// either rule with the dynamic coding (dist: all zero with RunsRule)
template <int E, class Rule>
__global__ __launch_bounds__(DF_THREADS) void k_deflate_dynamic(const uint8_t *__restrict__ src, long nbytes, int aligned, RowDists dist,
                                                                uint32_t *__restrict__ slots, uint32_t *__restrict__ sizes,
                                                                uint32_t *__restrict__ crc_out)
{
    Rule rule;
    rule.set(dist);
    deflate_own_chunk<E, true>(rule, dist, src, nbytes, aligned, slots, sizes, crc_out);
}

// ---- strips (tip_deflate_strips; tests/deflate_strips_restate.py) -----------------------------------------------------------------
// The pages of a TIFF are cut into strips of rows_per_strip rows, every strip a zlib stream of its own (RFC 1950) that a reader
// inflates without any other: 78 01, the body, the final empty stored block 01 00 00 FF FF, the strip's Adler-32.  The body is what
// the rows entry (codes 0) or the dynamic entry (codes 1) writes for the strip as a WHOLE BUFFER, so a strip is one chunk -- at
// most 65536 bytes -- and no match reaches before it: deflate_chunk with the strip as its buffer (ZLIB).  Strips are handed out
// like the inflate kernel's: workgroup g of G takes strips g, g + G, ... -- the trip count comes from the block number alone.
struct StripPlan {
    long rows, row_bytes, rows_per_strip, strips_per_page, n_strips;
    int slot_words;                           // words between two strips' slots: the longest strip's bound
};

template <int E, bool DYN, class Rule>
__global__ __launch_bounds__(DF_THREADS) void k_deflate_strips(const uint8_t *__restrict__ src, StripPlan plan, RowDists dist,
                                                               uint32_t *__restrict__ slots, uint32_t *__restrict__ sizes)
{
    Rule rule;
    rule.set(dist);
    for (long s = blockIdx.x; s < plan.n_strips; s += gridDim.x) {
        const long page = s / plan.strips_per_page, row0 = (s % plan.strips_per_page) * plan.rows_per_strip;
        const long nrows = plan.rows - row0 < plan.rows_per_strip ? plan.rows - row0 : plan.rows_per_strip;
        const uint8_t *strip = src + (page * plan.rows + row0) * plan.row_bytes;
        deflate_chunk<E, DYN, true>(rule, dist, strip, nrows * plan.row_bytes, 0, (int)(((uintptr_t)strip & 3u) == 0),
                                    slots + (size_t)s * plan.slot_words, sizes + s, nullptr);
        __syncthreads();                      // (the next strip is staged over this one's words)
    }
}

// offsets[c] = sizes[0] + ... + sizes[c - 1]; *total = the sum.  One workgroup, 256 chunks per step.  even: every size counts
// rounded up to an even number (strips start on word boundaries).  table, when given: (offset, size) per chunk as int64 pairs,
// the total behind them.
__global__ __launch_bounds__(256) void k_deflate_offsets(const uint32_t *__restrict__ sizes, long n, unsigned long *__restrict__ offsets,
                                                         unsigned long *__restrict__ total, int even, long *__restrict__ table)
{
    __shared__ unsigned long wave_sums[4];
    const int t = threadIdx.x;
    unsigned long carry = 0;
    for (long c0 = 0; c0 < n; c0 += 256) {
        const unsigned long v = c0 + t < n ? (sizes[c0 + t] + (even ? 1ul : 0ul)) & ~(even ? 1ul : 0ul) : 0ul;
        unsigned long all;
        const unsigned long at = carry + block_exclusive_scan<4>(v, wave_sums, all);
        if (c0 + t < n) {
            offsets[c0 + t] = at;
            if (table) {
                table[2 * (c0 + t)] = (long)at;
                table[2 * (c0 + t) + 1] = (long)sizes[c0 + t];
            }
        }
        carry += all;
        __syncthreads();                      // (the next step overwrites wave_sums)
    }
    if (t == 0) {
        *total = carry;
        if (table) table[2 * n] = (long)carry;
    }
}

// slot_words: the words between two slots.  even: a stream of odd size is followed by one zero byte.
__global__ __launch_bounds__(256) void k_deflate_compact(const uint32_t *__restrict__ slots, int slot_words, const uint32_t *__restrict__ sizes,
                                                         const unsigned long *__restrict__ offsets, int even, uint8_t *__restrict__ dst)
{
    const uint8_t *slot = (const uint8_t *)(slots + (size_t)blockIdx.x * slot_words);
    uint8_t *to = dst + offsets[blockIdx.x];
    const uint32_t size = sizes[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < size; i += 256) to[i] = slot[i];
    if (even && (size & 1u) && threadIdx.x == 0) to[size] = 0;
}

// rows: the candidate distances of the rows rule, or null for the run-only rule; dynamic: the dynamic coding
template <int E>
static int launch_encode(const void *src, long nbytes, long chunks, const RowDists *rows, bool dynamic, uint32_t *slots, uint32_t *sizes,
                         uint32_t *crc)
{
    constexpr size_t lds = (size_t)DF_LDS_WORDS * 4;
    const int aligned = (int)(((uintptr_t)src & 3u) == 0);
    if (dynamic) {
        constexpr size_t dlds = lds + (size_t)DY_WORDS * 4;
        if (rows) {
            TIP_HIP(hipFuncSetAttribute((const void *)k_deflate_dynamic<E, RowsRule<E>>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dlds));
            TIP_LAUNCH("deflate_dynamic_rows", (k_deflate_dynamic<E, RowsRule<E>>), dim3((unsigned)chunks), dim3(DF_THREADS), dlds,
                       (const uint8_t *)src, nbytes, aligned, *rows, slots, sizes, crc);
            return TIP_OK;
        }
        TIP_HIP(hipFuncSetAttribute((const void *)k_deflate_dynamic<E, RunsRule<E>>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dlds));
        TIP_LAUNCH("deflate_dynamic_runs", (k_deflate_dynamic<E, RunsRule<E>>), dim3((unsigned)chunks), dim3(DF_THREADS), dlds,
                   (const uint8_t *)src, nbytes, aligned, RowDists{}, slots, sizes, crc);
        return TIP_OK;
    }
    if (rows) {
        TIP_HIP(hipFuncSetAttribute((const void *)k_deflate_rows<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        TIP_LAUNCH("deflate_rows", k_deflate_rows<E>, dim3((unsigned)chunks), dim3(DF_THREADS), lds, (const uint8_t *)src, nbytes, aligned,
                   *rows, slots, sizes, crc);
        return TIP_OK;
    }
    TIP_HIP(hipFuncSetAttribute((const void *)k_deflate_runs<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TIP_LAUNCH("deflate_runs", k_deflate_runs<E>, dim3((unsigned)chunks), dim3(DF_THREADS), lds, (const uint8_t *)src, nbytes, aligned,
               slots, sizes, crc);
    return TIP_OK;
}

// The rows rule's candidates P, P + e, P - e, each kept when e < d <= 32768, with their distance codes (RFC 1951 3.2.5): codes
// 0 .. 3 are the distances 1 .. 4; from 5 on, with h the highest bit of d - 1, the code is 2 h + the bit below h, and the
// h - 1 bits below that are the extra bits.
static RowDists row_dists(int e, long row_bytes)
{
    RowDists r{};
    if (row_bytes > 32768 + e) return r;      // none is kept: the run-only rule
    const long cand[3] = {row_bytes, row_bytes + e, row_bytes - e};
    for (int k = 0; k < 3; ++k) {
        if (cand[k] <= e || cand[k] > 32768) continue;
        const uint32_t t = (uint32_t)cand[k] - 1u;
        int h = 31;
        while (!(t >> h)) --h;
        const int eb = t < 4u ? 0 : h - 1;
        const uint32_t code = t < 4u ? t : 2u * h + ((t >> eb) & 1u);
        uint32_t rev = 0;
        for (int b = 0; b < 5; ++b) rev |= ((code >> b) & 1u) << (4 - b);
        r.c[k] = {(int)cand[k], rev | ((t & ((1u << eb) - 1u)) << 5), 5 + eb, (int)code};
        r.row_bytes = row_bytes;
    }
    return r;
}

// row_bytes: the rows entries' row length (positive there), 0 from the runs entries
static int check_args(const char *who, const void *src, long nbytes, int elem_bytes, long row_bytes, const void *dst, long cap,
                      const void *out_bytes, const void *crc)
{
    if (!src || !dst || !out_bytes || !crc) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return fail(TIP_ERR_ARG, "%s: elem_bytes %d (1, 2 or 4)", who, elem_bytes);
    if (nbytes < 0 || nbytes % elem_bytes) return fail(TIP_ERR_ARG, "%s: nbytes %ld is not a multiple of elem_bytes %d", who, nbytes, elem_bytes);
    if (row_bytes % elem_bytes) return fail(TIP_ERR_ARG, "%s: row_bytes %ld is not a multiple of elem_bytes %d", who, row_bytes, elem_bytes);
    if (nbytes / DF_CHUNK >= (1L << 31)) return fail(TIP_ERR_ARG, "%s: nbytes %ld (at most 2^47)", who, nbytes);
    if (cap < stream_bound(nbytes)) return fail(TIP_ERR_ARG, "%s: cap %ld is below tip_deflate_runs_bound(%ld) = %ld", who, cap, nbytes, stream_bound(nbytes));
    return TIP_OK;
}

// row_bytes 0: the run-only rule -- which the rows rule also is when its row is too long for any candidate distance
static int deflate_dev(const void *src, long nbytes, int elem_bytes, long row_bytes, bool dynamic, void *dst, int64_t *out_bytes,
                       uint32_t *crc32)
{
    *out_bytes = 0;
    *crc32 = 0;
    if (nbytes == 0) return TIP_OK;           // no chunk: the empty stream, whose CRC is 0
    Ctx &c = ctx();
    const long chunks = (nbytes + DF_CHUNK - 1) / DF_CHUNK;
    WsGuard ws;
    uint32_t *slots = ws.get<uint32_t>((size_t)chunks * DF_OUT_WORDS), *sizes = ws.get<uint32_t>(chunks);
    unsigned long *offsets = ws.get<unsigned long>(chunks), *result = ws.get<unsigned long>(2);      // {total, crc}
    unsigned long *pin = (unsigned long *)pinned_scratch(16);
    if (!slots || !sizes || !offsets || !result || !pin) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemsetAsync(result, 0, 16, c.stream));
    const RowDists dists = row_dists(elem_bytes, row_bytes), *rows = dists.row_bytes ? &dists : nullptr;
    int rc = elem_bytes == 1 ? launch_encode<1>(src, nbytes, chunks, rows, dynamic, slots, sizes, (uint32_t *)(result + 1))
           : elem_bytes == 2 ? launch_encode<2>(src, nbytes, chunks, rows, dynamic, slots, sizes, (uint32_t *)(result + 1))
                             : launch_encode<4>(src, nbytes, chunks, rows, dynamic, slots, sizes, (uint32_t *)(result + 1));
    if (rc) return rc;
    TIP_LAUNCH("deflate_offsets", k_deflate_offsets, dim3(1), dim3(256), 0, sizes, chunks, offsets, result, 0, (long *)nullptr);
    TIP_LAUNCH("deflate_compact", k_deflate_compact, dim3((unsigned)chunks), dim3(256), 0, slots, DF_OUT_WORDS, sizes, offsets, 0, (uint8_t *)dst);
    TIP_HIP(hipMemcpyAsync(pin, result, 16, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    *out_bytes = (int64_t)pin[0];
    *crc32 = (uint32_t)pin[1];
    return TIP_OK;
}

// the two entry forms of both rules (row_bytes 0: run-only) and both codings
static int entry_dev(const char *who, const void *src, long nbytes, int elem_bytes, long row_bytes, bool dynamic, void *dst, long cap,
                     int64_t *out_bytes, uint32_t *crc32)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_args(who, src, nbytes, elem_bytes, row_bytes, dst, cap, out_bytes, crc32)) return rc;
    return deflate_dev(src, nbytes, elem_bytes, row_bytes, dynamic, dst, out_bytes, crc32);
}

static int entry_host(const char *who, const void *src, long nbytes, int elem_bytes, long row_bytes, bool dynamic, void *dst, long cap,
                      int64_t *out_bytes, uint32_t *crc32)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_args(who, src, nbytes, elem_bytes, row_bytes, dst, cap, out_bytes, crc32)) return rc;
    Staging st;
    const uint8_t *ds = st.in((const uint8_t *)src, (size_t)nbytes);
    uint8_t *dd = st.out((uint8_t *)dst, (size_t)stream_bound(nbytes));
    if (st.rc) return st.rc;
    if (int rc = deflate_dev(ds, nbytes, elem_bytes, row_bytes, dynamic, dd, out_bytes, crc32)) return rc;
    st.set_count(dd, (size_t)*out_bytes);
    return st.finish();
}

// ---- the strips entries ------------------------------------------------------------------------------------------------------
static StripPlan strip_plan(long n_pages, long rows, long row_bytes, long rps)
{
    StripPlan p{};
    p.rows = rows;
    p.row_bytes = row_bytes;
    p.rows_per_strip = rps;
    p.strips_per_page = (rows + rps - 1) / rps;
    p.n_strips = n_pages * p.strips_per_page;
    p.slot_words = (int)((strip_bound((rows < rps ? rows : rps) * row_bytes) + 3) / 4);
    return p;
}

static long strips_bound(long n_pages, long rows, long row_bytes, long rps)
{
    const long full = rows / rps, rest = rows % rps;
    return n_pages * (full * strip_bound(rps * row_bytes) + (rest ? strip_bound(rest * row_bytes) : 0));
}

static int check_strip_shape(const char *who, long n_pages, long rows, long row_bytes, long rps)
{
    if (n_pages < 0 || rows < 0) return fail(TIP_ERR_ARG, "%s: %ld pages of %ld rows", who, n_pages, rows);
    if (row_bytes < 1) return fail(TIP_ERR_ARG, "%s: row_bytes %ld is not positive", who, row_bytes);
    if (rps < 1) return fail(TIP_ERR_ARG, "%s: rows_per_strip %ld is not positive", who, rps);
    return TIP_OK;
}

static int check_strip_args(const char *who, const void *src, long n_pages, long rows, long row_bytes, int elem_bytes, long rps, int codes,
                            const void *dst, long cap, const void *table, const void *out_bytes)
{
    if (!src || !dst || !table || !out_bytes) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (elem_bytes != 1 && elem_bytes != 2) return fail(TIP_ERR_ARG, "%s: elem_bytes %d (1 or 2)", who, elem_bytes);
    if (codes != 0 && codes != 1) return fail(TIP_ERR_ARG, "%s: codes %d (0 fixed, 1 dynamic)", who, codes);
    if (int rc = check_strip_shape(who, n_pages, rows, row_bytes, rps)) return rc;
    if (row_bytes % elem_bytes) return fail(TIP_ERR_ARG, "%s: row_bytes %ld is not a multiple of elem_bytes %d", who, row_bytes, elem_bytes);
    if (rps > DF_CHUNK || rps * row_bytes > DF_CHUNK)
        return fail(TIP_ERR_UNSUPPORTED, "%s: a strip of %ld rows of %ld bytes is more than %d bytes", who, rps, row_bytes, DF_CHUNK);
    if (n_pages && (rows + rps - 1) / rps > 0x7FFFFFFFL / n_pages) return fail(TIP_ERR_ARG, "%s: more than 2^31 - 1 strips", who);
    if (cap < strips_bound(n_pages, rows, row_bytes, rps))
        return fail(TIP_ERR_ARG, "%s: cap %ld is below tip_deflate_strips_bound = %ld", who, cap, strips_bound(n_pages, rows, row_bytes, rps));
    return TIP_OK;
}

template <int E>
static int launch_strips(const uint8_t *src, const StripPlan &plan, const RowDists *rows, bool dynamic, unsigned groups, uint32_t *slots,
                         uint32_t *sizes)
{
    constexpr size_t lds = (size_t)DF_LDS_WORDS * 4, dlds = lds + (size_t)DY_WORDS * 4;
    if (dynamic && rows) {
        TIP_HIP(hipFuncSetAttribute((const void *)k_deflate_strips<E, true, RowsRule<E>>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dlds));
        TIP_LAUNCH("deflate_strips_dynamic_rows", (k_deflate_strips<E, true, RowsRule<E>>), dim3(groups), dim3(DF_THREADS), dlds, src, plan, *rows,
                   slots, sizes);
    } else if (dynamic) {
        TIP_HIP(hipFuncSetAttribute((const void *)k_deflate_strips<E, true, RunsRule<E>>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dlds));
        TIP_LAUNCH("deflate_strips_dynamic_runs", (k_deflate_strips<E, true, RunsRule<E>>), dim3(groups), dim3(DF_THREADS), dlds, src, plan,
                   RowDists{}, slots, sizes);
    } else if (rows) {
        TIP_HIP(hipFuncSetAttribute((const void *)k_deflate_strips<E, false, RowsRule<E>>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        TIP_LAUNCH("deflate_strips_rows", (k_deflate_strips<E, false, RowsRule<E>>), dim3(groups), dim3(DF_THREADS), lds, src, plan, *rows, slots,
                   sizes);
    } else {
        TIP_HIP(hipFuncSetAttribute((const void *)k_deflate_strips<E, false, RunsRule<E>>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        TIP_LAUNCH("deflate_strips_runs", (k_deflate_strips<E, false, RunsRule<E>>), dim3(groups), dim3(DF_THREADS), lds, src, plan, RowDists{},
                   slots, sizes);
    }
    return TIP_OK;
}

// all device addresses but table_host and out_bytes; the arguments are checked
static int deflate_strips_dev(const void *src, long n_pages, long rows, long row_bytes, int elem_bytes, long rps, bool dynamic, void *dst,
                              int64_t *table_host, int64_t *out_bytes)
{
    *out_bytes = 0;
    if (n_pages == 0 || rows == 0) return TIP_OK;
    Ctx &c = ctx();
    const StripPlan plan = strip_plan(n_pages, rows, row_bytes, rps);
    const long n = plan.n_strips;
    WsGuard ws;
    uint32_t *slots = ws.get<uint32_t>((size_t)n * plan.slot_words), *sizes = ws.get<uint32_t>(n);
    unsigned long *offsets = ws.get<unsigned long>(n), *total = ws.get<unsigned long>(1);
    long *table = ws.get<long>(2 * n + 1);
    long *pin = (long *)pinned_scratch((size_t)(2 * n + 1) * 8);
    if (!slots || !sizes || !offsets || !total || !table || !pin) return TIP_ERR_NOMEM;
    static int cus = 0;          // (same device model on every GPU of a node; a benign race writes the same value)
    if (!cus) {
        hipDeviceProp_t prop;
        cus = hipGetDeviceProperties(&prop, c.device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    const unsigned groups = (unsigned)(n < cus ? n : cus);      // one workgroup's LDS fills a CU
    const RowDists dists = row_dists(elem_bytes, row_bytes), *rd = dists.row_bytes ? &dists : nullptr;
    if (int rc = elem_bytes == 1 ? launch_strips<1>((const uint8_t *)src, plan, rd, dynamic, groups, slots, sizes)
                                 : launch_strips<2>((const uint8_t *)src, plan, rd, dynamic, groups, slots, sizes))
        return rc;
    TIP_LAUNCH("deflate_offsets", k_deflate_offsets, dim3(1), dim3(256), 0, sizes, n, offsets, total, 1, table);
    TIP_LAUNCH("deflate_compact", k_deflate_compact, dim3((unsigned)n), dim3(256), 0, slots, plan.slot_words, sizes, offsets, 1, (uint8_t *)dst);
    TIP_HIP(hipMemcpyAsync(pin, table, (size_t)(2 * n + 1) * 8, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    memcpy(table_host, pin, (size_t)n * 16);
    *out_bytes = pin[2 * n];
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_deflate_strips_bound(int64_t n_pages, int64_t rows, int64_t row_bytes, int64_t rows_per_strip, int64_t *bound_out)
{
    if (!bound_out) return fail(TIP_ERR_ARG, "tip_deflate_strips_bound: null pointer");
    if (int rc = check_strip_shape("tip_deflate_strips_bound", n_pages, rows, row_bytes, rows_per_strip)) return rc;
    *bound_out = strips_bound(n_pages, rows, row_bytes, rows_per_strip);
    return TIP_OK;
}

int tip_deflate_strips_dev(const void *src_dev, int64_t n_pages, int64_t rows, int64_t row_bytes, int elem_bytes, int64_t rows_per_strip,
                           int codes, void *dst_dev, int64_t cap, int64_t *table_host, int64_t *out_bytes_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_strip_args("tip_deflate_strips_dev", src_dev, n_pages, rows, row_bytes, elem_bytes, rows_per_strip, codes, dst_dev, cap,
                                  table_host, out_bytes_host))
        return rc;
    return deflate_strips_dev(src_dev, n_pages, rows, row_bytes, elem_bytes, rows_per_strip, codes == 1, dst_dev, table_host, out_bytes_host);
}

int tip_deflate_strips(const void *src, int64_t n_pages, int64_t rows, int64_t row_bytes, int elem_bytes, int64_t rows_per_strip, int codes,
                       void *dst, int64_t cap, int64_t *table, int64_t *out_bytes)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_strip_args("tip_deflate_strips", src, n_pages, rows, row_bytes, elem_bytes, rows_per_strip, codes, dst, cap, table,
                                  out_bytes))
        return rc;
    Staging st;
    const uint8_t *ds = st.in((const uint8_t *)src, (size_t)(n_pages * rows * row_bytes));
    uint8_t *dd = st.out((uint8_t *)dst, (size_t)strips_bound(n_pages, rows, row_bytes, rows_per_strip));
    if (st.rc) return st.rc;
    if (int rc = deflate_strips_dev(ds, n_pages, rows, row_bytes, elem_bytes, rows_per_strip, codes == 1, dd, table, out_bytes)) return rc;
    st.set_count(dd, (size_t)*out_bytes);
    return st.finish();
}

int tip_deflate_runs_bound(int64_t nbytes, int64_t *bound_out)
{
    if (!bound_out || nbytes < 0) return fail(TIP_ERR_ARG, "tip_deflate_runs_bound: null pointer or negative size");
    *bound_out = stream_bound(nbytes);
    return TIP_OK;
}

int tip_deflate_runs_dev(const void *src_dev, int64_t nbytes, int elem_bytes, void *dst_dev, int64_t cap, int64_t *out_bytes_host,
                         uint32_t *crc32_host)
{
    return entry_dev("tip_deflate_runs_dev", src_dev, nbytes, elem_bytes, 0, false, dst_dev, cap, out_bytes_host, crc32_host);
}

int tip_deflate_runs(const void *src, int64_t nbytes, int elem_bytes, void *dst, int64_t cap, int64_t *out_bytes, uint32_t *crc32)
{
    return entry_host("tip_deflate_runs", src, nbytes, elem_bytes, 0, false, dst, cap, out_bytes, crc32);
}

int tip_deflate_rows_dev(const void *src_dev, int64_t nbytes, int elem_bytes, int64_t row_bytes, void *dst_dev, int64_t cap,
                         int64_t *out_bytes_host, uint32_t *crc32_host)
{
    if (row_bytes <= 0) return fail(TIP_ERR_ARG, "tip_deflate_rows_dev: row_bytes %ld is not positive", (long)row_bytes);
    return entry_dev("tip_deflate_rows_dev", src_dev, nbytes, elem_bytes, row_bytes, false, dst_dev, cap, out_bytes_host, crc32_host);
}

int tip_deflate_rows(const void *src, int64_t nbytes, int elem_bytes, int64_t row_bytes, void *dst, int64_t cap, int64_t *out_bytes,
                     uint32_t *crc32)
{
    if (row_bytes <= 0) return fail(TIP_ERR_ARG, "tip_deflate_rows: row_bytes %ld is not positive", (long)row_bytes);
    return entry_host("tip_deflate_rows", src, nbytes, elem_bytes, row_bytes, false, dst, cap, out_bytes, crc32);
}

int tip_deflate_dynamic_dev(const void *src_dev, int64_t nbytes, int elem_bytes, int64_t row_bytes, void *dst_dev, int64_t cap,
                            int64_t *out_bytes_host, uint32_t *crc32_host)
{
    if (row_bytes < 0) return fail(TIP_ERR_ARG, "tip_deflate_dynamic_dev: row_bytes %ld is negative", (long)row_bytes);
    return entry_dev("tip_deflate_dynamic_dev", src_dev, nbytes, elem_bytes, row_bytes, true, dst_dev, cap, out_bytes_host, crc32_host);
}

int tip_deflate_dynamic(const void *src, int64_t nbytes, int elem_bytes, int64_t row_bytes, void *dst, int64_t cap, int64_t *out_bytes,
                        uint32_t *crc32)
{
    if (row_bytes < 0) return fail(TIP_ERR_ARG, "tip_deflate_dynamic: row_bytes %ld is negative", (long)row_bytes);
    return entry_host("tip_deflate_dynamic", src, nbytes, elem_bytes, row_bytes, true, dst, cap, out_bytes, crc32);
}

}  // extern "C"
