// tip_deflate.hip -- run-only deflate (RFC 1951) and CRC-32 of a device buffer, so that a label map or a type map leaves its
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
// k_deflate_runs: one workgroup (256 threads) per chunk, one thread per segment.
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
#include "tip_internal.h"

namespace tip {

constexpr int DF_CHUNK = 65536, DF_SEG = 256, DF_THREADS = DF_CHUNK / DF_SEG;
constexpr int DF_SEG_LD = DF_SEG / 4 + 1;                       // dwords between two segments in LDS
constexpr uint32_t DF_POLY = 0xEDB88320u;

// The most bytes a chunk of n input bytes takes: 3 header bits, at most 9 bits per byte (the longest literal; a match of
// R >= 3 bytes takes at most 8 + 5 + 5 bits, fewer than R literals), 7 bits of end-of-block, the 3 header bits of the
// stored block, the padding, LEN and NLEN.
__host__ __device__ constexpr long chunk_bound(long n) { return (3 + 9 * n + 7 + 3 + 7) / 8 + 4; }

constexpr int DF_OUT_WORDS = (int)((chunk_bound(DF_CHUNK) + 3) / 4) + 1;      // LDS output words (+1: the accumulator's last flush)
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
    __device__ void put(uint32_t v, int n)  // n <= 18 and nacc < 32: the accumulator never passes 50 bits
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

template <int E, class Sink> __device__ static inline void put_match(Sink &s, int len)      // 3 <= len <= 256, distance E
{
    const uint32_t n = (uint32_t)len - 3u;
    const int eb = n < 8u ? 0 : (31 - __clz((int)n)) - 2;          // extra bits of the length symbol
    const uint32_t sym = n < 8u ? 257u + n : 261u + 4u * eb + ((n >> eb) & 3u);
    uint32_t v;
    int nb;
    if (sym < 280u) { v = __brev(sym - 256u) >> 25; nb = 7; }
    else { v = __brev(0xC0u + (sym - 280u)) >> 24; nb = 8; }
    v |= (n & ((1u << eb) - 1u)) << nb;
    nb += eb;
    constexpr uint32_t dist_rev5 = E == 1 ? 0u : E == 2 ? 16u : 24u;   // distance codes 0, 1, 3 (distances 1, 2, 4), five bits reversed
    v |= dist_rev5 << nb;
    s.put(v, nb + 5);
}

template <int E, class Sink> __device__ static inline void put_run(Sink &s, int run, uint32_t elem)
{
    if (run == 0) return;
    if (run >= (E > 3 ? E : 3)) { put_match<E>(s, run); return; }
    for (int i = 0; i < run; ++i) put_literal(s, (elem >> (8 * (i % E))) & 255u);      // (E = 1: run 1, 2; E = 2: run 2)
}

// one thread's segment: nb valid bytes (a multiple of E) at seg[0 ..]; prev: the element before it, when has_prev
template <int E, class Sink> __device__ static inline void encode_segment(Sink &s, const uint32_t *seg, int nb, bool has_prev, uint32_t prev)
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
                    put_run<E>(s, run, prev);
                    run = 0;
#pragma unroll
                    for (int b = 0; b < E; ++b) put_literal(s, (x >> (8 * b)) & 255u);
                }
                prev = x;
                has_prev = true;
            }
        }
    }
    put_run<E>(s, run, prev);
}

template <int E>
__global__ __launch_bounds__(DF_THREADS) void k_deflate_runs(const uint8_t *__restrict__ src, long nbytes, int aligned,
                                                             uint32_t *__restrict__ slots, uint32_t *__restrict__ sizes,
                                                             uint32_t *__restrict__ crc_out)
{
    extern __shared__ uint32_t df_lds[];
    uint32_t *in = df_lds, *out = df_lds + DF_IN_WORDS, *crctab = out + DF_OUT_WORDS, *misc = crctab + 256;
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * DF_CHUNK;
    const int L = (int)(nbytes - base < DF_CHUNK ? nbytes - base : DF_CHUNK);      // 1 .. 65536, a multiple of E
    const uint8_t *chunk = src + base;

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
    const int out_words = (int)((chunk_bound(L) + 3) / 4) + 1;
    for (int i = t; i < out_words; i += DF_THREADS) out[i] = 0;
    {
        uint32_t c = (uint32_t)t;             // the CRC of the one byte t: eight steps of the bitwise definition
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? DF_POLY : 0u);
        crctab[t] = c;
    }
    if (t < 8) misc[t] = 0;                   // [0..3] the waves' bit totals, [4] the workgroup's CRC
    __syncthreads();

    const int first = t * DF_SEG;
    const int nb = L - first < 0 ? 0 : (L - first < DF_SEG ? L - first : DF_SEG);
    const uint32_t *seg = in + t * DF_SEG_LD;
    const bool has_prev = t > 0 && nb > 0;
    const uint32_t prev = has_prev ? in[(t - 1) * DF_SEG_LD + 63] >> (32 - 8 * E) : 0u;      // the segment before is full

    CountSink cs;
    encode_segment<E>(cs, seg, nb, has_prev, prev);
    // exclusive block scan of the bit counts: within the wave by shuffles, across the four waves through LDS
    const int lane = t & 63, wave = t >> 6;
    uint32_t incl = cs.bits;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) misc[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < DF_THREADS / 64; ++w) {
        if (w < wave) before += misc[w];
        total += misc[w];
    }
    const uint32_t bitpos = 3u + before + (incl - cs.bits);

    WordSink ws(out, t == 0 ? 0u : bitpos);
    if (t == 0) ws.put(2u, 3);                // BFINAL 0, then BTYPE 01 least significant bit first
    encode_segment<E>(ws, seg, nb, has_prev, prev);
    ws.flush();
    // end of block (seven zero bits) and the stored block's header (three) are zeros already; behind the padding LEN = 0, NLEN = FFFF
    const uint32_t body = (3u + total + 7u + 3u + 7u) / 8u, size = body + 4u;
    if (t == 0) {
        atomicOr(&out[(body + 2u) >> 2], 0xFFu << (8u * ((body + 2u) & 3u)));
        atomicOr(&out[(body + 3u) >> 2], 0xFFu << (8u * ((body + 3u) & 3u)));
    }

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
    __syncthreads();                          // the output words and the CRC are complete

    uint32_t *slot = slots + (size_t)blockIdx.x * DF_OUT_WORDS;
    for (uint32_t i = t; 4u * i < size; i += DF_THREADS) slot[i] = out[i];
    if (t == 0) {
        sizes[blockIdx.x] = size;
        atomicXor(crc_out, misc[4]);
    }
}

// offsets[c] = sizes[0] + ... + sizes[c - 1]; *total = the sum.  One workgroup, 256 chunks per step.
__global__ __launch_bounds__(256) void k_deflate_offsets(const uint32_t *__restrict__ sizes, long n, unsigned long *__restrict__ offsets,
                                                         unsigned long *__restrict__ total)
{
    __shared__ unsigned long wave_sum[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long carry = 0;
    for (long c0 = 0; c0 < n; c0 += 256) {
        const unsigned long v = c0 + t < n ? sizes[c0 + t] : 0ul;
        unsigned long incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned long before = 0, all = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wave_sum[w];
            all += wave_sum[w];
        }
        if (c0 + t < n) offsets[c0 + t] = carry + before + incl - v;
        carry += all;
        __syncthreads();                      // (the next step overwrites wave_sum)
    }
    if (t == 0) *total = carry;
}

__global__ __launch_bounds__(256) void k_deflate_compact(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ sizes,
                                                         const unsigned long *__restrict__ offsets, uint8_t *__restrict__ dst)
{
    const uint8_t *slot = (const uint8_t *)(slots + (size_t)blockIdx.x * DF_OUT_WORDS);
    uint8_t *to = dst + offsets[blockIdx.x];
    const uint32_t size = sizes[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < size; i += 256) to[i] = slot[i];
}

template <int E> static int launch_encode(const void *src, long nbytes, long chunks, uint32_t *slots, uint32_t *sizes, uint32_t *crc)
{
    constexpr size_t lds = (size_t)DF_LDS_WORDS * 4;
    TIP_HIP(hipFuncSetAttribute((const void *)k_deflate_runs<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TIP_LAUNCH("deflate_runs", k_deflate_runs<E>, dim3((unsigned)chunks), dim3(DF_THREADS), lds, (const uint8_t *)src, nbytes,
               (int)(((uintptr_t)src & 3u) == 0), slots, sizes, crc);
    return TIP_OK;
}

static int check_args(const char *who, const void *src, long nbytes, int elem_bytes, const void *dst, long cap, const void *out_bytes,
                      const void *crc)
{
    if (!src || !dst || !out_bytes || !crc) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return fail(TIP_ERR_ARG, "%s: elem_bytes %d (1, 2 or 4)", who, elem_bytes);
    if (nbytes < 0 || nbytes % elem_bytes) return fail(TIP_ERR_ARG, "%s: nbytes %ld is not a multiple of elem_bytes %d", who, nbytes, elem_bytes);
    if (nbytes / DF_CHUNK >= (1L << 31)) return fail(TIP_ERR_ARG, "%s: nbytes %ld (at most 2^47)", who, nbytes);
    if (cap < stream_bound(nbytes)) return fail(TIP_ERR_ARG, "%s: cap %ld is below tip_deflate_runs_bound(%ld) = %ld", who, cap, nbytes, stream_bound(nbytes));
    return TIP_OK;
}

static int deflate_runs_dev(const void *src, long nbytes, int elem_bytes, void *dst, int64_t *out_bytes, uint32_t *crc32)
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
    int rc = elem_bytes == 1 ? launch_encode<1>(src, nbytes, chunks, slots, sizes, (uint32_t *)(result + 1))
           : elem_bytes == 2 ? launch_encode<2>(src, nbytes, chunks, slots, sizes, (uint32_t *)(result + 1))
                             : launch_encode<4>(src, nbytes, chunks, slots, sizes, (uint32_t *)(result + 1));
    if (rc) return rc;
    TIP_LAUNCH("deflate_offsets", k_deflate_offsets, dim3(1), dim3(256), 0, sizes, chunks, offsets, result);
    TIP_LAUNCH("deflate_compact", k_deflate_compact, dim3((unsigned)chunks), dim3(256), 0, slots, sizes, offsets, (uint8_t *)dst);
    TIP_HIP(hipMemcpyAsync(pin, result, 16, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    *out_bytes = (int64_t)pin[0];
    *crc32 = (uint32_t)pin[1];
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_deflate_runs_bound(int64_t nbytes, int64_t *bound_out)
{
    if (!bound_out || nbytes < 0) return fail(TIP_ERR_ARG, "tip_deflate_runs_bound: null pointer or negative size");
    *bound_out = stream_bound(nbytes);
    return TIP_OK;
}

int tip_deflate_runs_dev(const void *src_dev, int64_t nbytes, int elem_bytes, void *dst_dev, int64_t cap, int64_t *out_bytes_host,
                         uint32_t *crc32_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_args("tip_deflate_runs_dev", src_dev, nbytes, elem_bytes, dst_dev, cap, out_bytes_host, crc32_host)) return rc;
    return deflate_runs_dev(src_dev, nbytes, elem_bytes, dst_dev, out_bytes_host, crc32_host);
}

int tip_deflate_runs(const void *src, int64_t nbytes, int elem_bytes, void *dst, int64_t cap, int64_t *out_bytes, uint32_t *crc32)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_args("tip_deflate_runs", src, nbytes, elem_bytes, dst, cap, out_bytes, crc32)) return rc;
    Staging st;
    const uint8_t *ds = st.in((const uint8_t *)src, (size_t)nbytes);
    uint8_t *dd = st.out((uint8_t *)dst, (size_t)stream_bound(nbytes));
    if (st.rc) return st.rc;
    if (int rc = deflate_runs_dev(ds, nbytes, elem_bytes, dd, out_bytes, crc32)) return rc;
    st.set_count(dd, (size_t)*out_bytes);
    return st.finish();
}

}  // extern "C"
