// tip_inflate.hip -- inflate of many independent deflate streams (the strips of a compressed TIFF) on the device, and the
// row pass that finishes 16-bit TIFF samples (byte order, horizontal predictor).  The decoder itself is tip_inflate_core.h,
// the same text for the device, for tip_inflate_strips_host and for the host sanitizer program.
//
// Kernel shape (k_inflate_strips): one wave per strip, four waves per 256-thread workgroup, the current block's decode
// tables in that wave's own 4 KB of LDS.  The wave walks the bit stream as ONE thread of control: every lane runs the
// decoder on the same bits (a uniform load is one broadcast, a uniform branch costs nothing), so no lane ever waits for a
// "decoding lane" and no token has to be handed over.  What the lanes share out is the output:
//   * literals collect in a 64-entry queue, one per lane's register, and leave as one 64-byte store;
//   * a match is copied by all lanes, byte k of it from window byte (k mod distance): a match that overlaps its own output
//     (distance < length) repeats its first `distance` bytes, which are complete before the match starts, so no lane reads a
//     byte another lane of the same copy writes;
//   * a match's source must be visible to every lane: the queue is flushed and, when the source reaches into bytes written
//     since the wave last waited, the wave waits for its stores (a workgroup-scope fence; L1 is per CU) before it reads;
//   * the Adler-32 is the wave's sum over the finished strip (position-weighted partial sums, one reduction).
// Strips differ in length, so they are handed out from a list sorted by compressed size, longest first, wave w of W taking
// entries w, w + W, ...: the long strips start first and on different workgroups, every wave's share is one of each size
// class, and a wave that is done leaves its SIMD to another workgroup -- no wave waits on a workgroup's other three.  (A frame
// of 64 KB strips has about as many strips as the grid has waves: one each.)
#include <algorithm>
#include <numeric>
#include "tip_internal.h"
#include "tip_inflate_core.h"

namespace tip {

using tip_inflate::Tables;

// the wave's number, said to the compiler to be the same in every lane
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the wave's Out (tip_inflate_core.h): positions are checked by the core before they arrive here
struct WaveOut {
    uint8_t *dst;
    int lane;
    int nlit = 0;            // literals queued: lane k holds the k-th
    int64_t lit_pos = 0;     // the first queued literal's position
    uint32_t held = 0;
    int64_t seen = 0;        // output below this position is visible to every lane (the wave has waited for those stores)

    __device__ __forceinline__ void flush()
    {
        if (lane < nlit) dst[lit_pos + lane] = (uint8_t)held;
        nlit = 0;
    }
    __device__ __forceinline__ void lit(int64_t pos, uint32_t byte)
    {
        if (nlit == 0) lit_pos = pos;
        if (lane == nlit) held = byte;
        if (++nlit == 64) flush();
    }
    __device__ __forceinline__ void wait_stores(int64_t pos)
    {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        seen = pos;
    }
    __device__ __forceinline__ void match(int64_t pos, int length, int distance)
    {
        flush();
        const int period = distance < length ? distance : length;      // the source bytes really read: [pos - distance, + period)
        if (pos - distance + period > seen) wait_stores(pos);
        const uint8_t *from = dst + (pos - distance);
        if (distance >= length) {
            for (int k = lane; k < length; k += 64) dst[pos + k] = from[k];
        } else {
            for (int k = lane; k < length; k += 64) dst[pos + k] = from[k % distance];
        }
    }
    __device__ __forceinline__ uint32_t adler(int64_t n)
    {
        flush();
        wait_stores(n);
        uint64_t s1 = 0, s2 = 0;
        int64_t w = (n - lane) % 65521;          // (n - i) mod 65521 at i = lane; n - lane may be negative on a short strip
        if (w < 0) w += 65521;
        for (int64_t i = lane; i < n; i += 64) {
            const uint32_t d = dst[i];
            s1 += d;
            s2 += (uint64_t)w * d;
            w -= 64;
            if (w < 0) w += 65521;
        }
        const uint32_t a = wave_sum((uint32_t)(s1 % 65521u)), b = wave_sum((uint32_t)(s2 % 65521u));
        return tip_inflate::adler_from_sums(a % 65521u, b % 65521u, n);
    }
};

constexpr int INF_WAVES = 4;

// The wave's strips are order[w], order[w + W], order[w + 2 W], ... with w its number in the grid and W the grid's waves: the
// loop's trip count and every address in it come from the wave's number alone, so the loop is uniform by construction.  (A
// work counter taken by `if (lane == 0) atomicAdd` and broadcast with readfirstlane is NOT: the compiler may thread the
// lane-0 branch through the loop's back edge and run the body once more for the other 63 lanes alone, where readfirstlane
// reads a lane that never took a number -- an endless loop.  No branch on the lane number stands between two iterations here.)
__global__ __launch_bounds__(64 * INF_WAVES) void k_inflate_strips(const uint8_t *__restrict__ src, const int64_t *__restrict__ strips,
                                                                    const int32_t *__restrict__ order, int n_strips, int wrapper,
                                                                    uint8_t *dst, int32_t *status)
{
    __shared__ Tables tables[INF_WAVES];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = uniform((int)(threadIdx.x >> 6));
    Tables &T = tables[wave];
    T.fixed_ready = 0;
    const long stride = (long)gridDim.x * INF_WAVES;
    for (long i = (long)blockIdx.x * INF_WAVES + wave; i < n_strips; i += stride) {
        const long s = order[i];
        const int64_t src_off = strips[4 * s], src_len = strips[4 * s + 1], dst_off = strips[4 * s + 2], dst_len = strips[4 * s + 3];
        WaveOut out{dst + dst_off, lane};
        const int st = tip_inflate::inflate_stream(src + src_off, src_len, dst_len, wrapper, T, out);
        out.flush();
        status[s] = st;               // (every lane stores the same word)
    }
}

// the number of non-zero status words, by one workgroup
__global__ __launch_bounds__(256) void k_inflate_count_bad(const int32_t *__restrict__ status, int n_strips, unsigned *n_bad)
{
    __shared__ unsigned part[4];
    unsigned mine = 0;
    for (int i = (int)threadIdx.x; i < n_strips; i += 256) mine += status[i] != 0;
    mine = block_sum<4>(mine, part);
    if (threadIdx.x == 0) *n_bad = mine;
}

// One wave per row, in place: each 16-bit sample's bytes swapped when the file's order is not the host's, then (predictor 2)
// the running sum along the row modulo 2^16 -- libtiff's order.  64 samples a step: a shuffle scan, the carry from lane 63.
__global__ __launch_bounds__(256) void k_tiff_finish_u16(uint16_t *stack, long n_rows, long row_elems, int predictor, int swap)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int lane = (int)(threadIdx.x & 63u);
    uint16_t *p = stack + row * row_elems;
    uint32_t carry = 0;
    for (long base = 0; base < row_elems; base += 64) {
        const long i = base + lane;
        uint32_t v = i < row_elems ? p[i] : 0u;
        if (swap) v = ((v & 0xFFu) << 8) | (v >> 8);
        if (predictor == 2) {
            v = wave_inclusive_scan(v) + carry;
            carry = (uint32_t)__shfl((int)v, 63, 64);
        }
        if (i < row_elems) p[i] = (uint16_t)v;
    }
}

// The table's checks, on a host copy: every strip inside both buffers, the non-empty destinations disjoint.  order: the
// strips by compressed size, longest first.
static int check_strips(const char *who, const int64_t *strips, long n, long src_bytes, long dst_bytes, std::vector<int32_t> &order)
{
    for (long i = 0; i < n; ++i) {
        const int64_t so = strips[4 * i], sl = strips[4 * i + 1], d0 = strips[4 * i + 2], dl = strips[4 * i + 3];
        if (so < 0 || sl < 0 || so > src_bytes || sl > src_bytes - so)
            return fail(TIP_ERR_ARG, "%s: strip %ld's source [%ld, +%ld) leaves the %ld source bytes", who, i, (long)so, (long)sl, src_bytes);
        if (d0 < 0 || dl < 0 || d0 > dst_bytes || dl > dst_bytes - d0)
            return fail(TIP_ERR_ARG, "%s: strip %ld's destination [%ld, +%ld) leaves the %ld destination bytes", who, i, (long)d0, (long)dl, dst_bytes);
    }
    order.resize((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return strips[4 * (long)a + 2] != strips[4 * (long)b + 2] ? strips[4 * (long)a + 2] < strips[4 * (long)b + 2] : a < b;
    });
    int64_t end = 0;
    long owner = -1;
    for (int32_t s : order) {
        if (strips[4 * (long)s + 3] == 0) continue;
        if (strips[4 * (long)s + 2] < end)
            return fail(TIP_ERR_ARG, "%s: the destinations of strips %ld and %ld overlap", who, owner, (long)s);
        end = strips[4 * (long)s + 2] + strips[4 * (long)s + 3];
        owner = s;
    }
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return strips[4 * (long)a + 1] != strips[4 * (long)b + 1] ? strips[4 * (long)a + 1] > strips[4 * (long)b + 1] : a < b;
    });
    return TIP_OK;
}

static int check_call(const char *who, const void *src, long src_bytes, const void *strips, long n, int wrapper, const void *dst,
                      long dst_bytes, const void *status, const void *n_bad)
{
    if (!src || !strips || !dst || !status || !n_bad) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (src_bytes < 0 || dst_bytes < 0 || n < 0 || n > 0x7FFFFFFFL) return fail(TIP_ERR_ARG, "%s: a negative size, or more than 2^31 - 1 strips", who);
    if (wrapper != 0 && wrapper != 1) return fail(TIP_ERR_ARG, "%s: wrapper %d (0 raw, 1 zlib)", who, wrapper);
    return TIP_OK;
}

// all device addresses; `order` the host's list.  Leaves the count of failed strips in *n_bad after one wait.
static int inflate_dev(const uint8_t *src, const int64_t *strips, const std::vector<int32_t> &order, int wrapper, uint8_t *dst,
                       int32_t *status, int32_t *n_bad)
{
    Ctx &c = ctx();
    const long n = (long)order.size();
    WsGuard ws;
    int32_t *d_order = ws.get<int32_t>((size_t)n);
    unsigned *bad = ws.get<unsigned>(1);              // failed strips
    unsigned *pin = (unsigned *)pinned_scratch(4);
    if (!d_order || !bad || !pin) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(d_order, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, c.stream));
    static int cus = 0;          // (same device model on every GPU of a node; a benign race writes the same value)
    if (!cus) {
        hipDeviceProp_t prop;
        cus = hipGetDeviceProperties(&prop, c.device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    const long groups = std::min<long>((n + INF_WAVES - 1) / INF_WAVES, (long)cus * 8);      // 8: the 256-thread workgroups a CU holds
    TIP_LAUNCH("inflate_strips", k_inflate_strips, dim3((unsigned)groups), dim3(64 * INF_WAVES), 0, src, strips, d_order, (int)n, wrapper, dst,
               status);
    TIP_LAUNCH("inflate_count_bad", k_inflate_count_bad, dim3(1), dim3(256), 0, status, (int)n, bad);
    TIP_HIP(hipMemcpyAsync(pin, bad, 4, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    *n_bad = (int32_t)pin[0];
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_inflate_strips_host(const void *src, int64_t src_bytes, const int64_t *strips, int64_t n_strips, int wrapper, void *dst,
                            int64_t dst_bytes, int32_t *status, int32_t *n_bad)
{
    const char *who = "tip_inflate_strips_host";
    if (int rc = check_call(who, src, src_bytes, strips, n_strips, wrapper, dst, dst_bytes, status, n_bad)) return rc;
    std::vector<int32_t> order;
    if (int rc = check_strips(who, strips, n_strips, src_bytes, dst_bytes, order)) return rc;
    std::vector<Tables> tables(1);
    tables[0].fixed_ready = 0;
    int32_t bad = 0;
    for (long i = 0; i < n_strips; ++i) {
        status[i] = tip_inflate::inflate_strip_serial((const uint8_t *)src, strips + 4 * i, wrapper, (uint8_t *)dst, tables[0]);
        bad += status[i] != 0;
    }
    *n_bad = bad;
    return TIP_OK;
}

int tip_inflate_strips_dev(const void *src_dev, int64_t src_bytes, const int64_t *strips_dev, int64_t n_strips, int wrapper, void *dst_dev,
                           int64_t dst_bytes, int32_t *status_dev, int32_t *n_bad_host)
{
    const char *who = "tip_inflate_strips_dev";
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_call(who, src_dev, src_bytes, strips_dev, n_strips, wrapper, dst_dev, dst_bytes, status_dev, n_bad_host)) return rc;
    *n_bad_host = 0;
    if (n_strips == 0) return TIP_OK;
    // the checks need the table on the host: one small download (32 bytes a strip) before anything is launched
    std::vector<int64_t> table((size_t)n_strips * 4);
    TIP_HIP(hipMemcpyAsync(table.data(), strips_dev, table.size() * 8, hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    std::vector<int32_t> order;
    if (int rc = check_strips(who, table.data(), n_strips, src_bytes, dst_bytes, order)) return rc;
    return inflate_dev((const uint8_t *)src_dev, strips_dev, order, wrapper, (uint8_t *)dst_dev, status_dev, n_bad_host);
}

int tip_inflate_strips(const void *src, int64_t src_bytes, const int64_t *strips, int64_t n_strips, int wrapper, void *dst, int64_t dst_bytes,
                       int32_t *status, int32_t *n_bad)
{
    const char *who = "tip_inflate_strips";
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (int rc = check_call(who, src, src_bytes, strips, n_strips, wrapper, dst, dst_bytes, status, n_bad)) return rc;
    *n_bad = 0;
    if (n_strips == 0) return TIP_OK;
    std::vector<int32_t> order;
    if (int rc = check_strips(who, strips, n_strips, src_bytes, dst_bytes, order)) return rc;
    Staging st;
    const uint8_t *d_src = st.in((const uint8_t *)src, (size_t)src_bytes);
    const int64_t *d_strips = st.in(strips, (size_t)n_strips * 4);
    uint8_t *d_dst = st.in((const uint8_t *)dst, (size_t)dst_bytes);      // the bytes between the strips come back as they went
    int32_t *d_status = st.out(status, (size_t)n_strips);
    if (st.rc) return st.rc;
    if (d_dst) st.outs.push_back({dst, d_dst, (size_t)dst_bytes});
    if (int rc = inflate_dev(d_src, d_strips, order, wrapper, d_dst, d_status, n_bad)) return rc;
    return st.finish();
}

int tip_tiff_finish_u16_dev(void *stack_dev, int64_t n_rows, int64_t row_elems, int predictor, int swap_bytes)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!stack_dev || n_rows < 0 || row_elems < 0) return fail(TIP_ERR_ARG, "tip_tiff_finish_u16_dev: null pointer or a negative extent");
    if (predictor != 1 && predictor != 2) return fail(TIP_ERR_UNSUPPORTED, "tip_tiff_finish_u16_dev: predictor %d (1: none, 2: horizontal differencing)", predictor);
    if ((n_rows + 3) / 4 > 0x7FFFFFFFL) return fail(TIP_ERR_ARG, "tip_tiff_finish_u16_dev: %ld rows (at most 2^33 - 4)", (long)n_rows);
    if (n_rows == 0 || row_elems == 0 || (predictor == 1 && !swap_bytes)) return TIP_OK;
    TIP_LAUNCH("tiff_finish_u16", k_tiff_finish_u16, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (uint16_t *)stack_dev, (long)n_rows,
               (long)row_elems, predictor, swap_bytes ? 1 : 0);
    return TIP_OK;
}

}  // extern "C"
