// mfma_f16_shape_lds.hip -- which fp16 MFMA shape is faster BY WALL at k_unet_conv's wave tile and LDS traffic?  The go / no-go
// measurement in front of a 16x16x32 version of the f16x3 convolution.  mfma_f16_rate.hip runs the two shapes from
// registers only and on eight accumulators; this one runs them the way the convolution's main loop would:
//   * a wave owns 64 pixels x 128 output channels = 128 accumulator registers (32x32x16: 2 x 4 tiles of 16; 16x16x32: 4 x 8 tiles
//     of 4), eight waves per workgroup, one workgroup per CU = two waves per SIMD, 152 KB of LDS like the 16-row kernel;
//   * three products per term (lo x hi, hi x lo, hi x hi of two-piece operands), weights as the A operand;
//   * every fragment is re-read from LDS by ds_read_b128 at the kernel's ratio: a K = 16 step is 12 reads for 24 32x32x16 MFMAs, a
//     K = 32 pair step -- lanes 0-31 on step 2j, lanes 32-63 on step 2j + 1 -- is 24 reads for 96 16x16x32 MFMAs; the addresses are
//     the kernel's (34-pixel halo rows, the tap's shifted window, 32-byte rows with the XOR swizzle, a ring of weight tiles), and the
//     16x16x32 reads use the row / pixel order 8-11 <-> 12-15 inside a 16-group, which keeps ds_read_b128's lane groups on 16 different
//     bank quads (checked below at compile time for every alignment);
//   * LDS holds random fp16 bits (finite, exponents near 1) or zeros.  No global -> LDS copies, no barriers, no epilogue: the
//     question is the matrix pipe's clock and issue under the main loop's operand traffic, nothing else.
// Wave 0 of block 0 reads s_memtime and s_memrealtime around its loop (mfma_f16_rate.hip): shader clock and clocks per MFMA.  The
// register-only rows (same tile, fragments read once) are there to show what the LDS reads cost, and whether 16x16x32 issues in
// 16 clocks: mfma_f16_rate.hip's 17.0 (26.8 with one wave per SIMD) is not the instruction -- the compiler shifts that loop's
// accumulator tuples by two registers in the third round and moves them back with 57 v_accvgpr_read / write / mov per 24 MFMAs.
//   hipcc -O3 --offload-arch=gfx950 tools/ubench/mfma_f16_shape_lds.hip -o /tmp/mfma_f16_shape_lds && /tmp/mfma_f16_shape_lds
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) unsigned char lds_byte;

constexpr int HW = 34;                                  // halo row (pixels) of the 16-row tile
constexpr int A_PLANE = 1280 * 16, A_BYTES = 2 * A_PLANE;   // one piece's halo tile padded to whole waves of slots; two pieces
constexpr int B_PLANE = 256 * 16, B_BYTES = 2 * B_PLANE;    // one (chunk, tap) step's weight tile: 128 rows of 32 bytes per piece
constexpr int NB = 6;                                   // weight ring: three pair steps
constexpr int LDS_BYTES = 2 * A_BYTES + 9 * B_BYTES;    // the 16-row kernel's 152 KB (one workgroup per CU)

// stored row (weights) / pixel (activations) of index i inside a 16-group
constexpr int map16(int i) { return i < 8 ? i : i ^ 4; }
constexpr int slot_of(int row, int half) { return row * 2 + (half ^ ((row >> 3) & 1)); }
// ds_read_b128 serves a wave in four groups of 16 lanes: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32
constexpr int group_lane(int g, int i) { return (g & 1 ? (i < 8 ? 4 + i : i < 12 ? 8 + i : 16 + i) : (i < 4 ? i : i < 8 ? 8 + i : 12 + i)) + 32 * (g >> 1); }
constexpr bool k32_conflict_free()
{
    for (int align = 0; align < 64; ++align)            // first row / pixel of the 16-group, any alignment
        for (int g = 0; g < 2; ++g) {                   // (lanes 32-63 repeat the pattern on another step's tile)
            unsigned seen = 0;
            for (int i = 0; i < 16; ++i) {
                const int lane = group_lane(g, i), quad = slot_of(align + map16(lane & 15), (lane >> 4) & 1) & 15;
                if (seen & (1u << quad)) return false;
                seen |= 1u << quad;
            }
        }
    return true;
}
constexpr bool map16_bijective()
{
    unsigned seen = 0;
    for (int i = 0; i < 16; ++i) seen |= 1u << map16(i);
    return seen == 0xffffu;
}
static_assert(map16_bijective(), "a permutation of the 16 rows / pixels");
static_assert(k32_conflict_free(), "16 different bank quads per lane group at every alignment");

template <int OFF>
__device__ __forceinline__ void lds_read(u32x4 &v, unsigned addr)
{
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
}
template <int N>
__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N)); }
__device__ __forceinline__ void tie(u32x4 &v) { asm volatile("" : "+v"(v)); }        // (behind a wait: no use of v is scheduled in front of it)
__device__ __forceinline__ f32x16 mfma32(const u32x4 &a, const u32x4 &b, const f32x16 &c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(const u32x4 &a, const u32x4 &b, const f32x4 &c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ int tap_dy(int t) { return ((t * 11) >> 5) - 1; }          // t / 3 - 1 for t < 9
__device__ __forceinline__ int tap_dx(int t) { return t - 3 * ((t * 11) >> 5) - 1; }

// SHAPE 0: 32x32x16, two K = 16 steps per iteration.  SHAPE 1: 16x16x32, one K = 32 pair step per iteration.  Both: 2 x 24 x 32768
// = 96 x 16384 FLOP per wave and iteration, 24 ds_read_b128.  LDS == 0: the fragments are read once, in front of the loop.
template <int SHAPE, int LDS>
__global__ void __launch_bounds__(512, 2) k_loop(float *out, unsigned long long *clk, int iters, const uint4 *fill)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int q = tid; q < LDS_BYTES / 16; q += 512) reinterpret_cast<uint4 *>(smem)[q] = fill[q];
    __syncthreads();
    const unsigned sA = (unsigned)(unsigned long long)(const lds_byte *)smem, sB = sA + 2 * A_BYTES;
    f32x16 acc[2][4];
    f32x4 acd[4][8];
    for (int m = 0; m < 2; ++m) for (int n = 0; n < 4; ++n) for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.f;
    for (int g = 0; g < 4; ++g) for (int n = 0; n < 8; ++n) for (int i = 0; i < 4; ++i) acd[g][n][i] = 0.f;
    int tap = 0, chunk = 0, wb = 0;                     // of the iteration's first step (scalar)
    auto next = [&]() { if (++tap == 9) { tap = 0; chunk ^= 1; } if (++wb == NB) wb = 0; };
    u32x4 fa[2][2], fb[4][2], ga[4][2], gb[8][2];
    auto read32 = [&]() {
        const int r = lane & 31, h = lane >> 5;
        const int px0 = (wave * 2 + 1 + tap_dy(tap)) * HW + r + 1 + tap_dx(tap), px1 = px0 + HW;
        const unsigned ra0 = sA + chunk * A_BYTES + slot_of(px0, h) * 16, ra1 = sA + chunk * A_BYTES + slot_of(px1, h) * 16;
        const unsigned rb = sB + wb * B_BYTES + slot_of(r, h) * 16;
        lds_read<A_PLANE>(fa[0][1], ra0); lds_read<A_PLANE>(fa[1][1], ra1);
        lds_read<0>(fb[0][0], rb); lds_read<1024>(fb[1][0], rb); lds_read<2048>(fb[2][0], rb); lds_read<3072>(fb[3][0], rb);
        lds_read<0>(fa[0][0], ra0); lds_read<0>(fa[1][0], ra1);
        lds_read<B_PLANE>(fb[0][1], rb); lds_read<B_PLANE + 1024>(fb[1][1], rb); lds_read<B_PLANE + 2048>(fb[2][1], rb); lds_read<B_PLANE + 3072>(fb[3][1], rb);
    };
    auto read16 = [&]() {
        // lanes 0-31: step 2j (tap, wb), lanes 32-63: step 2j + 1; K-group bit 0 = which 8-channel half of the 16-channel row
        const int c = map16(lane & 15), half = (lane >> 4) & 1, odd = lane >> 5;
        int tap1 = tap + 1, chunk1 = chunk;
        if (tap1 == 9) { tap1 = 0; chunk1 ^= 1; }       // (a pair that straddles the chunk boundary reads both activation buffers)
        const int wb1 = wb + 1 == NB ? 0 : wb + 1;
        const int t = odd ? tap1 : tap, ch = odd ? chunk1 : chunk, w = odd ? wb1 : wb;
        const int px0 = (wave * 2 + 1 + tap_dy(t)) * HW + c + 1 + tap_dx(t), px1 = px0 + HW;
        const unsigned ra0 = sA + ch * A_BYTES + slot_of(px0, half) * 16, ra1 = sA + ch * A_BYTES + slot_of(px1, half) * 16;
        const unsigned rb = sB + w * B_BYTES + slot_of(c, half) * 16;
        // pixel groups g = 2 (tile row) + (16-pixel half of the row): + 16 pixels = + 512 bytes, same swizzle bit
        lds_read<A_PLANE>(ga[0][1], ra0); lds_read<A_PLANE + 512>(ga[1][1], ra0); lds_read<A_PLANE>(ga[2][1], ra1); lds_read<A_PLANE + 512>(ga[3][1], ra1);
        lds_read<0>(gb[0][0], rb); lds_read<512>(gb[1][0], rb); lds_read<1024>(gb[2][0], rb); lds_read<1536>(gb[3][0], rb);
        lds_read<2048>(gb[4][0], rb); lds_read<2560>(gb[5][0], rb); lds_read<3072>(gb[6][0], rb); lds_read<3584>(gb[7][0], rb);
        lds_read<0>(ga[0][0], ra0); lds_read<512>(ga[1][0], ra0); lds_read<0>(ga[2][0], ra1); lds_read<512>(ga[3][0], ra1);
        lds_read<B_PLANE>(gb[0][1], rb); lds_read<B_PLANE + 512>(gb[1][1], rb); lds_read<B_PLANE + 1024>(gb[2][1], rb); lds_read<B_PLANE + 1536>(gb[3][1], rb);
        lds_read<B_PLANE + 2048>(gb[4][1], rb); lds_read<B_PLANE + 2560>(gb[5][1], rb); lds_read<B_PLANE + 3072>(gb[6][1], rb); lds_read<B_PLANE + 3584>(gb[7][1], rb);
    };
    auto tie32 = [&](int pa, int pb) { for (int m = 0; m < 2; ++m) tie(fa[m][pa]); for (int n = 0; n < 4; ++n) tie(fb[n][pb]); };
    auto tie16 = [&](int pa, int pb) { for (int g = 0; g < 4; ++g) tie(ga[g][pa]); for (int n = 0; n < 8; ++n) tie(gb[n][pb]); };
#define P32(PA, PB) _Pragma("unroll") for (int m = 0; m < 2; ++m) _Pragma("unroll") for (int n = 0; n < 4; ++n) acc[m][n] = mfma32(fb[n][PB], fa[m][PA], acc[m][n]);
#define P16(PA, PB) _Pragma("unroll") for (int g = 0; g < 4; ++g) _Pragma("unroll") for (int n = 0; n < 8; ++n) acd[g][n] = mfma16(gb[n][PB], ga[g][PA], acd[g][n]);
    if (!LDS) {
        if (SHAPE == 0) { read32(); lds_wait<0>(); tie32(1, 0); tie32(0, 1); }
        else { read16(); lds_wait<0>(); tie16(1, 0); tie16(0, 1); }
    }
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < iters; ++i) {
        if (SHAPE == 0) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (LDS) { read32(); lds_wait<6>(); tie32(1, 0); }
                P32(1, 0)
                if (LDS) { lds_wait<0>(); tie32(0, 1); }
                P32(0, 1) P32(0, 0)
                next();
            }
        } else {
            if (LDS) { read16(); lds_wait<12>(); tie16(1, 0); }
            P16(1, 0)
            if (LDS) { lds_wait<0>(); tie16(0, 1); }
            P16(0, 1) P16(0, 0)
            next(); next();
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
#undef P32
#undef P16
    float s = 0.f;
    if (SHAPE == 0) { for (int m = 0; m < 2; ++m) for (int n = 0; n < 4; ++n) for (int i = 0; i < 16; ++i) s += acc[m][n][i]; }
    else { for (int g = 0; g < 4; ++g) for (int n = 0; n < 8; ++n) for (int i = 0; i < 4; ++i) s += acd[g][n][i]; }
    out[blockIdx.x * 512 + tid] = s;
    if (blockIdx.x == 0 && tid == 0) { clk[0] = t1 - t0; clk[1] = r1 - r0; }
}

struct Bufs { float *out; unsigned long long *clk; uint4 *fill[2]; int cus; };

template <int SHAPE, int LDS>
static double run(const Bufs &b, int iters, int random_bits, const char *tag)
{
    hipFuncSetAttribute(reinterpret_cast<const void *>(k_loop<SHAPE, LDS>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((k_loop<SHAPE, LDS>), dim3(b.cus), dim3(512), LDS_BYTES, 0, b.out, b.clk, 200, b.fill[random_bits]);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL((k_loop<SHAPE, LDS>), dim3(b.cus), dim3(512), LDS_BYTES, 0, b.out, b.clk, iters, b.fill[random_bits]);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    if (hipGetLastError() != hipSuccess) { printf("launch failed\n"); exit(1); }
    float ms = 0.f;
    unsigned long long hclk[2];
    hipEventElapsedTime(&ms, e0, e1);
    hipMemcpy(hclk, b.clk, 16, hipMemcpyDeviceToHost);
    const int per_iter = SHAPE == 0 ? 48 : 96;                       // MFMAs of one wave per iteration
    const double flop = (double)b.cus * 8 * (double)iters * per_iter * (SHAPE == 0 ? 32768.0 : 16384.0);
    const double mhz = (double)hclk[0] / ((double)hclk[1] / 100.0);
    const double cyc = (double)hclk[0] / ((double)iters * per_iter * 2);     // per SIMD: two waves share it
    printf("%-5s %s, %s, %s operands: %8.3f ms, %4.0f TFLOP/s, shader clock %4.0f MHz, %5.2f clocks per MFMA per SIMD (%5.2f per 32x32x16's worth)\n",
           tag, SHAPE == 0 ? "32x32x16" : "16x16x32", LDS ? "12 ds_read_b128 per 24 / 24 per 96 MFMAs" : "operands in registers               ",
           random_bits ? "random" : "zero  ", ms, flop / ms / 1e9, mhz, cyc, SHAPE == 0 ? cyc : 2 * cyc);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return ms;
}

int main()
{
    hipDeviceProp_t p;
    hipGetDeviceProperties(&p, 0);
    Bufs b;
    b.cus = p.multiProcessorCount;
    printf("%s, %d CUs, clockRate %d kHz; 512 threads and %d bytes of LDS per workgroup, one workgroup per CU\n", p.name, b.cus, p.clockRate, LDS_BYTES);
    hipMalloc(&b.out, (size_t)b.cus * 512 * sizeof(float));
    hipMalloc(&b.clk, 16);
    std::vector<unsigned> h(LDS_BYTES / 4);
    srand(1);
    for (int rnd = 0; rnd < 2; ++rnd) {
        // random mantissas and signs with exponents near 1.0 (finite, no denormals), as in mfma_f16_rate.hip
        for (auto &w : h) w = rnd ? ((0x3800u | (rand() & 0x87ffu)) | ((0x3800u | (rand() & 0x87ffu)) << 16)) : 0u;
        hipMalloc(&b.fill[rnd], LDS_BYTES);
        hipMemcpy(b.fill[rnd], h.data(), LDS_BYTES, hipMemcpyHostToDevice);
    }
    const int iters = 100000;                           // ~ 0.15 - 0.2 s a run
    // warm-up: two seconds of the loaded loops, so that every measured run starts from the clock the chip holds under this load
    for (int k = 0; k < 6; ++k) { run<0, 1>(b, iters, 1, "warm"); run<1, 1>(b, iters, 1, "warm"); }
    double ms[2][3];
    for (int k = 0; k < 3; ++k) {                       // three alternating rounds a side
        ms[0][k] = run<0, 1>(b, iters, 1, "A/B");
        ms[1][k] = run<1, 1>(b, iters, 1, "A/B");
    }
    double lo[2], hi[2];
    for (int s = 0; s < 2; ++s) {
        lo[s] = hi[s] = ms[s][0];
        for (int k = 1; k < 3; ++k) { lo[s] = ms[s][k] < lo[s] ? ms[s][k] : lo[s]; hi[s] = ms[s][k] > hi[s] ? ms[s][k] : hi[s]; }
    }
    printf("wall, three alternating runs a side: 32x32x16 %.3f .. %.3f ms, 16x16x32 %.3f .. %.3f ms; slowest 16x16x32 / fastest 32x32x16 = %.4f, fastest / slowest = %.4f\n",
           lo[0], hi[0], lo[1], hi[1], hi[1] / lo[0], lo[1] / hi[0]);
    printf("verdict: 16x16x32 is %s\n", hi[1] < lo[0] ? "FASTER by more than the spread of the runs" : lo[1] > hi[0] ? "SLOWER by more than the spread of the runs" : "NOT SEPARABLE from 32x32x16 by these runs");
    run<0, 0>(b, iters, 1, "regs"); run<1, 0>(b, iters, 1, "regs");
    run<0, 0>(b, iters, 1, "regs"); run<1, 0>(b, iters, 1, "regs");
    run<0, 1>(b, iters, 0, "zero"); run<1, 1>(b, iters, 0, "zero");
    run<0, 0>(b, iters, 0, "zero"); run<1, 0>(b, iters, 0, "zero");
    return 0;
}
