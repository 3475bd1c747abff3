// tip_unet_first.h -- the U-Net's first layer, Conv2D(2 -> 128, 3x3) on the float32 (2, H, W) network input: the float32 vector kernel
// and, for the fp16 pieces, the same layer on the matrix cores.  The piece formats and the epilogue's helpers are tip_unet_conv.h's.
#pragma once
#include "tip_unet_conv.h"

namespace tip {

// ---- first layer: Conv2D(2 -> 128, 3x3) on the float32 (2, H, W) network input --------------------------------------------------
// The vector kernel: the bf16 modes' first layer (two bf16 pieces of the input would be less accurate than these exact FMAs), and
// mode f16x3's behind TIP_UNET_FIRST=valu; f16x3 runs k_unet_conv_first_mfma below by default.  K = 18 and float32 operands: nothing
// for the matrix cores here -- the layer is its 2.1 GB of output.  Exact float32 FMAs; a thread owns 4 adjacent output
// channels, keeps their 18 x 4 weights in registers and walks a run of FIRST_RUN consecutive pixels of one row with the 3 x 3 x 2
// input window sliding through registers (six loads and no address arithmetic per pixel: with per-pixel tap addressing the kernel
// was bound by its own index arithmetic, 210 vector instructions per pixel and thread, 0.8 ms against 0.45 ms for the stores
// alone).  Thirty-two threads share a pixel, so the split of two adjacent channels is one v_cvt_pk_bf16_f32 (no lane exchange) and
// a pixel's 256 bytes per piece leave in one piece.
constexpr int FIRST_RUN = 32;       // consecutive pixels per 32-thread slot; a 256-thread block covers 8 runs = 256 pixels of a row
constexpr int FIRST_PIX = 8 * FIRST_RUN;
template <int NPL, bool F16 = false>
__global__ void __launch_bounds__(256) k_unet_conv_first(const float *__restrict__ in, int H, int W, const float *__restrict__ wgt /* [9][2][128] */,
                                                         const float *__restrict__ bias, const float *__restrict__ scale,
                                                         const float *__restrict__ shift, uint16_t *__restrict__ out,
                                                         unsigned *__restrict__ status /* fp16 pieces: the range word (uc_range_flag) */)
{
    const int cg = threadIdx.x & 31, slot = threadIdx.x >> 5;
    float4 w4[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) w4[k] = *reinterpret_cast<const float4 *>(wgt + k * 128 + cg * 4);
    const float4 bb = *reinterpret_cast<const float4 *>(bias + cg * 4);
    const float4 ss = *reinterpret_cast<const float4 *>(scale + cg * 4);
    const float4 tt = *reinterpret_cast<const float4 *>(shift + cg * 4);
    const long plane = (long)H * W * 128, chan = (long)H * W;
    const long pix0 = (long)blockIdx.x * FIRST_PIX + slot * FIRST_RUN;        // (W % FIRST_RUN == 0: a run stays inside one row)
    const int y = (int)(pix0 / W), x0 = (int)(pix0 - (long)y * W);
    // the three input rows (clamped addresses, zero where the row lies outside the image: 'same' padding)
    const float *rowp[3];
    bool rowin[3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = y + dy - 1;
        rowin[dy] = yy >= 0 && yy < H;
        rowp[dy] = in + (long)min(max(yy, 0), H - 1) * W;
    }
    auto column = [&](int xx, float (&c)[3][2]) {          // input column xx of the window: [row][channel]
        const bool xin = xx >= 0 && xx < W;
        const int xc = min(max(xx, 0), W - 1);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const float a = rowp[dy][xc], b = rowp[dy][chan + xc];
            c[dy][0] = xin && rowin[dy] ? a : 0.f;
            c[dy][1] = xin && rowin[dy] ? b : 0.f;
        }
    };
    float win[3][3][2];          // [column slot][row][channel]; slot (it + k) % 3 holds column x - 1 + k
    column(x0 - 1, win[0]);
    column(x0, win[1]);
    uint16_t *dst = out + pix0 * 128 + cg * 4;
    float amax = 0.f;            // fp16 pieces: the thread's largest |value| in front of the clamp
    for (int it0 = 0; it0 < FIRST_RUN; it0 += 3) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {        // (unrolled by the window's period: every slot index is a compile-time constant)
            const int it = it0 + u;
            if (it >= FIRST_RUN) break;
            column(x0 + it + 1, win[(u + 2) % 3]);
            f32x2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};       // packed FMAs: two channels per instruction
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float v0 = win[(u + t % 3) % 3][t / 3][0], v1 = win[(u + t % 3) % 3][t / 3][1];
                a01 = __builtin_elementwise_fma(f32x2{v0, v0}, f32x2{w4[2 * t].x, w4[2 * t].y}, a01);
                a23 = __builtin_elementwise_fma(f32x2{v0, v0}, f32x2{w4[2 * t].z, w4[2 * t].w}, a23);
                a01 = __builtin_elementwise_fma(f32x2{v1, v1}, f32x2{w4[2 * t + 1].x, w4[2 * t + 1].y}, a01);
                a23 = __builtin_elementwise_fma(f32x2{v1, v1}, f32x2{w4[2 * t + 1].z, w4[2 * t + 1].w}, a23);
            }
            float a[4] = {a01[0] + bb.x, a01[1] + bb.y, a23[0] + bb.z, a23[1] + bb.w};
            const float sv[4] = {ss.x, ss.y, ss.z, ss.w}, tv[4] = {tt.x, tt.y, tt.z, tt.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float r = a[j] > 0.f ? a[j] : 0.f;
                a[j] = r * sv[j] + tv[j];
            }
            if constexpr (F16) {      // (s and t carry the activation scale)
                amax = uc_amax3(uc_amax3(amax, a[0], a[1]), a[2], a[3]);
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = uc_sat_f16(a[j]);
            }
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) {
                unsigned wd[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) wd[q] = uc_piece_word<F16>(a[2 * q], a[2 * q + 1], pl + 1 < NPL);
                *reinterpret_cast<uint2 *>(dst + (long)it * 128 + pl * plane) = make_uint2(wd[0], wd[1]);
            }
        }
    }
    if constexpr (F16) uc_range_flag(amax, status, threadIdx.x & 63);
}

// ---- the same layer on the matrix cores, fp16 pieces only (mode f16x3) ------------------------------------------------------------
// With a value held as two fp16 pieces the layer is "just another layer": an implicit im2col with K = 18 padded to 32 -- index
// k = 2 tap + channel (tap = 3 ky + kx, the order of the vector kernel's [9][2][128] weights), k = 18 .. 31 zero -- is two K steps of
// v_mfma_f32_32x32x16_f16, three products per term as in k_unet_conv: 24 MFMAs per 32 pixels x 128 channels, ~0.05 ms of the
// chip for 2048^2.  What is left is the epilogue k_unet_conv runs on the same bytes: about 13 wave instructions per pixel where the
// vector kernel above issues 60, so the layer is its 2.1 GB of stores.
//   * Weights (A operand) arrive packed like every layer's (host: _split_pack, one tap x 32 input channels, their own power-of-two
//     scale); a wave keeps its sixteen 16-byte fragments (4 blocks x 2 steps x 2 planes) in registers for its whole life.
//   * Pixels are the B operand: lane (pixel = lane & 31, g = lane >> 5) supplies k = 8 g .. 8 g + 7 of each step, i.e. taps
//     4 g .. 4 g + 3 in step 0 and (g = 0 only) tap 8 in step 1: at most ten float32 loads per lane and segment, clamped addresses and
//     a select to zero outside the image.  The values are scaled by the activation scale and split here; they pass through the
//     range check's running maximum in front of the clamp, so an input beyond the range raises the flag.
//   * A wave walks 32-pixel segments of a row (W % 32 == 0), segment s of wave g: g + s x (waves of the launch) -- neighbouring
//     waves store neighbouring 8 KB.  The next segment's input is loaded in front of the current one's epilogue.
//   * Epilogue: the math and the order of k_unet_conv's fp16 branch, one segment (its m = 0) at a time, through the wave's own
//     8.5 KB LDS image.
// UC_FIRST_STORES_ONLY (timing builds only, never the product): no input loads, no MFMAs -- the epilogue and the stores on their own.
constexpr int FIRST_MFMA_WGS_PER_CU = 2;                  // workgroups per CU a launch is cut to: as many as are resident (two waves per SIMD: 64 weight + 64 accumulator registers)
static __global__ void __launch_bounds__(256) k_unet_conv_first_mfma(const float *__restrict__ in, int H, int W,
                                                              const uint16_t *__restrict__ wgt /* packed [2 steps][1][2 planes][128][16] */,
                                                              float acc_scale, const float *__restrict__ bias, const float *__restrict__ scale,
                                                              const float *__restrict__ shift, uint16_t *__restrict__ out,
                                                              unsigned *__restrict__ status /* the range word (uc_range_flag) */)
{
#if defined(__HIP_DEVICE_COMPILE__)       // (the matrix-core builtins exist in the device pass only)
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * EP_BYTES];
    // The per-channel constants live in LDS: read from memory inside the loop, they would sit BEHIND the previous segment's stores in
    // the wave's vector-memory queue (one counter for loads and stores), and every segment would wait for its predecessor's 16 KB to
    // be acknowledged.  The only loads left in the loop are the next segment's input, issued in front of the stores.
    __shared__ __attribute__((aligned(16))) float cst[3][UC_BN];
    if (threadIdx.x < UC_BN) {
        cst[0][threadIdx.x] = bias[threadIdx.x];
        cst[1][threadIdx.x] = scale[threadIdx.x];
        cst[2][threadIdx.x] = shift[threadIdx.x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // (scalar: so are the segment, its row and the store's base)
    const int pxl = lane & 31, hf = lane >> 5;
    unsigned char *ep = smem + wave * EP_BYTES;
    const long chan = (long)H * W, plane = chan * 128;
    const int segs_row = W / 32;
    const long nseg = chan / 32, seg_step = (long)gridDim.x * 4;

    uint4 wf[2][2][4];          // weight fragments [step][plane][block of 32 channels]: row (block, lane & 31), k = 8 hf .. 8 hf + 7
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int n = 0; n < 4; ++n)
                wf[s][pl][n] = *reinterpret_cast<const uint4 *>(wgt + ((s * 2 + pl) * UC_BN + n * 32 + pxl) * UC_KC + hf * 8);

    // the lane's five taps: 4 hf + j (j < 4) and tap 8, which only half-wave 0 supplies (k = 16, 17 of step 1)
    int tdy[5], tdx[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int tap = j < 4 ? 4 * hf + j : 8;
        tdy[j] = tap / 3 - 1;
        tdx[j] = tap % 3 - 1;
    }
    const float *in1 = in + chan;
    // (raw values and a mask of the taps inside the image: the select is applied where the values are used, so nothing waits for a load at its issue)
    auto load_segment = [&](long seg, float (&v)[5][2], unsigned &inmask) {
#ifndef UC_FIRST_STORES_ONLY
        const int y = (int)(seg / segs_row), x = (int)(seg - (long)y * segs_row) * 32 + pxl;
        unsigned m = 0u;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int yy = y + tdy[j], xx = x + tdx[j];
            const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W && (j < 4 || hf == 0);
            const unsigned o = (unsigned)(min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1));     // (H W < 2^30: the output is 512 bytes per pixel)
            v[j][0] = in[o];
            v[j][1] = in1[o];
            m |= inside ? 1u << j : 0u;
        }
        inmask = m;
#else
#pragma unroll
        for (int j = 0; j < 5; ++j) v[j][0] = v[j][1] = 0.f;
        inmask = 0u;
#endif
    };

    const f32x2 inv2 = {acc_scale, acc_scale};
    const unsigned coff = 16 * hf;                                 // the lane's sixteen channels of a 32-channel block
    const int rd_row = lane >> 4, rd_col = (lane & 15) * 16;       // read-back: 16 lanes = one pixel's 256 bytes
    float amax = 0.f;           // the lane's largest |value| in front of a clamp, inputs and outputs alike
    long seg = (long)blockIdx.x * 4 + wave;
    float cur[5][2];
    unsigned curmask = 0u;
    if (seg < nseg) {
        load_segment(seg, cur, curmask);
#pragma unroll
        for (int j = 0; j < 5; ++j) asm volatile("" : "+v"(cur[j][0]), "+v"(cur[j][1]));     // (landed in front of the loop: inside it the wait counts only the stores behind the loads)
    }
    for (; seg < nseg; seg += seg_step) {
        // B fragments: the ten values times the activation scale, split into fp16 pieces (words j: taps of step 0; word 4: tap 8)
        unsigned bhi[5], blo[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            asm volatile("" : "+v"(cur[j][0]), "+v"(cur[j][1]));      // (waited for HERE, behind the previous segment's stores, not where they were issued)
            const bool inside = (curmask >> j) & 1u;
            float a = inside ? cur[j][0] * 16.f : 0.f, b = inside ? cur[j][1] * 16.f : 0.f;      // (16: the activation scale of the fp16 pieces, _F16_ACT_SCALE)
            amax = uc_amax3(amax, a, b);
            a = uc_sat_f16(a);
            b = uc_sat_f16(b);
            bhi[j] = uc_piece_word<true>(a, b, true);
            blo[j] = uc_piece_word<true>(a, b, false);
        }
        if (seg + seg_step < nseg) load_segment(seg + seg_step, cur, curmask);     // (in flight behind the products and the epilogue)
        asm volatile("" ::: "memory");       // (the loads stay here, in front of this segment's stores: see cst)
        const uint4 xh[2] = {make_uint4(bhi[0], bhi[1], bhi[2], bhi[3]), make_uint4(bhi[4], 0u, 0u, 0u)};
        const uint4 xl[2] = {make_uint4(blo[0], blo[1], blo[2], blo[3]), make_uint4(blo[4], 0u, 0u, 0u)};
        f32x16 acc[4];
#ifndef UC_FIRST_STORES_ONLY
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
        // products from the smallest magnitude class to the largest: lo x hi, hi x lo, hi x hi (weights = the A operand)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = uc_mfma<true>(wf[s][0][n], xl[s], acc[n]);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = uc_mfma<true>(wf[s][1][n], xh[s], acc[n]);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = uc_mfma<true>(wf[s][0][n], xh[s], acc[n]);
#else
        {
            float z = __uint_as_float(xh[0].x | xl[1].x);      // (zero, but not to the compiler: the epilogue stays inside the loop)
            asm volatile("" : "+v"(z));
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[n][i] = z;
        }
#endif
        // epilogue: accumulator x acc_scale + bias -> ReLU -> BatchNorm scale / shift (both carry the activation scale) -> range
        // check -> clamp (uc_activate4, as in k_unet_conv); a lane holds channels n * 32 + 16 hf + i of its pixel
#pragma unroll
        for (int n = 0; n < 4; ++n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b = *reinterpret_cast<const float4 *>(&cst[0][coff + n * 32 + q * 4]);
                const float4 s = *reinterpret_cast<const float4 *>(&cst[1][coff + n * 32 + q * 4]), t = *reinterpret_cast<const float4 *>(&cst[2][coff + n * 32 + q * 4]);
                f32x2 v01 = {acc[n][q * 4 + 0], acc[n][q * 4 + 1]}, v23 = {acc[n][q * 4 + 2], acc[n][q * 4 + 3]};
                uc_activate4<true>(v01, v23, b, s, t, inv2, amax);
                acc[n][q * 4 + 0] = v01[0]; acc[n][q * 4 + 1] = v01[1];
                acc[n][q * 4 + 2] = v23[0]; acc[n][q * 4 + 3] = v23[1];
            }
        }
        // split and store: one piece at a time through the wave's LDS image, read back four whole pixels per store instruction (EP_ROW of tip_unet_conv.h)
        uint16_t *orow = out + seg * 32 * 128;
        const unsigned ooff = (unsigned)((lane & 15) * 8 + rd_row * 128);
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = acc[n][q * 8 + j];
                    const uint4 w = uc_pack8<true>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], pl == 0);
                    if (pl == 0) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[n][q * 8 + j] = v[j];
                    }
                    *reinterpret_cast<uint4 *>(ep + pxl * EP_ROW + (n * 32 + 16 * hf + 8 * q) * 2) = w;
                }
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int row = it * 4 + rd_row;
                *reinterpret_cast<uint4 *>(orow + pl * plane + it * 4 * 128 + ooff) = *reinterpret_cast<const uint4 *>(ep + row * EP_ROW + rd_col);
            }
        }
    }
    uc_range_flag(amax, status, lane);
#endif
}

}  // namespace tip
