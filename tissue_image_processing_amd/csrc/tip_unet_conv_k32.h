// tip_unet_conv_k32.h -- k_unet_conv's two-piece fp16 arithmetic (f16x3) on v_mfma_f32_16x16x32_f16, for stencils of four and more
// taps: on 16-row tiles (512 threads, one workgroup per CU) and, asked for by flag, on 8-row tiles (256 threads, two per CU).  Why: the pass runs at the board's power limit, and the clock the chip holds there depends on the MFMA
// shape -- at this kernel's wave tile and LDS traffic the 16x16x32 loop runs 12 % faster by wall than the 32x32x16 one
// (tools/ubench/mfma_f16_shape_lds.hip).  Everything around the products is tip_unet_conv.h's: the packed weights, the
// LDS image (32-byte rows with the XOR swizzle, filled by asynchronous copies), the descriptor, the epilogue's five forms.
// Shared as CODE, not as a copy: the tile layout (UcLayout<2, 16, 4> / UcLayout<2, 8, 2>: the kernel's template parameter), the swizzle (uc_slot) and its conflict check
// (uc_conflict_free, here under this kernel's read pattern), the copy plans and the copies (UcCopies), the workgroup map
// (uc_workgroup) and the (chunk, tap) stepper (uc_next_step).  This file has what differs: the lane maps, the pair step's products
// and schedule, the weight ring, and the epilogue and seed loads on this kernel's lane map.
//
// The K = 32 pair step.  The instruction contracts 32 K values, a chunk has 16 channels, and a 32-channel chunk does not fit LDS.
// So K = 32 is formed from two CONSECUTIVE (chunk, tap) steps of the linear step order: lanes 0-31 (K-groups 0 / 1: the two
// 8-channel halves of a row) read step 2j, lanes 32-63 (K-groups 2 / 3) step 2j + 1, for both operands.  The weight tile and the
// shifted activation window of every step lie where tip_unet_conv.h puts them; only the per-lane read addresses differ.  A pair
// step is 24 ds_read_b128 and 96 MFMAs of a wave, one barrier per pair step.
//   * Odd tap counts: one pair in two chunks straddles the chunk boundary (and possibly in0 / in1) and reads both activation
//     buffers.
//   * An odd step count: the last step is alone.  Lanes 32-63 then read the same step as lanes 0-31 (finite values, not whatever
//     the ring holds) and their activation fragments are zeroed in registers: once per workgroup.
//   * 16-row tiles.  Weight ring: three pair steps = six 8 KB tiles.  With the two 40 KB activation buffers: 128 KB.  The
//     workgroup's barrier stands in the MIDDLE of a pair step; the copies of pair j + 2 and of the next chunk go out right behind
//     it (the main loop has the ordering argument).
//   * 8-row tiles.  Two workgroups share a CU, so a workgroup has 80 KB: two 24 KB activation buffers and a ring of TWO pair steps
//     (four tiles).  A ring of two cannot carry the middle barrier -- pair j + 1 would land in the slots pair j - 1's second half
//     still reads -- so the barrier stands BETWEEN pair steps and the copies of pair j + 1 go out behind the one that opens pair j.
// Everything per wave is the same in both: lane maps, reads, products and their order, the epilogue.
// Lane maps.  Weights stay the A operand (M = output channels).  MFMA row rho of a 16-row block reads stored weight row
// uk_map16(rho), MFMA column j reads pixel uk_map16(j) of a 16-pixel group: 8-11 <-> 12-15.  With ds_read_b128's lane groups and the
// swizzle the identity order conflicts two-way; this order is conflict-free for 16 consecutive rows or pixels at any alignment
// (static_asserts below).  A lane ends up with ONE pixel per 16-pixel group (4 groups: 2 tile rows x 2 halves of the 32 columns)
// and FOUR adjacent channels per 16-row block (8 blocks): channel uk_chan(K-group) + 32 (n >> 1) + 8 (n & 1) + i.
#pragma once
#include "tip_unet_conv.h"
#include <type_traits>

namespace tip {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int uk_map16(int i) { return i < 8 ? i : i ^ 4; }                          // stored row / pixel of MFMA row / column i
// first channel (inside a 32-channel block pair n >> 1, plus 8 (n & 1)) of the four a lane of K-group kq (lane >> 4) holds: MFMA
// rows 4 kq .. 4 kq + 3 are stored rows 4 kq' .. with kq' = 0, 1, 3, 2, and stored row 8 g + 4 h + j holds channel 16 h + 4 g + j
constexpr int uk_chan(int kq) { return 16 * ((kq < 2 ? kq : kq ^ 1) & 1) + 4 * ((kq < 2 ? kq : kq ^ 1) >> 1); }
struct UkRead16 {                             // both operands: 16 consecutive rows / pixels in uk_map16's order, a half per K-group parity
    static constexpr int row(int lane) { return uk_map16(lane & 15); }
    static constexpr int half(int lane) { return (lane >> 4) & 1; }
};
constexpr bool uk_conflict_free() { return uc_conflict_free<UkRead16>(); }      // (uc_slot's swizzle under this kernel's read pattern)
constexpr bool uk_bijective()
{
    unsigned rows = 0, chans = 0;
    for (int i = 0; i < 16; ++i) rows |= 1u << uk_map16(i);
    for (int n = 0; n < 2; ++n)                          // the 32 channels of a block: two 16-row blocks x four K-groups x four registers
        for (int kq = 0; kq < 4; ++kq)
            for (int i = 0; i < 4; ++i) {
                const int ch = uk_chan(kq) + 8 * n + i;
                // the same channel by the stored-row route: MFMA row 4 kq + i of block n -> stored row -> split_pack's channel
                const int r32 = 16 * n + uk_map16(4 * kq + i), via_row = 16 * ((r32 >> 2) & 1) + 4 * (r32 >> 3) + (r32 & 3);
                if (ch != via_row || (chans & (1u << ch))) return false;
                chans |= 1u << ch;
            }
    return rows == 0xffffu && chans == 0xffffffffu;
}
static_assert(uk_bijective(), "the row / pixel map is a permutation and a lane's channels are what the packed rows hold");
static_assert(uk_conflict_free(), "16 different bank quads per lane group of ds_read_b128, at every alignment");

__device__ __forceinline__ f32x4 uk_mfma(const u32x4 &a, const u32x4 &b, const f32x4 &c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <int N>
__device__ __forceinline__ void uc_lds_wait(u32x4 &a, u32x4 &b, u32x4 &c, u32x4 &d, u32x4 &e)
{
    asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : "n"(N));
}

// What a K = 32 launch adds to its tile layout L (tip_unet_conv.h: UcLayout; the tiles are those of k_unet_conv<2, 16, 4> resp.
// <2, 8, 2>): where the workgroup's barrier stands, the weight ring, and with it the LDS size.  The launch table reads THREADS and LDS.
template <typename L>
struct UkLaunch {
    static constexpr bool MID = L::ROWS == 16;                         // the barrier in the middle of a pair step (else: between two)
    static constexpr int AHEAD = MID ? 2 : 1;                          // pair steps the weight copies run ahead
    static constexpr int NB = 2 * (AHEAD + 1);                         // weight tiles: three pair steps / two
    static constexpr int THREADS = L::THREADS;
    static constexpr int LDS = 2 * L::A_BYTES + NB * L::B_BYTES;       // two activation buffers and the ring
    static_assert(L::ROWS == 16 || L::ROWS == 8, "two tile rows per wave, eight waves or four");
    static_assert(THREADS / 64 * EP_BYTES <= LDS, "the staging images fit the tile buffers");
};
using UkTiles16 = UcLayout<2, 16, 4>;         // 512 threads; 128 KB: two 40 KB activation buffers, six 8 KB tiles
using UkTiles8 = UcLayout<2, 8, 2>;           // 256 threads;  80 KB: two 24 KB activation buffers, four 8 KB tiles
static_assert(UkLaunch<UkTiles16>::LDS == 128 * 1024, "one 16-row workgroup per CU");
static_assert(2 * UkLaunch<UkTiles8>::LDS == 160 * 1024, "two 8-row workgroups are resident: each has exactly half a CU's LDS");

template <typename UkTiles>
__global__ void __launch_bounds__(UkTiles::THREADS, 2) k_unet_conv_k32(const ConvParams p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr bool F16 = true;
    using K = UkLaunch<UkTiles>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *sA = smem, *sB = smem + 2 * UkTiles::A_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tilesX = p.W / UC_TW;
    const UcWorkgroup wg = uc_workgroup(p);
    const int nblk = wg.nblk;
    const int ty0 = (wg.tile / tilesX) * UkTiles::ROWS, tx0 = (wg.tile % tilesX) * UC_TW;
    const int cin = p.c0 + p.c1, nchunks = cin / UC_KC, nsteps = nchunks * p.ntaps;
    UcCopies<2, UkTiles> cp(p, sA, sB, tid, wave, ty0, tx0, nblk);       // the tile copies (tip_unet_conv.h)

    // Accumulators: [pixel group g = 2 (tile row) + (16-pixel half)][16-row block n]; the lane's pixel and channels: see the top
    f32x4 acd[4][8];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int n = 0; n < 8; ++n)
#pragma unroll
            for (int i = 0; i < 4; ++i) acd[g][n][i] = 0.f;

    const int kq = lane >> 4, khalf = kq & 1, odd = lane >> 5;
    const int c16 = uk_map16(lane & 15);                 // the lane's pixel inside a 16-pixel group, and its weight row inside a 16-row block
    const int cbch = uk_chan(kq);

    // prologue: activation chunk 0, the weight tiles of the first AHEAD pair steps (a step that does not exist: the last one again --
    // every wave issues the same number of copies, and nothing reads the tile)
    cp.copy_a(0, 0);
    for (int s0 = 0; s0 < 2 * K::AHEAD; ++s0) {
        const int st = min(s0, nsteps - 1);
        cp.copy_b(st / p.ntaps, st % p.ntaps, s0);
    }
    if (p.seed) {
        const float up = 1.f / p.acc_scale;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float *sp = p.seed + ((long)(ty0 + wave * 2 + (g >> 1)) * p.W + tx0 + 16 * (g & 1) + c16) * p.cout + nblk * UC_BN + cbch;
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const float4 v = *reinterpret_cast<const float4 *>(sp + 32 * (n >> 1) + 8 * (n & 1));
                acd[g][n][0] = v.x * up; acd[g][n][1] = v.y * up; acd[g][n][2] = v.z * up; acd[g][n][3] = v.w * up;
            }
        }
    }
    uc_wait_barrier<0>();

    const unsigned sA_addr = uc_lds_addr(sA), sB_addr = uc_lds_addr(sB);
    const unsigned b_lane = (unsigned)(uc_slot(c16, khalf) * 16);
    u32x4 ga[4][2], gb[8][2];           // [pixel group][piece], [16-row block][piece]
    // products from the smallest magnitude class to the largest, per accumulator: lo x hi, hi x lo, hi x hi (as tip_unet_conv.h)
#define UK_ROW(N_, PA, PB)                                                                                      \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) acd[g][N_] = uk_mfma(gb[N_][PB], ga[g][PA], acd[g][N_]);
    // One pair step.  (ca, ta) / (cb, tb): (chunk, tap) of the lanes' steps 2j / 2j + 1; wbuf: the ring tile of step 2j.
    // `head` runs behind the first reads' issue, `mid` between the two halves: the loop's copies and barrier (see there).
    auto pair_products = [&](auto tail_c, int ca, int ta, int cb2, int tb2, int wbuf, auto &&head, auto &&mid) {
        constexpr bool TAIL = decltype(tail_c)::value;
        const int dya = p.dy[ta], dxa = p.dx[ta], dyb = p.dy[tb2], dxb = p.dx[tb2];
        const int dyl = odd ? dyb : dya, dxl = odd ? dxb : dxa, cl = odd ? cb2 : ca;
        const int px0 = (wave * 2 + 1 + dyl) * UC_HW + c16 + 1 + dxl, px1 = px0 + UC_HW;
        const unsigned abase = sA_addr + (unsigned)((cl & 1) * UkTiles::A_BYTES);
        const unsigned ra0 = abase + (unsigned)(uc_slot(px0, khalf) * 16), ra1 = abase + (unsigned)(uc_slot(px1, khalf) * 16);
        const unsigned rb = sB_addr + (unsigned)((wbuf + (TAIL ? 0 : odd)) * UkTiles::B_BYTES) + b_lane;
        constexpr int AP = UkTiles::A_PLANE * 16, BP = 256 * 16, XH = 16 * 32, BN = 16 * 32;     // + 16 pixels / + 16 rows: the same swizzle bit
        // The eight 16-row blocks go in two halves, so that 64 registers of fragments are live: the four activation fragments of
        // both pieces stay, the weight fragments of a half are read as the registers of the half before fall free.  Reads return in
        // order; W(N, ...) waits until at most N are out (the unpaired last step: for all of them) and ties the fragments it names.
#define UK_W(N_, ...) uc_lds_wait<TAIL ? 0 : N_>(__VA_ARGS__)
        auto zero_upper = [&](int pl) {                  // the unpaired last step: K-groups 2 / 3 contribute nothing
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int q = 0; q < 4; ++q) ga[g][pl][q] = odd ? 0u : ga[g][pl][q];
        };
        uc_lds_read<AP>(ga[0][1], ra0); uc_lds_read<AP + XH>(ga[1][1], ra0); uc_lds_read<AP>(ga[2][1], ra1); uc_lds_read<AP + XH>(ga[3][1], ra1);
        uc_lds_read<0>(gb[0][0], rb); uc_lds_read<BN>(gb[1][0], rb); uc_lds_read<2 * BN>(gb[2][0], rb); uc_lds_read<3 * BN>(gb[3][0], rb);
        __builtin_amdgcn_sched_barrier(0);
        head();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        UK_W(3, ga[0][1], ga[1][1], ga[2][1], ga[3][1], gb[0][0]);
        if constexpr (TAIL) zero_upper(1);
        UK_ROW(0, 1, 0)
        __builtin_amdgcn_sched_barrier(0);
        uc_lds_read<0>(ga[0][0], ra0); uc_lds_read<XH>(ga[1][0], ra0); uc_lds_read<0>(ga[2][0], ra1); uc_lds_read<XH>(ga[3][0], ra1);
        uc_lds_read<BP>(gb[0][1], rb); uc_lds_read<BP + BN>(gb[1][1], rb); uc_lds_read<BP + 2 * BN>(gb[2][1], rb); uc_lds_read<BP + 3 * BN>(gb[3][1], rb);
        __builtin_amdgcn_sched_barrier(0);
        UK_W(10, gb[1][0]);
        UK_ROW(1, 1, 0)
        UK_W(9, gb[2][0]);
        UK_ROW(2, 1, 0)
        UK_W(8, gb[3][0]);
        UK_ROW(3, 1, 0)
        UK_W(3, ga[0][0], ga[1][0], ga[2][0], ga[3][0], gb[0][1]);
        if constexpr (TAIL) zero_upper(0);
        UK_ROW(0, 0, 1)
        UK_W(2, gb[1][1]);
        UK_ROW(1, 0, 1)
        UK_W(1, gb[2][1]);
        UK_ROW(2, 0, 1)
        UK_W(0, gb[3][1]);
        UK_ROW(3, 0, 1)
        __builtin_amdgcn_sched_barrier(0);
        uc_lds_read<4 * BN>(gb[4][0], rb); uc_lds_read<5 * BN>(gb[5][0], rb); uc_lds_read<6 * BN>(gb[6][0], rb); uc_lds_read<7 * BN>(gb[7][0], rb);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 4; ++n) { UK_ROW(n, 0, 0) }
        __builtin_amdgcn_sched_barrier(0);
        uc_lds_read<BP + 4 * BN>(gb[4][1], rb); uc_lds_read<BP + 5 * BN>(gb[5][1], rb); uc_lds_read<BP + 6 * BN>(gb[6][1], rb); uc_lds_read<BP + 7 * BN>(gb[7][1], rb);
        __builtin_amdgcn_sched_barrier(0);
        mid();
        __builtin_amdgcn_sched_barrier(0);
        UK_W(7, gb[4][0]);
        UK_ROW(4, 1, 0)
        UK_W(6, gb[5][0]);
        UK_ROW(5, 1, 0)
        UK_W(5, gb[6][0]);
        UK_ROW(6, 1, 0)
        UK_W(4, gb[7][0]);
        UK_ROW(7, 1, 0)
        UK_W(3, gb[4][1]);
        UK_ROW(4, 0, 1)
        UK_W(2, gb[5][1]);
        UK_ROW(5, 0, 1)
        UK_W(1, gb[6][1]);
        UK_ROW(6, 0, 1)
        UK_W(0, gb[7][1]);
        UK_ROW(7, 0, 1)
#pragma unroll
        for (int n = 4; n < 8; ++n) { UK_ROW(n, 0, 0) }
#undef UK_W
        __builtin_amdgcn_s_setprio(0);
    };

    {
        int c0 = 0, t0 = 0;                              // (chunk, tap) of the pair's first step
        int cw = 2 * K::AHEAD / p.ntaps, tw = 2 * K::AHEAD % p.ntaps;      // ... and of the next weight copy (AHEAD pair steps ahead)
        int pb = 0;                                      // the pair's place in the ring (tiles 2 pb, 2 pb + 1)
        int a_issued = 0;                                // highest chunk whose activations are on their way (chunk 0: prologue)
        // 16-row tiles.  The workgroup's barrier stands in the MIDDLE of a pair step, not between two: a wave that has issued the
        // pair's last read waits there until its copies of the next pair's tiles have landed (issued a pair step ago), and behind the barrier
        //   * every wave's copies of pair j + 1 have landed, so a wave goes from pair j's last product straight to pair j + 1's
        //     reads -- no barrier, no first-operand latency with an empty matrix pipe between two pair steps;
        //   * every wave has read all of pair j - 1, so the copies of pair j + 2 (its place in the ring) and, when pair j BEGINS
        //     inside chunk c, of chunk c + 1 (the buffer of chunk c - 1) go out right there, in front of the second half's products.
        // The next chunk is then waited for at the next middle barrier, a pair step before its first read at the earliest (t0 is 0
        // or 1 where it is issued, and the stencils have four taps and more); a_due covers the case that is not.
        // 8-row tiles.  The barrier stands BETWEEN pair steps (the ring of two, see the top).  Behind the barrier that opens pair j
        // every wave has read all of pair j - 1, so the copies of pair j + 1 (pair j - 1's place) and of chunk c + 1 (as above:
        // the buffer of chunk c - 1, which pair j, beginning in chunk c, does not read) go out there -- behind the issue of the
        // pair's first reads, which do not wait for them.  In front of the barrier that closes pair j a wave waits for its own
        // copies: a whole pair step of flight.  A chunk issued where t0 is 0 or 1 is first read by a LATER pair (four taps and
        // more), so it has landed and been waited for: no a_due here.
        for (int s = 0; s + 1 < nsteps; s += 2) {
            int c1 = c0, t1 = t0;
            uc_next_step(c1, t1, p.ntaps);
            const bool issue_a = c0 + 1 < nchunks && c0 + 1 > a_issued;
            const int ca = c0 + 1;
            const bool issue_b = s + 2 * K::AHEAD < nsteps;
            auto copies = [&]() {
                if (issue_a) { a_issued = ca; cp.copy_a(ca, ca & 1); }
                if (issue_b) {
                    const int wb = 2 * (K::MID ? (pb == 0 ? 2 : pb - 1) : pb ^ 1);       // pair j + AHEAD takes the place pair j - 1 had
                    const int cw0 = cw, tw0 = tw;
                    cp.copy_b(cw0, tw0, wb);
                    uc_next_step(cw, tw, p.ntaps);
                    if (s + 2 * K::AHEAD + 1 < nsteps) { cp.copy_b(cw, tw, wb + 1); uc_next_step(cw, tw, p.ntaps); }
                    else cp.copy_b(cw0, tw0, wb + 1);       // (an odd step count: the unpaired step's tile twice, the second one unread)
                }
            };
            if constexpr (K::MID) {
                const bool a_due = issue_a && t0 + 3 >= p.ntaps;
                pair_products(std::false_type{}, c0, t0, c1, t1, 2 * pb, []() {}, [&]() {
                    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                    copies();
                });
                if (a_due) uc_wait_barrier<0>();
            } else {
                pair_products(std::false_type{}, c0, t0, c1, t1, 2 * pb, copies, []() {});
                uc_wait_barrier<0>();
            }
            c0 = c1; t0 = t1;
            uc_next_step(c0, t0, p.ntaps);
            pb = pb == K::AHEAD ? 0 : pb + 1;
        }
        // an odd step count: the last step alone, behind the loop (inside it, a second product path makes the compiler spill the
        // accumulators); its tile landed in front of the last barrier
        if (nsteps & 1) pair_products(std::true_type{}, c0, t0, c0, t0, 2 * pb, []() {}, []() {});
        // the epilogue writes its staging images over the tile buffers (8-row tiles, even step count: the loop's last barrier was that one)
        if (K::MID || (nsteps & 1)) uc_wait_barrier<0>();
    }
#undef UK_ROW

    // ---- epilogue: tip_unet_conv.h's five forms on this kernel's lane map ------------------------------------------------------------
    // No barrier in front (every wave is past the last pair's barrier, behind which no copy is in flight and no fragment unread).
    int px16 = c16, ch0 = cbch, kqe = kq;
    asm volatile("" : "+v"(px16), "+v"(ch0), "+v"(kqe));       // (opaque: none of the epilogue's addressing is hoisted into the main loop)
    unsigned char *ep = smem + wave * EP_BYTES;
    if (p.raw_out) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int y = ty0 + wave * 2 + (g >> 1);
            float *op = p.raw_out + ((long)(y * p.sy + p.oy) * p.outW + ((long)(tx0 + 16 * (g & 1) + px16) * p.sx + p.ox)) * p.cout + nblk * UC_BN + ch0;
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                float4 v = {acd[g][n][0], acd[g][n][1], acd[g][n][2], acd[g][n][3]};
                v.x *= p.acc_scale; v.y *= p.acc_scale; v.z *= p.acc_scale; v.w *= p.acc_scale;
                *reinterpret_cast<float4 *>(op + 32 * (n >> 1) + 8 * (n & 1)) = v;
            }
        }
        return;
    }
    {
        const float *bip = p.bias + nblk * UC_BN + ch0;
        const float *scp = p.scale + nblk * UC_BN + ch0, *shp = p.shift + nblk * UC_BN + ch0;
        const f32x2 inv2 = {p.acc_scale, p.acc_scale};
        float amax = 0.f;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int co = 32 * (n >> 1) + 8 * (n & 1);
            const float4 b = *reinterpret_cast<const float4 *>(bip + co);
            if (p.scale) {
                const float4 s = *reinterpret_cast<const float4 *>(scp + co), t = *reinterpret_cast<const float4 *>(shp + co);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x2 v01 = {acd[g][n][0], acd[g][n][1]}, v23 = {acd[g][n][2], acd[g][n][3]};
                    uc_activate4<F16>(v01, v23, b, s, t, inv2, amax);
                    acd[g][n][0] = v01[0]; acd[g][n][1] = v01[1]; acd[g][n][2] = v23[0]; acd[g][n][3] = v23[1];
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x2 v01 = {acd[g][n][0], acd[g][n][1]}, v23 = {acd[g][n][2], acd[g][n][3]};
                    uc_activate4<F16>(v01, v23, b, inv2, amax);
                    acd[g][n][0] = v01[0]; acd[g][n][1] = v01[1]; acd[g][n][2] = v23[0]; acd[g][n][3] = v23[1];
                }
            }
            if (n & 1) asm volatile("" ::: "memory");
        }
        uc_range_flag(amax, p.status, lane);
    }
    if (p.head_out) {
        // the fused head: a lane holds 32 of its four pixels' 128 channels, the other 96 sit in the lanes of the other K-groups
        // (lane ^ 16, lane ^ 32); K-group g then writes pixel group g
        float z[4][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
        const float *hw0 = p.head_w + ch0, *hw1 = p.head_w + UC_BN + ch0;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int co = 32 * (n >> 1) + 8 * (n & 1);
            const float4 a4 = *reinterpret_cast<const float4 *>(hw0 + co), b4 = *reinterpret_cast<const float4 *>(hw1 + co);
            const float wa[4] = {a4.x, a4.y, a4.z, a4.w}, wb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    z[g][0] = __builtin_fmaf(acd[g][n][j], wa[j], z[g][0]);
                    z[g][1] = __builtin_fmaf(acd[g][n][j], wb[j], z[g][1]);
                }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                z[g][c] += __shfl_xor(z[g][c], 16, 64);
                z[g][c] += __shfl_xor(z[g][c], 32, 64);
            }
        const float s0 = kqe == 0 ? z[0][0] : kqe == 1 ? z[1][0] : kqe == 2 ? z[2][0] : z[3][0];
        const float s1 = kqe == 0 ? z[0][1] : kqe == 1 ? z[1][1] : kqe == 2 ? z[2][1] : z[3][1];
        const long o = (long)(ty0 + wave * 2 + (kqe >> 1)) * p.W + tx0 + 16 * (kqe & 1) + px16;
        uc_softmax2(s0 + p.head_b[0], s1 + p.head_b[1], p.head_out, o, (long)p.H * p.W + o);
        return;
    }
    // Staging image as in tip_unet_conv.h ([32 pixels][128 channels] of one piece, 272-byte rows); a lane's channels come in fours,
    // so it writes 8 bytes at a time.  Read-back and stores are unchanged: 16 lanes = one pixel's 256 bytes.
    const int rd_row = lane >> 4, rd_col = (lane & 15) * 16;
    const long out_plane = (long)p.outH * p.outW * p.cout;
    if (p.pool_out) {
        // the 2 x 2 window of a pooled pixel: the lane's two tile rows (groups g and g + 2) x the neighbouring lane (pixels
        // uk_map16(j) and uk_map16(j ^ 1) are neighbours).  Both lanes of a pair hold the maxima: the even pixel's lane writes the
        // even 16-row blocks, the odd one's the odd blocks.
        const long pool_plane = (long)(p.outH / 2) * (p.outW / 2) * p.cout;
        const bool oddp = px16 & 1;
        float q4[2][4][4];
#pragma unroll
        for (int xh = 0; xh < 2; ++xh)
#pragma unroll
            for (int n = 0; n < 8; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = fmax_pair(fmax_raw(acd[xh][n][i], acd[2 + xh][n][i]));
                    if (!(n & 1)) q4[xh][n >> 1][i] = v; else if (oddp) q4[xh][n >> 1][i] = v;
                }
        uint16_t *prow = p.pool_out + ((long)(ty0 / 2 + wave) * (p.outW / 2) + tx0 / 2) * p.cout + nblk * UC_BN + (lane & 15) * 8;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
            for (int xh = 0; xh < 2; ++xh)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint2 w;
                    w.x = uc_piece_word<F16>(q4[xh][k][0], q4[xh][k][1], pl == 0);
                    w.y = uc_piece_word<F16>(q4[xh][k][2], q4[xh][k][3], pl == 0);
                    *reinterpret_cast<uint2 *>(ep + (8 * xh + (px16 >> 1)) * EP_ROW + (ch0 + 32 * k + (oddp ? 8 : 0)) * 2) = w;
                }
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int row = it * 4 + rd_row;
                *reinterpret_cast<uint4 *>(prow + pl * pool_plane + (long)row * p.cout) = *reinterpret_cast<const uint4 *>(ep + row * EP_ROW + rd_col);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int y = ty0 + wave * 2 + m;
        uint16_t *orow = p.out + ((long)(y * p.sy + p.oy) * p.outW + ((long)tx0 * p.sx + p.ox)) * p.cout + nblk * UC_BN + (lane & 15) * 8;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
            for (int xh = 0; xh < 2; ++xh)
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = acd[2 * m + xh][n][j];
                    uint2 w;
                    w.x = uc_piece_word<F16>(v[0], v[1], pl == 0);
                    w.y = uc_piece_word<F16>(v[2], v[3], pl == 0);
                    if (pl == 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acd[2 * m + xh][n][j] = v[j];
                    }
                    *reinterpret_cast<uint2 *>(ep + (16 * xh + px16) * EP_ROW + (ch0 + 32 * (n >> 1) + 8 * (n & 1)) * 2) = w;
                }
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int row = it * 4 + rd_row;
                *reinterpret_cast<uint4 *>(orow + pl * out_plane + (long)row * p.sx * p.cout) = *reinterpret_cast<const uint4 *>(ep + row * EP_ROW + rd_col);
            }
        }
    }
#endif
}

}  // namespace tip
