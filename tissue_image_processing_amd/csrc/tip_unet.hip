// tip_unet.hip -- the U-Net's layers: the launchers of the hand-written kernels on split planes (tip_unet_conv.h, tip_unet_first.h,
// tip_unet_planes.h), the convolutions' launch table (per flavour code: kernel, threads and LDS size of everything that can be launched,
// taken from the kernels' own layout constants) and the one function that picks from it, the fp16 pieces' range word, and the torch
// path's epilogue.
//
// The torch path (the convolutions left to PyTorch-ROCm / MIOpen): epilogue of the U-Net's convolutions (pl.py:31-37: Conv2D + bias
// -> ReLU -> BatchNormalization at inference = per-channel scale and shift), fused into ONE in-place pass over the NHWC activation.
// Left to torch, the epilogue is four full passes over activations of up to 2.1 GB (bias add, relu, multiply, add): 14 % of the
// network's time at 2048^2.  Same float32 operations in the same order (the library is built with -ffp-contract=off, so
// the multiply and the add round separately like torch's two kernels): bit-identical, one read + one write instead of four.
// Runs on the stream the caller names (torch's current stream), so no cross-stream synchronisation is needed.
#include "tip_internal.h"
#include "tip_unet_conv.h"
#include "tip_unet_conv_k32.h"
#include "tip_unet_first.h"
#include "tip_unet_planes.h"
#include <algorithm>
#include <atomic>
#include <type_traits>

namespace tip {

__global__ void __launch_bounds__(256) k_bias_relu_affine_f32(float *__restrict__ x, const float *__restrict__ bias,
                                                              const float *__restrict__ scale, const float *__restrict__ shift,
                                                              long n4, int C)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = reinterpret_cast<float4 *>(x)[i];
    const int c = (int)((i * 4) % C);                       // C % 4 == 0: the four lanes are channels c .. c+3
    const float4 b = *reinterpret_cast<const float4 *>(bias + c);
    const float4 s = *reinterpret_cast<const float4 *>(scale + c);
    const float4 t = *reinterpret_cast<const float4 *>(shift + c);
    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f; v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
    v.x = v.x * s.x + t.x; v.y = v.y * s.y + t.y; v.z = v.z * s.z + t.z; v.w = v.w * s.w + t.w;
    reinterpret_cast<float4 *>(x)[i] = v;
}

// The piece formats of a split tensor: two or three planes of bf16 pieces (format 0) or two planes of fp16 pieces (format 1).
// Returns f(NPL, F16) -- integral constants, the template arguments of the kernels -- or TIP_ERR_ARG for any other pair.
template <typename Fn>
static int with_pieces(int planes, int format, Fn &&f)
{
    if (format == 1 && planes == 2) return f(std::integral_constant<int, 2>{}, std::true_type{});
    if (format == 0 && planes == 2) return f(std::integral_constant<int, 2>{}, std::false_type{});
    if (format == 0 && planes == 3) return f(std::integral_constant<int, 3>{}, std::false_type{});
    return TIP_ERR_ARG;
}
static bool pieces_ok(int planes, int format) { return with_pieces(planes, format, [](auto, auto) { return TIP_OK; }) == TIP_OK; }

// The launch table of the convolutions.  A row: the code tip_unet_conv_flavour returns (include/tissue_hip.h tabulates them), the
// template shape <pieces, tile rows, weight steps ahead, activation chunks ahead, steps per barrier> of k_unet_conv, and what can be
// LAUNCHED for the code -- kernel, threads per workgroup, dynamic LDS bytes -- with bf16 pieces, with fp16 pieces, and with fp16
// pieces on 16x16x32 MFMAs (k_unet_conv_k32 on the shape's tiles in its place: 16-row tiles with the four-step weight schedule, codes
// 2 and 6, and the two-piece 8-row tiles, code 0, which only TIP_UNET_CONV_ROWS8_K32 selects).
// kernel == nullptr: there is none (fp16 pieces come in two planes only).  Threads and LDS bytes are the kernels' own constants
// (UcLayout, UkLaunch): nothing about a launch is computed a second time.
typedef void (*ConvKernel)(const ConvParams);
struct ConvLaunch {
    ConvKernel kernel;
    int threads, lds;
};
enum { CONV_BF16, CONV_F16, CONV_F16_K32, N_CONV_LAUNCHES };
struct ConvFlavour {
    int code, npl, th, d, da, spb;
    ConvLaunch launch[N_CONV_LAUNCHES];
};
constexpr int CONV_LDS_MAX = 160 * 1024;       // a CU's LDS
template <int NPL, int TH, int D, int DA, int SPB, bool F16>
constexpr ConvLaunch conv_launch()
{
    using L = UcLayout<NPL, TH, D, DA, SPB>;
    static_assert(L::LDS <= CONV_LDS_MAX, "the tile buffers fit a CU's LDS");
    return {k_unet_conv<NPL, TH, D, DA, SPB, F16>, L::THREADS, L::LDS};
}
template <typename L>
constexpr ConvLaunch conv_launch_k32()
{
    static_assert(UkLaunch<L>::LDS <= CONV_LDS_MAX, "the tile buffers fit a CU's LDS");
    return {k_unet_conv_k32<L>, UkLaunch<L>::THREADS, UkLaunch<L>::LDS};
}
template <int CODE, int NPL, int TH, int D, int DA = 1, int SPB = 1>
constexpr ConvFlavour conv_flavour()
{
    ConvLaunch f16 = {nullptr, 0, 0}, f16_k32 = {nullptr, 0, 0};
    if constexpr (NPL == 2) f16 = conv_launch<NPL, TH, D, DA, SPB, true>();
    if constexpr (NPL == 2 && TH == 16 && D == 4) f16_k32 = conv_launch_k32<UkTiles16>();
    if constexpr (NPL == 2 && TH == 8) f16_k32 = conv_launch_k32<UkTiles8>();
    return {CODE, NPL, TH, D, DA, SPB, {conv_launch<NPL, TH, D, DA, SPB, false>(), f16, f16_k32}};
}
constexpr ConvFlavour CONV_FLAVOURS[] = {      //                                                     LDS bytes (K = 32: 131 072; code 0: 81 920)
    conv_flavour<0, 2, 8, 2>(),                // 8-row tiles (two workgroups per CU)                    73 728
    conv_flavour<1, 2, 16, 2>(),               // 16-row tiles, three taps                              106 496
    conv_flavour<2, 2, 16, 4>(),               // ... four and more taps, one step per barrier          122 880
    conv_flavour<3, 3, 8, 2>(),                // three pieces                                          110 592
    conv_flavour<4, 2, 16, 2, 2>(),            // ... one and two taps                                  147 456
    conv_flavour<6, 2, 16, 4, 1, 3>(),         // ... 3x3 stencils, three steps per barrier             155 648
};
constexpr int N_CONV_FLAVOURS = sizeof(CONV_FLAVOURS) / sizeof(CONV_FLAVOURS[0]);
static_assert(N_CONV_FLAVOURS * N_CONV_LAUNCHES <= 32, "one bit per table entry in the attribute's once-flag");

}  // namespace tip

using namespace tip;

extern "C" {

// x: n float32 values of a channels-last (NHWC-contiguous) activation with C channels, updated in place:
// x = relu(x + bias[c]) * scale[c] + shift[c].  `stream`: the hipStream_t to launch on, taken as is -- 0 is HIP's null
// stream, which is what torch.cuda.current_stream() is unless the caller changed it.
int tip_bias_relu_affine_f32_dev(float *x, const float *bias, const float *scale, const float *shift, long n, int c, void *stream)
{
    Ctx &cx = ctx();
    if (!cx.stream) return TIP_ERR_HIP;
    if (!x || !bias || !scale || !shift || n < 0 || c < 4 || (c & 3) || (n % c)) return fail(TIP_ERR_ARG, "bias_relu_affine: bad arguments");
    if (n == 0) return TIP_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bias_relu_affine_f32, dim3(cdiv(n / 4, 256)), dim3(256), 0, s, x, bias, scale, shift, n / 4, c);
    return launch_check("bias_relu_affine");
}

// ---- the network's layers on split planes (tip_unet_conv.h, tip_unet_first.h, tip_unet_planes.h).  All of them launch on the stream the caller names
// (torch's current stream: the buffers are torch tensors), like tip_bias_relu_affine_f32_dev. -----------------------------------

// the range word's way to the host: one thread stores it into pinned host memory, in stream order (no copy engine, no second queue)
static __global__ void k_unet_range_fetch(const unsigned *__restrict__ word, int *__restrict__ host) { *host = (int)*word; }

// The calling thread's range word of the fp16-piece kernels (tip_unet_conv.h: uc_range_flag): made on the thread's first U-Net
// launch or range call, zeroed in stream order in front of whatever that call queues on `s`, released with the context.  nullptr
// on failure (error text set).
static unsigned *unet_status_word(Ctx &c, hipStream_t s)
{
    if (c.unet_status) return c.unet_status;
    unsigned *w = nullptr;
    int *h = nullptr;
    hipError_t e = hipMalloc(&w, sizeof(unsigned));
    if (e == hipSuccess) e = hipHostMalloc(&h, sizeof(int), hipHostMallocMapped);
    if (e == hipSuccess) e = hipMemsetAsync(w, 0, sizeof(unsigned), s);
    if (e != hipSuccess) {
        if (w) (void)hipFree(w);
        if (h) (void)hipHostFree(h);
        fail(TIP_ERR_HIP, "the U-Net's range word: %s", hipGetErrorString(e));
        return nullptr;
    }
    c.unet_status = w;
    c.unet_status_host = h;
    return w;
}

// What a descriptor's launch runs, and everything else that follows from the descriptor and the tuning alone.
struct ConvPlan {
    const ConvFlavour *fl;         // the row of CONV_FLAVOURS: code and shape
    ConvLaunch launch;             // ... and the entry of it that is launched
    int entry;                     // the entry's position in the table (the bit of the attribute's once-flag)
    int mfma_k;                    // 16: the flavour's own kernel (32x32x16 MFMAs); 32: k_unet_conv_k32 in its place (16x16x32, tip_unet_conv_k32.h)
    int ntiles, nblks, xcd_map;
};

// Validates the descriptor and chooses the flavour: TIP_OK and `pl`, or the error tip_unet_conv_dev returns.  Touches no device.
// flags: the caller's per-call choices (TIP_UNET_CONV_*, include/tissue_hip.h); 0 is what the entries without flags ask for.
static int unet_conv_plan(const tip_unet_conv_desc *d, int flags, ConvPlan &pl)
{
    if (flags & ~TIP_UNET_CONV_ROWS8_K32) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: unknown flags 0x%x", flags);
    if (!d || !d->in0 || !d->weights || (!d->bias && !d->raw_out) || (!d->out && !d->head_out && !d->raw_out)) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: null pointer");
    if (!pieces_ok(d->planes, d->format)) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: pieces are 2 or 3 planes of bf16 (format 0) or 2 planes of fp16 (format 1)");
    if (d->format == 1 && !(d->acc_scale > 0.f)) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: fp16 pieces come with a positive acc_scale");
    if (d->h < 8 || d->w < UC_TW || d->h % 8 || d->w % UC_TW)
        return fail(TIP_ERR_UNSUPPORTED, "tip_unet_conv_dev: the grid %dx%d is not a multiple of the 8x%d pixel tile", d->h, d->w, UC_TW);
    if (d->c0 < UC_KC || d->c0 % UC_KC || d->c1 < 0 || d->c1 % UC_KC || (d->c1 > 0 && !d->in1) || d->cout < UC_BN || d->cout % UC_BN)
        return fail(TIP_ERR_UNSUPPORTED, "tip_unet_conv_dev: channels (%d + %d -> %d) must be multiples of %d / %d", d->c0, d->c1, d->cout, UC_KC, UC_BN);
    if (d->ntaps < 1 || d->ntaps > 9 || d->sy < 1 || d->sx < 1 || d->oy < 0 || d->ox < 0 ||
        (d->h - 1) * d->sy + d->oy >= d->out_h || (d->w - 1) * d->sx + d->ox >= d->out_w)
        return fail(TIP_ERR_ARG, "tip_unet_conv_dev: bad taps / output mapping");
    if ((d->scale == nullptr) != (d->shift == nullptr)) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: scale and shift come together");
    // a tile's halo window ((tile rows + 2) image rows of one plane) is addressed through 32-bit buffer offsets; tensors may be any size
    if (18L * d->w * (d->c0 > d->c1 ? d->c0 : d->c1) * 2 >= (1L << 32) - 65536)
        return fail(TIP_ERR_UNSUPPORTED, "tip_unet_conv_dev: 18 rows of %d pixels x %d channels exceed the 4 GB a buffer resource addresses",
                    d->w, d->c0 > d->c1 ? d->c0 : d->c1);
    for (int t = 0; t < d->ntaps; ++t)
        if (d->dy[t] < -1 || d->dy[t] > 1 || d->dx[t] < -1 || d->dx[t] > 1) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: tap offsets are -1, 0 or 1");
    if (d->head_out && (!d->head_w || !d->head_b || d->cout != UC_BN || !d->scale || d->pool_out || d->sy != 1 || d->sx != 1 || d->oy != 0 || d->ox != 0 ||
                        d->out_h != d->h || d->out_w != d->w))
        return fail(TIP_ERR_ARG, "tip_unet_conv_dev: the fused head needs a 128-channel Conv2D + BatchNorm layer with the plain output mapping");
    if (d->pool_out && (d->sy != 1 || d->sx != 1 || d->oy != 0 || d->ox != 0 || d->out_h != d->h || d->out_w != d->w))
        return fail(TIP_ERR_ARG, "tip_unet_conv_dev: pool_out needs the plain output mapping");
    if (d->raw_out && (d->head_out || d->pool_out)) return fail(TIP_ERR_ARG, "tip_unet_conv_dev: raw output goes without the head and the pooled map");
    if (d->seed && (d->sy != 1 || d->sx != 1 || d->oy != 0 || d->ox != 0 || d->out_h != d->h || d->out_w != d->w))
        return fail(TIP_ERR_ARG, "tip_unet_conv_dev: the accumulator seed needs the plain output mapping");
    // 16-row tiles (one 512-thread workgroup per CU) where the grid allows: half the weight copies per MFMA, and LDS for five
    // weight buffers (copies four steps ahead) when the stencil has >= 4 taps; two pieces only (LDS)
    const int t8 = tuning().unet_tile8;
    // (measured per layer at 2048^2: the short K loops of the 128-channel 3x3 layers gain 1-3 % from two workgroups per CU -- one's
    // epilogue behind the other's products -- every other layer is faster with the shared weight tile of the 16-row workgroup)
    const bool want8 = t8 == 1 || (t8 < 0 && d->ntaps == 9 && d->c0 + d->c1 <= 128);
    const int th = (d->planes == 2 && d->h % 16 == 0 && !want8) ? 16 : 8;
    const int dist = (th == 16 && d->ntaps >= 4) ? 4 : 2;
    const int da = (th == 16 && d->ntaps <= 2) ? 2 : 1;       // one- and two-tap stencils: activation tiles two chunks ahead
    pl.ntiles = (d->h / th) * (d->w / UC_TW); pl.nblks = d->cout / UC_BN;
    pl.xcd_map = (tuning().unet_xcd_map && pl.nblks > 1 && pl.ntiles % 8 == 0) ? 1 : 0;
    // three steps per barrier: 3x3 stencils on 16-row tiles (a chunk's nine taps in three iterations, nine weight buffers), and the
    // six-tap classes of a composed decoder level (two iterations per chunk) from 256 input channels on -- measured 3.5-6.5 % faster
    // there; shorter six-tap loops were not measured and keep one step per barrier.
    // TIP_UNET_SPB = 1 keeps one step per barrier everywhere, every larger value means three
    const bool three = d->ntaps == 9 || (d->ntaps == 6 && d->c0 + d->c1 >= 256);
    const int spb = (th == 16 && dist == 4 && three && tuning().unet_spb > 1) ? 3 : 1;
    // The MFMA shape is a second property of the launch: the codes below do not change with it.  Two fp16 pieces on 16-row tiles with
    // four and more taps (flavours 2 and 6) run ONE K = 32 kernel, one pair step per barrier, unless TIP_UNET_MFMA=16 -- so
    // TIP_UNET_SPB does not change a bit of what these launches compute.  The 8-row launches with four and more taps (flavour 0) run
    // that kernel on their own tiles only where the CALLER asks for it (TIP_UNET_CONV_ROWS8_K32): K = 32 rounds two steps' sums
    // together, so its bits are not the 32x32x16 kernel's, and what a call without the flag computes does not change.
    const bool k32_tiles = (th == 16 && dist == 4) || (th == 8 && d->ntaps >= 4 && (flags & TIP_UNET_CONV_ROWS8_K32));
    pl.mfma_k = (d->format == 1 && d->planes == 2 && k32_tiles && tuning().unet_mfma == 32) ? 32 : 16;
    const int which = pl.mfma_k == 32 ? CONV_F16_K32 : d->format == 1 ? CONV_F16 : CONV_BF16;
    for (int row = 0; row < N_CONV_FLAVOURS; ++row) {
        const ConvFlavour &f = CONV_FLAVOURS[row];
        if (f.npl != d->planes || f.th != th || f.d != dist || f.da != da || f.spb != spb || !f.launch[which].kernel) continue;
        pl.fl = &f; pl.launch = f.launch[which]; pl.entry = row * N_CONV_LAUNCHES + which;
        return TIP_OK;
    }
    return fail(TIP_ERR_UNSUPPORTED, "tip_unet_conv_dev: no kernel flavour <%d, %d, %d, %d, %d>", d->planes, th, dist, da, spb);
}

int tip_unet_conv_flavour_ex(const tip_unet_conv_desc *d, int flags)
{
    ConvPlan pl;
    const int rc = unet_conv_plan(d, flags, pl);
    return rc ? rc : pl.fl->code;
}
int tip_unet_conv_flavour(const tip_unet_conv_desc *d) { return tip_unet_conv_flavour_ex(d, 0); }

int tip_unet_conv_mfma_k_ex(const tip_unet_conv_desc *d, int flags)
{
    ConvPlan pl;
    const int rc = unet_conv_plan(d, flags, pl);
    return rc ? rc : pl.mfma_k;
}
int tip_unet_conv_mfma_k(const tip_unet_conv_desc *d) { return tip_unet_conv_mfma_k_ex(d, 0); }

int tip_unet_conv_dev(const tip_unet_conv_desc *d, void *stream) { return tip_unet_conv_ex_dev(d, 0, stream); }

int tip_unet_conv_ex_dev(const tip_unet_conv_desc *d, int flags, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    ConvPlan pl;
    if (const int rc = unet_conv_plan(d, flags, pl)) return rc;
    ConvParams p;
    p.in0 = (const uint16_t *)d->in0; p.in1 = (const uint16_t *)(d->c1 > 0 ? d->in1 : d->in0);
    p.c0 = d->c0; p.c1 = d->c1; p.H = d->h; p.W = d->w;
    p.w = (const uint16_t *)d->weights; p.ntaps = d->ntaps;
    for (int t = 0; t < 9; ++t) {
        p.dy[t] = t < d->ntaps ? d->dy[t] : 0; p.dx[t] = t < d->ntaps ? d->dx[t] : 0;
    }
    p.cout = d->cout; p.bias = d->bias; p.scale = d->scale; p.shift = d->shift;
    p.out = (uint16_t *)d->out; p.outH = d->out_h; p.outW = d->out_w; p.sy = d->sy; p.sx = d->sx; p.oy = d->oy; p.ox = d->ox;
    p.pool_out = (uint16_t *)d->pool_out;
    p.acc_scale = d->format == 1 ? d->acc_scale : 1.f;
    p.status = nullptr;
    if (d->format == 1 && !d->raw_out && !(p.status = unet_status_word(c, (hipStream_t)stream))) return TIP_ERR_HIP;
#ifdef UC_TRACE
    static unsigned long long *trace_dev = nullptr;
    if (!trace_dev) { TIP_HIP(hipMalloc(&trace_dev, 1024)); }
    TIP_HIP(hipMemsetAsync(trace_dev, 0, 1024, (hipStream_t)stream));
    p.trace = trace_dev;
#endif
    p.head_w = d->head_w; p.head_b = d->head_b; p.head_out = d->head_out;
    p.raw_out = d->raw_out; p.seed = d->seed;
    p.xcd_map = pl.xcd_map;
    const ConvLaunch &ln = pl.launch;
    const dim3 grid = p.xcd_map ? dim3((unsigned)(pl.ntiles * pl.nblks)) : dim3(pl.ntiles, pl.nblks);
    hipStream_t s = (hipStream_t)stream;
    // the >64 KB dynamic LDS attribute is set once per (device, table entry): one atomic bit each
    static std::atomic<unsigned> attr_done[64];
    const unsigned bit = 1u << pl.entry;
    const int dev = c.device >= 0 && c.device < 64 ? c.device : 0;
    if (!(attr_done[dev].load(std::memory_order_acquire) & bit)) {
        TIP_HIP(hipFuncSetAttribute((const void *)ln.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ln.lds));
        attr_done[dev].fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL(ln.kernel, grid, dim3(ln.threads), (size_t)ln.lds, s, p);
#ifdef UC_TRACE
    {
        unsigned long long tr[128];
        TIP_HIP(hipStreamSynchronize(s));
        TIP_HIP(hipMemcpy(tr, trace_dev, sizeof tr, hipMemcpyDeviceToHost));
        for (int k = 0; k < pl.fl->th / 2; ++k) {
            const unsigned long long *t = tr + 16 * k;
            const double n = (double)t[4];
            fprintf(stderr, "UC_TRACE th %d spb %d taps %d cin %d cout %d grid %dx%d wave %d simd %d: per STEP (shader clocks; sums over the loop / steps): copies %.0f, products %.0f (first MFMA out after %.0f), "
                            "vmcnt wait %.0f, barrier %.0f, total %.0f; steps %.0f; whole loop %.0f, prologue %.0f, epilogue %.0f clocks\n",
                    pl.fl->th, pl.fl->spb, d->ntaps, d->c0 + d->c1, d->cout, d->h, d->w, k, (int)((t[7] >> 4) & 3), t[0] / n, t[2] / n, t[1] / n, t[6] / n, (t[3] - t[6]) / n, t[5] / n, n, (double)t[5], (double)t[8], (double)t[9]);
        }
    }
#endif
    return launch_check("unet_conv");
}

// Border pass of a composed decoder level (tip_unet_planes.h) on the float32 partial of 2h x 2w x cout values: the edge
// bias table on all four edges, then the bottom row's, the right column's and the corner's linear corrections, in stream order.
int tip_unet_compose_border_dev(const void *x, int planes, int format, int h, int w, int cin, int cout, const float *row_w, const float *col_w,
                                const float *corner_w, const float *bias_tab, float *part, float xscale, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!x || !row_w || !col_w || !corner_w || !bias_tab || !part || !pieces_ok(planes, format) ||
        h < 1 || w < 1 || cin < 1 || cout < 128 || cout % 128 || !(xscale > 0.f))
        return fail(TIP_ERR_ARG, "tip_unet_compose_border_dev: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int H2 = 2 * h, W2 = 2 * w;
    const long nb = (2L * W2 + 2L * (H2 - 2)) * (cout / 4);
    hipLaunchKernelGGL(k_unet_compose_edge_bias, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, s, part, H2, W2, cout, bias_tab);
    EdgeParams p;
    p.x = (const uint16_t *)x; p.xplane = (long)h * w * cin; p.planes = planes; p.f16 = format; p.xscale = xscale;
    p.cin = cin; p.cout = cout; p.part = part;
    const long wstride = (long)cin * cout;
    // bottom row: positions run along x on input row h - 1, output row 2h - 1
    p.L = w; p.x0 = (long)(h - 1) * w * cin; p.xstep = cin; p.tapmask = 0x1f;
    for (int t = 0; t < 5; ++t) p.wgt[t] = row_w + t * wstride;
    p.o0 = (long)(H2 - 1) * W2 * cout; p.ostep = cout;
    hipLaunchKernelGGL(k_unet_compose_edge, dim3((unsigned)cdiv(p.L, EB_J), (unsigned)(cout / EB_CO)), dim3(EB_CO * EB_G), 0, s, p);
    // right column: positions run along y on input column w - 1, output column 2w - 1
    p.L = h; p.x0 = (long)(w - 1) * cin; p.xstep = (long)w * cin;
    for (int t = 0; t < 5; ++t) p.wgt[t] = col_w + t * wstride;
    p.o0 = (long)(W2 - 1) * cout; p.ostep = (long)W2 * cout;
    hipLaunchKernelGGL(k_unet_compose_edge, dim3((unsigned)cdiv(p.L, EB_J), (unsigned)(cout / EB_CO)), dim3(EB_CO * EB_G), 0, s, p);
    // corner: the doubly removed term back -- one position, its parity-1 pixel, the tap at offset 0
    p.L = 1; p.x0 = ((long)(h - 1) * w + (w - 1)) * cin; p.xstep = cin; p.tapmask = 0x8;
    for (int t = 0; t < 5; ++t) p.wgt[t] = corner_w;
    p.o0 = ((long)(H2 - 1) * W2 + (W2 - 2)) * cout; p.ostep = cout;
    hipLaunchKernelGGL(k_unet_compose_edge, dim3(1, (unsigned)(cout / EB_CO)), dim3(EB_CO * EB_G), 0, s, p);
    return launch_check("unet_compose_border");
}

int tip_unet_conv_first_dev(const float *in, int h, int w, const float *wgt, const float *bias, const float *scale, const float *shift,
                            void *out, int planes, int format, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !wgt || !bias || !scale || !shift || !out || h < 1 || w < 1 || w % FIRST_RUN || ((long)h * w) % FIRST_PIX || !pieces_ok(planes, format))
        return fail(TIP_ERR_ARG, "tip_unet_conv_first_dev: bad arguments (w must be a multiple of 32, h * w of 256)");
    const dim3 grid((unsigned)((long)h * w / FIRST_PIX));
    hipStream_t s = (hipStream_t)stream;
    unsigned *status = nullptr;
    if (format == 1 && !(status = unet_status_word(c, s))) return TIP_ERR_HIP;
    return with_pieces(planes, format, [&](auto npl, auto f16) {
        hipLaunchKernelGGL((k_unet_conv_first<decltype(npl)::value, decltype(f16)::value>), grid, dim3(256), 0, s, in, h, w, wgt, bias, scale, shift, (uint16_t *)out, status);
        return launch_check("unet_conv_first");
    });
}

// The same layer for the fp16 pieces on the matrix cores (k_unet_conv_first_mfma): packed_weights as every layer's, one tap x 32
// input channels whose rows 0 .. 17 are the 18 (tap, channel) terms.  Which of the two entries a forward pass calls is decided
// in one place, by the caller, from tip_unet_first_mfma().
int tip_unet_conv_first_packed_dev(const float *in, int h, int w, const void *packed_weights, float acc_scale, const float *bias,
                                   const float *scale, const float *shift, void *out, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !packed_weights || !bias || !scale || !shift || !out || h < 1 || w < 1 || w % FIRST_RUN || ((long)h * w) % FIRST_PIX)
        return fail(TIP_ERR_ARG, "tip_unet_conv_first_packed_dev: bad arguments (w must be a multiple of 32, h * w of 256)");
    hipStream_t s = (hipStream_t)stream;
    unsigned *status = unet_status_word(c, s);
    if (!status) return TIP_ERR_HIP;
    // four waves per workgroup, a wave walks the 32-pixel segments wave, wave + waves, ...: TIP_UNET_FIRST > 1 is the number of
    // workgroups per CU (256 CUs) the launch is cut to; the default was chosen by measurement
    const long wgs = (long)h * w / 128;                    // one segment per wave
    const int per_cu = tuning().unet_first_mfma > 1 ? tuning().unet_first_mfma : FIRST_MFMA_WGS_PER_CU;
    const dim3 grid((unsigned)std::min(wgs, 256L * per_cu));
    hipLaunchKernelGGL(k_unet_conv_first_mfma, grid, dim3(256), 0, s, in, h, w, (const uint16_t *)packed_weights, acc_scale, bias, scale, shift,
                       (uint16_t *)out, status);
    return launch_check("unet_conv_first_mfma");
}

int tip_unet_first_mfma(void) { return tuning().unet_first_mfma != 0; }

// The fp16 pieces' range flag (tip_unet_conv.h: uc_range_flag).  reset: the calling thread's word is zeroed in stream order; read:
// the word as it stands behind everything queued on `stream` so far -- the host waits for that stream alone.
int tip_unet_range_reset(void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    const bool fresh = !c.unet_status;
    unsigned *w = unet_status_word(c, (hipStream_t)stream);
    if (!w) return TIP_ERR_HIP;
    if (!fresh) TIP_HIP(hipMemsetAsync(w, 0, sizeof(unsigned), (hipStream_t)stream));
    return TIP_OK;
}

int tip_unet_range_read(void *stream, int *flags)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!flags) return fail(TIP_ERR_ARG, "tip_unet_range_read: null pointer");
    unsigned *w = unet_status_word(c, (hipStream_t)stream);
    if (!w) return TIP_ERR_HIP;
    int *host_dev = nullptr;        // (the pinned word as the device addresses it)
    TIP_HIP(hipHostGetDevicePointer((void **)&host_dev, c.unet_status_host, 0));
    hipLaunchKernelGGL(k_unet_range_fetch, dim3(1), dim3(1), 0, (hipStream_t)stream, (const unsigned *)w, host_dev);
    int rc = launch_check("unet_range_fetch");
    if (rc) return rc;
    TIP_HIP(hipStreamSynchronize((hipStream_t)stream));
    *flags = *(volatile int *)c.unet_status_host;
    return TIP_OK;
}

int tip_unet_pool2_dev(const void *in, int h, int w, int ch, int planes, int format, void *out, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !out || h < 2 || w < 2 || (h & 1) || (w & 1) || ch < 8 || ch % 8 || !pieces_ok(planes, format))
        return fail(TIP_ERR_ARG, "tip_unet_pool2_dev: bad arguments");
    const long n = (long)(h / 2) * (w / 2) * (ch / 8);
    hipStream_t s = (hipStream_t)stream;
    return with_pieces(planes, format, [&](auto npl, auto f16) {
        hipLaunchKernelGGL((k_unet_pool2<decltype(npl)::value, decltype(f16)::value>), dim3(cdiv(n, 256)), dim3(256), 0, s, (const uint16_t *)in, h, w, ch, (uint16_t *)out);
        return launch_check("unet_pool2");
    });
}

int tip_unet_head_dev(const void *in, long npix, const float *wgt, const float *bias, float *out, int planes, int format, int logits, void *stream)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !wgt || !bias || !out || npix < 1 || !pieces_ok(planes, format))
        return fail(TIP_ERR_ARG, "tip_unet_head_dev: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(npix * 8, 256));
    return with_pieces(planes, format, [&](auto npl, auto f16) {
        hipLaunchKernelGGL((k_unet_head<decltype(npl)::value, decltype(f16)::value>), grid, dim3(256), 0, s, (const uint16_t *)in, npix, wgt, bias, out, logits);
        return launch_check("unet_head");
    });
}

}  // extern "C"

