/*
 * tissue_hip.h -- C-ABI of libtissue_hip.so (MI355X / gfx950 hot path).
 *
 * The reference (kasirershahartau/tissue_image_processing) is pure Python and has no
 * native boundary of its own; each entry point below replaces the third-party call
 * the reference makes at the cited line, so that the Python drop-in modules
 * (tissue_image_processing_amd/{basic_image_manipulations,surface_projection,
 * tissue_info,prediction_local}.py) can keep the reference's signatures and bind
 * these symbols through ctypes.
 *
 * Conventions
 *   - plain C types only; row-major contiguous arrays; explicit dims
 *   - return 0 on success, negative tip_status on error; text via tip_last_error()
 *   - `*_dev` variants take DEVICE pointers, run asynchronously on the calling
 *     thread's stream and do not synchronise; the others take HOST pointers,
 *     stage through device workspaces and return after the result is in `out`
 *   - re-entrant: one HIP stream + workspace pool per calling thread
 *   - float arithmetic reproduces scipy.ndimage bit for bit: double accumulation in
 *     scipy's tap order, separately rounded multiply and add (no FMA contraction),
 *     rounding to the array dtype after every axis pass
 */
#ifndef TISSUE_HIP_H
#define TISSUE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIP_API __attribute__((visibility("default")))

typedef enum {
    TIP_OK = 0,
    TIP_ERR_HIP = -1,        /* a HIP runtime call failed */
    TIP_ERR_ARG = -2,        /* bad argument (ValueError in the Python mirror) */
    TIP_ERR_NOMEM = -3,
    TIP_ERR_INDEX = -4,      /* the reference would raise IndexError (sp.py:62,68 clip upper bound) */
    TIP_ERR_UNSUPPORTED = -5,
    TIP_ERR_OVERFLOW = -6,   /* caller-provided capacity too small */
    TIP_ERR_DEGENERATE = -7  /* no convex hull: fewer than three distinct points, or all on one line (ValueError in the mirror) */
} tip_status;

/* ---- lifecycle / plumbing ------------------------------------------------------------------- */
TIP_API int tip_init(int device);                 /* bind the calling thread to `device` (default 0) */
TIP_API int tip_shutdown(void);                   /* free this thread's stream + workspaces */
TIP_API int tip_last_error(char *buf, size_t n);  /* copy this thread's last error text */
TIP_API int tip_device_count(void);
TIP_API int tip_version(void);
TIP_API int tip_malloc(void **dptr, size_t bytes);
TIP_API int tip_free(void *dptr);
TIP_API int tip_memcpy_h2d(void *dst, const void *src, size_t bytes);
TIP_API int tip_memcpy_d2h(void *dst, const void *src, size_t bytes);
TIP_API int tip_memcpy_d2d(void *dst, const void *src, size_t bytes);   /* asynchronous, calling thread's stream */
/* a (height x width_bytes) block between pitched device buffers: the windows of the local-drift map (ti.py:2152-2166) */
TIP_API int tip_memcpy2d_d2d(void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t width_bytes, size_t height);
/* out[c][r] = in[r][c] for a (rows x cols) plane of 4- or 8-byte elements (elem_bytes), DEVICE buffers, asynchronous on   */
/* the calling thread's stream.  Replaces the `.T` a caller applies to SegmentationPredictor.predict's outputs (gui.py:2063: */
/* predict(image (C, Y, X)) returns its int32 labels and float64 HC map as (X, Y), pl.py:102, 194) when it wants them in   */
/* the image's own orientation and they are device tensors.  A bit copy (NaN payloads and -0.0 survive); any extents; not */
/* in place: in == out, a null pointer, an extent < 1 or another element size give TIP_ERR_ARG.                           */
TIP_API int tip_transpose2d_dev(const void *in, void *out, int rows, int cols, int elem_bytes);
TIP_API int tip_memset(void *dst, int value, size_t bytes);
TIP_API int tip_sync(void);                       /* wait for this thread's stream */
/* Tuning and test hooks, process-wide.  The library reads the TIP_* environment variables ONCE (at first use) and   */
/* never again; afterwards a hook changes only through this call.  value NULL or "" restores the default.           */
/*   TIP_WS_TIES = exact | fast          tie policy of the watershed (default exact, see below)                      */
/*   TIP_WS_OPEN = a,b, TIP_WS_NO_SKIP                                                 tile schedule                 */
/*   TIP_WS_DEBUG, TIP_WS_NO_ENDGAME, TIP_WS_NO_WIDE                                   counters / stall machinery    */
/*   TIP_PROJECT_EXACT_SCORE, TIP_PROJECT_GENERIC, TIP_PROJECT_UNFUSED_PREBLUR, TIP_PROJECT_UNFUSED_MASK,            */
/*   TIP_PROJECT_DEBUG                                                                 projection kernel selection   */
/*   TIP_UNET_TILE8 = -1|0|1, TIP_UNET_SPB = 1|3, TIP_UNET_XCD_MAP = 0|1               U-Net convolution schedule    */
/*                                                  (TIP_UNET_SPB: every value above 1 means 3)                       */
/*   TIP_UNET_MFMA = 32|16               K of the MFMA behind fp16 pieces on 16-row tiles with >= 4 taps: 32 (default)  */
/*                                       = v_mfma_f32_16x16x32_f16 on pairs of steps, 16 = 32x32x16 as everywhere else   */
/*   TIP_UNET_TAIL_UNFUSED                                                            tail morphology as separate launches */
/*   TIP_UNET_FIRST = mfma | valu | n    mode f16x3's first layer: matrix cores (default) or the float32 vector kernel; */
/*                                       n > 1: matrix cores with n workgroups per CU (measurements)                    */
/*   TIP_MB_SMALL = pixels, TIP_MB_BATCH = generations                                 two-valued flood: one-workgroup  */
/*                                                                                    generations / host looks         */
/* None of them changes results: they select between schedules / kernels that are tested to agree bit for bit       */
/* (TIP_WS_TIES = fast is the one exception and says so in `flags`).                                                */
/* Quiescent use only: entry points read the table without a lock (aligned ints: never torn, but a call in flight   */
/* while a hook changes may run partly under each value). Set hooks while no other thread is inside the library.    */
TIP_API int tip_set_tuning(const char *name, const char *value);

/* per-kernel timing with HIP events on the library's own stream (bench.py roofline leg) */
TIP_API int tip_prof_enable(int on);
TIP_API int tip_prof_reset(void);
/* writes lines "name count total_ms\n" ; returns number of bytes needed */
TIP_API int tip_prof_report(char *buf, size_t n);

/* ---- separable Gaussian: scipy.ndimage.gaussian_filter(mode='nearest') ---------------------- */
/* replaces bim.py:389 (blur_image), called from sp.py:37,55,70,71 and ti.py:142.                */
/* `taps` are scipy's _gaussian_kernel1d values (length 2*int(4*sigma+0.5)+1, symmetric); an axis */
/* with n==0 is skipped (scipy skips sigma<=1e-15).  dtype: 0=float32, 1=float64.               */
TIP_API int tip_gaussian_taps(double sigma, double truncate, double *taps, int cap); /* libm exp; returns n */
TIP_API int tip_correlate1d_dev(const void *in, void *out, int dtype, int z, int y, int x, int axis,
                                const double *taps_host, int n);
TIP_API int tip_gaussian3d_w(const void *in, void *out, int dtype, int z, int y, int x,
                             const double *tz, int nz, const double *ty, int ny, const double *tx, int nx);
TIP_API int tip_gaussian3d_dev_w(const void *in, void *out, int dtype, int z, int y, int x,
                                 const double *tz, int nz, const double *ty, int ny, const double *tx, int nx);
TIP_API int tip_gaussian3d_f32(const float *in, float *out, int z, int y, int x,
                               double sz, double sy, double sx, double truncate);
TIP_API int tip_gaussian2d_f64(const double *in, double *out, int y, int x, double sy, double sx, double truncate);

/* OR-ed into `method` of tip_project_u16_binned[_dev]: build_manifold=True (sp.py:56-57, 87-165), the z-map grown as a
 * spiral around the score's maximum instead of the per-pixel argmax.  bin_size must be 1; min_z is not added to the
 * z-map (as upstream). */
#define TIP_PROJECT_MANIFOLD 16
/* build_continues_manifold(score) itself (sp.py:87-165): score float32 (z, y, x) -> chosen int64 (y, x); host arrays. */
TIP_API int tip_build_manifold_f32(const float *score, int z, int y, int x, int64_t *chosen);

/* ---- surface projection: sp.py:17-85 (build_manifold=False) ---------------------------------- */
/* czyx: uint16 (C,Z,Y,X).  [zlo,zhi) is the z slice sp.py:30-31 takes when max_z>0 (else 0,Z).   */
/* taps: scipy taps for sigma 0.5 (5), 1 (9), 2 (17), 30 (241); pass NULL to have them built with */
/* libm.  proj: float64 (C,Y,X) (sp.py:74 np.zeros -> float64); zmap: int64 (Y,X) = min_z+argmax. */
/* ref_ch in [-c, 0) counts from the end like numpy's index, and like the reference (sp.py:76      */
/* compares the channel number with it) then gives EVERY channel the atoh_shift-ed mask.           */
TIP_API int tip_project_u16(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z,
                            int ref_ch, int airyscan, int atoh_shift,
                            const double *t05, const double *t1, const double *t2, const double *t30,
                            double *proj, int64_t *zmap);
TIP_API int tip_project_u16_dev(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z,
                                int ref_ch, int airyscan, int atoh_shift,
                                const double *t05, const double *t1, const double *t2, const double *t30,
                                double *proj, int64_t *zmap);
/* diagnostics of the certified-argmax score passes on the fp16 matrix cores (csrc/tip_corr_f16.h; tests): ONE sigma-30 pass  */
/* (241 float64 taps) of a host float32 volume along y (axis 1) or x (axis 2), data bounded by `clip`; flag bit 8: a sample   */
/* beyond that range.  tip_mfma_f16_probe: out[t] = C + sum_k a[t][k] b[t][k] as one v_mfma_f32_32x32x16_f16 computes it -- */
/* where the instruction rounds is what the certified error bound counts.                                                     */
TIP_API int tip_score_pass_f16(const float *in, float *out, int z, int y, int x, int axis, const double *taps, int ntaps, float clip,
                               int *flag);
TIP_API int tip_mfma_f16_probe(const float *a, const float *b, const float *c, float *out, int ncase);
/* sp.py:39-65, bin_size > 1: the score is reduced over bin x bin blocks (skimage block_reduce with */
/* np.mean / np.var, numpy's float32 summation order) and resized back (skimage.transform.resize,   */
/* order 1) before the argmax.  method: 0 'max_averages', 1 'max_std', 2 'multi_channel' (block     */
/* variance of the reference channel x block mean of channel (ref_ch+1)%c).  bin_size 1..128.       */
TIP_API int tip_project_u16_binned(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z,
                                   int ref_ch, int method, int bin_size, int airyscan, int atoh_shift,
                                   const double *t05, const double *t1, const double *t2, const double *t30,
                                   double *proj, int64_t *zmap);
TIP_API int tip_project_u16_binned_dev(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z,
                                       int ref_ch, int method, int bin_size, int airyscan, int atoh_shift,
                                       const double *t05, const double *t1, const double *t2, const double *t30,
                                       double *proj, int64_t *zmap);
/* Spatial tiles of one frame (BASELINE config 5; tiling.py): the 95th percentile of sp.py:33-36 is a property of the */
/* WHOLE reference channel, so tiles first add up 65536-bin histograms of their interiors (tip_hist_u16_box_dev adds   */
/* the box [z0,z1) x [y0,y1) x [x0,x1) of channel ch into hist_dev, uint64 counts of the offset-corrected values), and */
/* every tile (+ halo) is then projected with the frame's histogram instead of its own.                               */
TIP_API int tip_hist_u16_box_dev(const uint16_t *czyx, int c, int z, int y, int x, int ch, int z0, int z1, int y0, int y1,
                                 int x0, int x1, int airyscan, unsigned long long *hist_dev);
TIP_API int tip_project_u16_hist_dev(const uint16_t *czyx, int c, int z, int y, int x, int zlo, int zhi, int min_z,
                                     int ref_ch, int airyscan, int atoh_shift,
                                     const double *t05, const double *t1, const double *t2, const double *t30,
                                     const unsigned long long *hist_dev, double *proj, int64_t *zmap);

/* ---- U-Net convolution epilogue (pl.py:31-37): x = relu(x + bias[c]) * scale[c] + shift[c] in place on a channels-last */
/* float32 activation of n values with c channels (c % 4 == 0), launched on `stream` (a hipStream_t taken as is: NULL is */
/* HIP's null stream, torch's default).  The convolutions themselves run in PyTorch-ROCm / MIOpen.                       */
TIP_API int tip_bias_relu_affine_f32_dev(float *x, const float *bias, const float *scale, const float *shift, long n, int c,
                                         void *stream);
/* Ordering edges between the calling thread's library stream and another HIP stream (torch's current stream); neither */
/* blocks the host.  tip_wait_stream: later library work starts after everything queued on `stream` so far -- call it  */
/* AFTER allocating every torch tensor the library is going to write (the caching allocator hands out blocks whose     */
/* previous owner's kernels may still be queued on that stream).  tip_stream_wait_tip: the other direction.            */
/* >= 0: the device ordinal THIS library's HIP runtime attributes to device pointer p; negative: unknown to it (a     */
/* second copy of libamdhip64 in the process) -- callers that pass torch pointers / streams check this once.          */
TIP_API int tip_pointer_device(const void *p);
TIP_API int tip_wait_stream(void *stream);
TIP_API int tip_stream_wait_tip(void *stream);
/* ---- the U-Net's layers (pl.py:31-72) on the 16-bit matrix cores with split float32 operands ------------------- */
/* Activations between layers are `planes` 16-bit images [plane][y][x][channel] whose sum is the float32 value:       */
/* format 0 = bf16 pieces (planes 2: three products per term, 2^-16; planes 3: six products, float32-equivalent),      */
/* format 1 = fp16 pieces (planes 2) of values SCALED by a power of two: three products per term, float32-equivalent   */
/* to 2^-21 (csrc/tip_unet_conv.h has the arithmetic and its error bound).  Every call launches on `stream` (torch's   */
/* current stream: the buffers are torch tensors) and returns at once.  Tensors may be of any size (a tile's halo      */
/* window, 18 rows of one plane, has to stay below 4 GB).                                                              */
typedef struct tip_unet_conv_desc {
    const void *in0, *in1;      /* split activations; in1 (c1 channels) is appended to in0's channels: concatenate   */
    int c0, c1, h, w, planes;   /* channels (multiples of 16), input grid (multiples of 8 x 32), pieces per value     */
    const void *weights;        /* packed split weights [tap][cin/16][cout/128][plane][128][16] bf16; in every group of 32    */
                                /* output channels row 8g + 4h + j (g < 4, h < 2, j < 4) holds channel 16h + 4g + j            */
    int ntaps, dy[9], dx[9];    /* taps: input offset (-1, 0, 1) each; Conv2D 3x3: the nine offsets in kernel order   */
    int cout;                   /* multiple of 128                                                                     */
    const float *bias, *scale, *shift;   /* scale / shift NULL: bias only (Conv2DTranspose); else bias -> ReLU -> BN */
    void *out;                  /* [plane][out_h][out_w][cout]; input-grid pixel (y, x) -> (y * sy + oy, x * sx + ox)  */
    int out_h, out_w, sy, sx, oy, ox;
    void *pool_out;             /* NULL, or [plane][out_h / 2][out_w / 2][cout]: MaxPool2D(2) of the output, written from  */
                                /* the same registers (Conv2D -> MaxPool2D, pl.py:42-43); needs sy = sx = 1, oy = ox = 0   */
    const float *head_w, *head_b; /* NULL, or the network's head fused into this layer (cout == 128, plain mapping, BN present):  */
    float *head_out;            /* Conv2D(128 -> 2, 1x1) weights [2][128], bias [2], softmax -> float32 (2, h, w); `out` unused    */
    int format;                 /* 0: bf16 pieces; 1: fp16 pieces (planes == 2) -- activations, weights and the constants carry the  */
    float acc_scale;            /* caller's power-of-two scales, and the accumulator is multiplied by acc_scale before the bias      */
    float *raw_out;             /* NULL, or float32 [out_h][out_w][cout]: the launch writes accumulator x acc_scale there through the   */
                                /* output mapping and nothing else (no bias, no split, no saturation; out / bias may be NULL)           */
    const float *seed;          /* NULL, or float32 [h][w][cout] added to the layer's pre-bias sum (plain output mapping): with a       */
                                /* raw launch in front, one layer's sum over two launches                                               */
} tip_unet_conv_desc;
TIP_API int tip_unet_conv_dev(const tip_unet_conv_desc *d, void *stream);
/* Which kernel flavour tip_unet_conv_dev would run for `d` under the current tuning, without launching anything (no device call): */
/* the code below, or the negative error the launch would return (the pointers are only tested against NULL).                     */
/*   code   <pieces, tile rows, weight steps ahead D, activation chunks ahead DA, steps per barrier SPB>   chosen for               */
/*    0     <2,  8, 2, 1, 1>   two pieces; h % 16 != 0, TIP_UNET_TILE8=1, or (default) nine taps with c0 + c1 <= 128                */
/*    1     <2, 16, 2, 1, 1>   two pieces, 16-row tiles, three taps                                                                 */
/*    2     <2, 16, 4, 1, 1>   two pieces, 16-row tiles, four to eight taps (nine with TIP_UNET_SPB=1) except flavour 6's six taps     */
/*    3     <3,  8, 2, 1, 1>   three pieces (bf16 only), always 8-row tiles                                                         */
/*    4     <2, 16, 2, 2, 1>   two pieces, 16-row tiles, one or two taps                                                            */
/*    6     <2, 16, 4, 1, 3>   two pieces, 16-row tiles, nine taps, and six taps with c0 + c1 >= 256                               */
/* Every two-piece flavour exists with bf16 (format 0) and with fp16 pieces (format 1): the code does not depend on the format.   */
/* With fp16 pieces, codes 2 and 6 run one kernel on 16x16x32 MFMAs in place of their own (tip_unet_conv_mfma_k below): a launch  */
/* then computes the same bits whichever of the two codes the tuning gives it.  The codes are the rows of one launch table         */
/* (csrc/tip_unet.hip), which holds per code the kernel, threads and LDS size for bf16 pieces, fp16 pieces and fp16 pieces at      */
/* K = 32; both queries and the launch read the one plan made from it.                                                             */
TIP_API int tip_unet_conv_flavour(const tip_unet_conv_desc *d);
/* The MFMA shape is a second property of a launch and does not change the code: 16 = the flavour's own kernel                     */
/* (v_mfma_f32_32x32x16), 32 = fp16 pieces (format 1) under flavours 2 and 6 run one kernel on v_mfma_f32_16x16x32_f16, K = 32     */
/* formed from two consecutive (chunk, tap) steps, one such pair per barrier (TIP_UNET_MFMA=16 puts them back on 32x32x16).        */
/* Returns 16 or 32, or the negative error the launch would return.                                                                */
TIP_API int tip_unet_conv_mfma_k(const tip_unet_conv_desc *d);
/* The same three entries with the CALLER's per-call choices in `flags` (0: exactly the entries above, which call these with 0; an   */
/* unknown bit: TIP_ERR_ARG).  A choice is the call's own -- stateless, nothing process-wide changes under other threads.           */
/*   TIP_UNET_CONV_ROWS8_K32   fp16 pieces (format 1, two planes) on 8-row tiles with four and more taps run the K = 32 kernel on     */
/*                             their own tiles: 256 threads, two workgroups per CU with 80 KB of LDS each, the workgroup's barrier   */
/*                             between pair steps.  The code stays 0 and tip_unet_conv_mfma_k_ex answers 32 (TIP_UNET_MFMA=16: 16).  */
/*                             K = 32 rounds two steps' sums together: within the mode's per-layer bound of float64 like the          */
/*                             32x32x16 kernel, not bit-identical to it -- which is why it is a flag and not the default.             */
#define TIP_UNET_CONV_ROWS8_K32 1
TIP_API int tip_unet_conv_ex_dev(const tip_unet_conv_desc *d, int flags, void *stream);
TIP_API int tip_unet_conv_flavour_ex(const tip_unet_conv_desc *d, int flags);
TIP_API int tip_unet_conv_mfma_k_ex(const tip_unet_conv_desc *d, int flags);
/* Conv2DTranspose folded into the next Conv2D: border pass on the float32 partial `part` (2h x 2w x cout) that four  */
/* raw launches over the low-resolution tensor x (h x w x cin, split) left.  row_w / col_w: [5][cin][cout] float32 corrections of  */
/* the last output row / column, taps (parity, offset) = (0,-1) (0,0) (1,-1) (1,0) (1,+1); corner_w: [cin][cout]; bias_tab:        */
/* [3][3][cout], (top, inside, bottom) x (left, inside, right); xscale: 1 / the activations' scale (fp16 pieces), else 1.          */
TIP_API int tip_unet_compose_border_dev(const void *x, int planes, int format, int h, int w, int cin, int cout, const float *row_w,
                                        const float *col_w, const float *corner_w, const float *bias_tab, float *part, float xscale,
                                        void *stream);
/* first layer, Conv2D(2 -> 128): float32 (2, h, w) in, weights [9][2][128] float32, exact float32 FMAs               */
TIP_API int tip_unet_conv_first_dev(const float *in, int h, int w, const float *wgt, const float *bias, const float *scale,
                                    const float *shift, void *out, int planes, int format, void *stream);
/* the same layer for the fp16 pieces (format 1, two planes) on the matrix cores: packed_weights as tip_unet_conv_dev takes them  */
/* for ONE tap and 32 input channels, rows k = 2 (3 ky + kx) + channel < 18 the layer's terms and the rest zeros; acc_scale as in */
/* the descriptor; scale / shift carry the activation scale.  The input is scaled by 2^4 and split in the kernel: |x| <= 4094,    */
/* beyond that the range flag below is raised.                                                                                    */
TIP_API int tip_unet_conv_first_packed_dev(const float *in, int h, int w, const void *packed_weights, float acc_scale,
                                           const float *bias, const float *scale, const float *shift, void *out, void *stream);
/* 1: a forward pass in mode f16x3 runs its first layer through tip_unet_conv_first_packed_dev (default); 0: TIP_UNET_FIRST=valu  */
TIP_API int tip_unet_first_mfma(void);
/* The range of the fp16 pieces (format 1): activations are stored as fp16 pieces of scaled values and SATURATE at +-65504 (with  */
/* the network's 2^4 activation scale: |v| = 4094).  Every format-1 launch of tip_unet_conv_dev (not its raw output, which is not */
/* clamped) and of tip_unet_conv_first[_packed]_dev ORs bit 0 (TIP_UNET_RANGE_F16) into a status word of the CALLING THREAD when a value  */
/* on its way into the pieces had !(|x| <= 65504) in front of the clamp: beyond the range, infinite or NaN; exactly +-65504 is in */
/* range.  reset zeroes the thread's word in `stream`'s order; read waits for `stream` (that stream only) and returns the word.  */
#define TIP_UNET_RANGE_F16 1
TIP_API int tip_unet_range_reset(void *stream);
TIP_API int tip_unet_range_read(void *stream, int *flags);
TIP_API int tip_unet_pool2_dev(const void *in, int h, int w, int ch, int planes, int format, void *out, void *stream);   /* MaxPool2D(2) */
/* Conv2D(128 -> 2, 1x1) + softmax: float32 (2, npix) out; logits != 0: the pre-softmax values                         */
TIP_API int tip_unet_head_dev(const void *in, long npix, const float *wgt, const float *bias, float *out, int planes, int format,
                              int logits, void *stream);
/* U1, prepare_image + normalize_channel (pl.py:21-29, 90-122) on a device-resident image: img = (c, a, b) float64,       */
/* element strides (cstride, sa, sb), every channel plane dense in either orientation; kind = dtype of the caller's image  */
/* (0 float64, 1 float32, 2 integer: the clip values take it, pl.py:26-27).  Per channel: np.percentile 1 / 99 (exact order  */
/* statistics by radix select + numpy's lerp), clip, scale; out = (c, bp, ap) float32, transposed, zero-padded in front.      */
TIP_API int tip_unet_prepare_f64_dev(const double *img, int c, int a, int b, long cstride, long sa, long sb, int kind, float *out,
                                     int ap, int bp, void *stream);
/* pl.py:167-194 after the network, one submission: p = class-0 probability map on the device (y rows of x values, row  */
/* pitch ld elements; dtype 0 = float32, 1 = float64) -> 255 (p > thr) -> 5x5 closing -> HC = 7x7 erosion -> boundary = */
/* 5x5 dilation of (closed - HC) -> watershed(watershed_line=True).  labels / hc: caller-owned device buffers (y * x).  */
/* A boundary image that is not two-valued is an error (corrupted intermediate), never a slow flood.                   */
TIP_API int tip_unet_tail_dev(const void *p, int dtype, long ld, int y, int x, double thr, int32_t *labels, double *hc,
                              int32_t *flags_host);

/* ---- overlay images of Tissue.draw_* (ti.py:584-607, 2585-2645): (3, y, x) float64 images the GUI composites over a frame.   */
/* Host arrays in and out.  cell types: positive = all bits of must_mask set (and the byte != 255 unless must_mask is 0) and   */
/* no bit of lack_mask set on a valid byte (is_positive_for_type, ti.py:146-176); negative = valid and not positive.          */
/* tracking: colour cycle18[id % 6], id 0 black (ti.py:2625-2635).  disks: skimage.draw.disk(center, radius, shape), a later    */
/* disc paints over an earlier one (draw_events / draw_cell_tracking / draw_marking_points).  lines: skimage.draw.line          */
/* between (r0, c0, r1, c1) quadruples (draw_neighbors_connections).                                                            */
TIP_API int tip_draw_cell_types_u8(const uint8_t *types, long n, int must_mask, int lack_mask, const double *pos_rgb,
                                   const double *neg_rgb, double *out3);
TIP_API int tip_draw_tracking_i32(const int32_t *track, long n, const double *cycle18, double *out3);
TIP_API int tip_draw_disks_f64(int y, int x, int n, const double *cy, const double *cx, double radius, const double *rgb, double *out3);
TIP_API int tip_draw_lines_f64(int y, int x, int n, const int32_t *ends, const double *rgb, double *out3);

/* ---- rank filters ---------------------------------------------------------------------------- */
/* scipy.ndimage.maximum_filter / minimum_filter (ti.py:1822,2081,2969,4079-4084) and             */
/* skimage.morphology.erosion/dilation with a flat footprint (pl.py:170-193).                     */
/* footprint_kind: 0 = full ky x kx rectangle, 1 = 3x3 cross without centre ([[0,1,0],[1,0,1],[0,1,0]]). */
/* border_mode: 0 = constant 0, 1 = reflect.  is_max: 1 max / 0 min.  Window sides 1..255: up to   */
/* 31 x 31 in one pass over the window, wider rectangles as a row pass and a column pass (a         */
/* rectangular max / min is exactly separable: the same bits).                                     */
TIP_API int tip_rankfilter2d(const void *in, void *out, int dtype /*1=f64, 2=i32*/, int y, int x, int ky, int kx,
                             int footprint_kind, int border_mode, int is_max);
TIP_API int tip_rankfilter2d_dev(const void *in, void *out, int dtype, int y, int x, int ky, int kx,
                                 int footprint_kind, int border_mode, int is_max);
/* bim.py:464-473: thr = imgthresh*max_filter(img, block, reflect) ; out = img < thr ? 0 : img (float64). */
/* block 1..255, an even block acts as block + 1 (the GUI's spin box gives 0..100, taken as 1..101).     */
TIP_API int tip_local_threshold_f64_dev(const double *img, double *out, int y, int x, double imgthresh, int block);

/* ---- connected components: skimage.measure.label(connectivity=1) (ti.py:2922,3470) ----------- */
/* equal-valued 4-neighbours are connected, `bg` pixels -> 0, labels 1..n in raster order of the  */
/* component's first pixel.  Also scipy.ndimage.label on a boolean image (watershed markers).     */
TIP_API int tip_label4_i32(const int32_t *in, int32_t bg, int32_t *out, int y, int x, int32_t *n_labels);
TIP_API int tip_label4_i32_dev(const int32_t *in, int32_t bg, int32_t *out, int y, int x, int32_t *n_labels_host);

/* ---- watershed: skimage.segmentation.watershed(markers=None, connectivity=1) (bim.py:475, pl.py:194) */
/* markers = label(local_minima(img)).  The result equals skimage's bit for bit.  Three routes, reported in `flags`  */
/* (out, may be NULL):                                                                                               */
/*   - landscapes whose non-marker pixels carry distinct values: the data-parallel certified flood (no flag);        */
/*   - two-valued images (pl.py:194): TIP_WS_FLAG_TWO_VALUED, the generation-ranked flood, exact;                    */
/*   - other landscapes with value ties (TIP_WS_FLAG_TIES; the uint16 frames of gui.py:1841-1845): skimage's result */
/*     is a function of its heap array's history, so the flood itself runs as the exact serial (value, age) replay  */
/*     on one host core (TIP_WS_FLAG_SERIAL_EXACT; ~0.3 us per pixel), markers before and everything after on the   */
/*     device.  tip_set_tuning("TIP_WS_TIES", "fast") keeps such images on the device instead: ties are then broken */
/*     by raster index, not by push age, and the labels differ from skimage's in a fraction of the pixels.          */
/* TIP_WS_FLAG_SERIAL_FINISH: the device flood stalled on a serial dependency chain (plateaus larger than any       */
/* certificate; only with the fast tie policy) and the rest was finished on the host; the number of pixels decided  */
/* there is flags >> TIP_WS_FLAG_COUNT_SHIFT (saturating at 2^23 - 1).                                              */
#define TIP_WS_FLAG_TIES 1
#define TIP_WS_FLAG_TWO_VALUED 2
#define TIP_WS_FLAG_SERIAL_EXACT 4
#define TIP_WS_FLAG_SERIAL_FINISH 8
#define TIP_WS_FLAG_COUNT_SHIFT 8
TIP_API int tip_watershed_f64(const double *img, int32_t *labels, int y, int x, int wsl, int32_t *flags);
TIP_API int tip_watershed_f64_dev(const double *img, int32_t *labels, int y, int x, int wsl, int32_t *flags_host);
/* Pop order of m equal-keyed heap entries pushed in raster order when popping entry i is followed  */
/* by c[i] pushes of larger entries (skimage's heap_general.pxi mechanics; the marker phase of      */
/* pl.py:194): e[i] = position of entry i in the pop order.  Host arrays, no device involved.      */
TIP_API int tip_marker_pop_order_host(const uint8_t *c, long m, uint32_t *e);
/* The serial (value, age) flood by itself: host arrays, markers given (> 0 = seed), no device involved.            */
TIP_API int tip_watershed_serial_host(const double *img, const int32_t *markers, int32_t *labels, int y, int x);
/* number of labels (= markers) produced by the calling thread's last watershed call                 */
TIP_API int tip_last_watershed_labels(void);
/* bim.py:446-476 as one device pipeline: local threshold -> Gaussian(sigma) -> watershed.         */
/* block as tip_local_threshold_f64_dev; taps: odd, symmetric, at most 8191 (sigma up to 2047 at   */
/* truncate 4; more than 255 taps travel through device memory like tip_gaussian3d_w's), NULL or   */
/* ntaps 0: no blur.                                                                               */
TIP_API int tip_watershed_segmentation_f64_dev(const double *img, int32_t *labels, int y, int x, double imgthresh,
                                               const double *taps, int ntaps, int block, int32_t *flags_host);

/* ---- cell tables: regionprops_table + find_neighbors (ti.py:880-909,1815-1842) --------------- */
/* SoA outputs over labels 1..n: area, bbox(min_row,min_col,max_row+1,max_col+1), coordinate sums  */
/* (centroid = sum/area), perimeter code counts pc[3*l+{0,1,2}] (weights 1, sqrt2, (1+sqrt2)/2),   */
/* optional intensity sums.                                                                        */
TIP_API int tip_regionprops_i32(const int32_t *labels, const double *intensity /*nullable*/, int y, int x, int n,
                                int64_t *area, int64_t *bbox4, int64_t *sumy, int64_t *sumx, int64_t *pc3,
                                double *isum /*nullable*/);
TIP_API int tip_regionprops_i32_dev(const int32_t *labels, const double *intensity, int y, int x, int n,
                                    int64_t *area, int64_t *bbox4, int64_t *sumy, int64_t *sumx, int64_t *pc3,
                                    double *isum);
/* unique (hi,lo) pairs: a pixel labelled lo>0 whose zero-padded 5x5 maximum is hi != lo           */
TIP_API int tip_neighbor_pairs_i32(const int32_t *labels, int y, int x, int32_t *pairs, int64_t cap, int64_t *n_pairs);
TIP_API int tip_neighbor_pairs_i32_dev(const int32_t *labels, int y, int x, int32_t *pairs_dev, int64_t cap,
                                       int64_t *n_pairs_host);
/* Exact order statistics per label (calc_cell_types' per-cell np.percentile, ti.py:2349-2355) by radix select:       */
/* lo[l] = the value of 0-based rank ranks[l] among the pixels of label l+1 of img (float64), hi[l] = the value of rank */
/* ranks[l]+1 (= lo[l] when the label has no such pixel); ranks[l] < 0 skips label l+1.  labels == NULL: nlab must be 1 */
/* and the statistic is taken over the whole frame (np.percentile(img, 99), ti.py:2371).                               */
TIP_API int tip_label_order_stats_f64(const int32_t *labels, const double *img, int y, int x, int nlab, const int64_t *ranks,
                                      double *lo, double *hi);
/* calc_cell_types (ti.py:2338-2408) of one frame on DEVICE buffers, asynchronous on the calling thread's stream: labels     */
/* (int32) 1..n and the marker plane (float64, same orientation).  Per row l = label - 1 (n rows): out_type = 1 << type_index */
/* when np.percentile(marker[cell], 100 * q_over_100) > threshold * np.percentile(marker, 99) (and, peak_window_size > 0,   */
/* the cell holds a local maximum of the sigma-7 blur under maximum_filter(size=peak_window_size); label 1 never does), else */
/* 0; out_valid = min_cell_area * mean(area) < area < max_cell_area * mean(area) over all n rows; out_mean = intensity mean */
/* (NaN for absent labels).  out_type_map (uint8, y x x): the row's type where valid, 255 elsewhere and on label 0.          */
/* peak_taps: scipy's sigma-7 Gaussian taps (host array, read during the call), used when peak_window_size > 0.             */
TIP_API int tip_cell_types_i32_dev(const int32_t *labels, const double *marker, int y, int x, int n, double q_over_100,
                                   double threshold, int peak_window_size, const double *peak_taps, int n_peak_taps,
                                   int type_index, double min_cell_area, double max_cell_area, uint8_t *out_type,
                                   uint8_t *out_valid, double *out_mean, uint8_t *out_type_map);
/* Contact lengths (ti.py:1844-1872, 4073-4094): for every ordered label pair (hi > lo >= 1) the number of pixels whose  */
/* 4-neighbour maximum of the labels is hi and whose 4-neighbour minimum of the labels with zeros replaced by `big`    */
/* (= max label + 1, ti.py:4081) is lo; filters as scipy's with the cross footprint and mode='constant'.  pairs: (hi, */
/* lo) rows, counts: the pixel numbers, in no particular order.                                                        */
TIP_API int tip_contact_pairs_i32(const int32_t *labels, int y, int x, int big, int32_t *pairs, int64_t *counts, int64_t cap,
                                  int64_t *n_pairs);
/* The same on a DEVICE label map, the triples left in the caller's device buffers (cap rows); the number of triples comes */
/* back to the host, so the call waits for the stream.                                                                  */
TIP_API int tip_contact_pairs_i32_dev(const int32_t *labels, int y, int x, int big, int32_t *pairs_dev, int64_t *counts_dev,
                                      int64_t cap, int64_t *n_pairs_host);

/* ---- neighbour-graph features (ti.py:1752-1791 calculate_n_neighbors_from_type, 2513-2543 find_second_order_neighbors,   */
/* 1065-1096 / 1844-1872 contact lengths) ------------------------------------------------------------------------------- */
/* The graph is a CSR adjacency over the n table rows: offsets int32[n + 1], adj int32[n_adj] of 1-based labels, ASCENDING   */
/* within a row.  Per-row bytes: valid, empty (empty_cell; NULL = no empty row), type.  query: m row indices (0-based), or   */
/* NULL: query q is row q (m <= n).  Every entry has a host form (host arrays, checked before the upload: monotone offsets,  */
/* labels in 1..n ascending in a row, queries below n -- TIP_ERR_ARG otherwise -- returns when the results are in place) and  */
/* a _dev form (device arrays, asynchronous; reads are clamped to n_adj and labels outside 1..n skipped, a query outside     */
/* 0..n-1 gives -1).  n = 0 and m = 0 are valid.                                                                            */
#define TIP_GRAPH_ALL 0
#define TIP_GRAPH_VALID 1
#define TIP_GRAPH_INVALID 2
#define TIP_GRAPH_TYPE 3
/* The CSR that find_neighbors(only_for_labels=...) leaves in the table (ti.py:1815-1842), from the (hi, lo) rows of         */
/* tip_neighbor_pairs_i32[_dev]: a pair gives both directions when working[hi - 1] != 0 or working is NULL (upstream visits   */
/* the working cells and finds a pair from its larger label); a pair with a label outside 1..n takes no part.  adj has room  */
/* for cap entries; *n_adj = the entries needed, and TIP_ERR_OVERFLOW when that exceeds cap (nothing is written to adj then). */
/* _dev: n_adj_host NULL makes the call asynchronous -- rows that would not fit are left out, and cap = 2 n_pairs always fits. */
TIP_API int tip_neighbor_csr_i32(const int32_t *pairs, int64_t n_pairs, int64_t n, const uint8_t *working, int32_t *offsets,
                                 int32_t *adj, int64_t cap, int64_t *n_adj);
TIP_API int tip_neighbor_csr_i32_dev(const int32_t *pairs, int64_t n_pairs, int64_t n, const uint8_t *working, int32_t *offsets,
                                     int32_t *adj, int64_t cap, int64_t *n_adj_host);
/* out[q]: mode ALL the row's degree (ti.py:1782-1783); VALID / INVALID its neighbours with valid == 1 / == 0 and empty == 0  */
/* (ti.py:1784-1789); TYPE those with valid == 1, empty == 0 that are positive for type bit sel_bit (is_positive_for_type:    */
/* bit set and byte != 255) when sel_positive != 0, or not positive (255 included) otherwise (ti.py:1771-1781).              */
TIP_API int tip_graph_counts_i32(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid,
                                 const uint8_t *empty, const uint8_t *type, const int32_t *query, int64_t m, int mode, int sel_bit,
                                 int sel_positive, int64_t *out);
TIP_API int tip_graph_counts_i32_dev(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid,
                                     const uint8_t *empty, const uint8_t *type, const int32_t *query, int64_t m, int mode,
                                     int sel_bit, int sel_positive, int64_t *out);
/* find_second_order_neighbors: for query row i the set of k in N(j), j in N(i) with valid[j] == 1, that have valid[k] == 1,  */
/* pass the selector (sel_bit -1: all; else type bit and polarity as above, without the empty test) and are not i itself;    */
/* first neighbours stay in (upstream drops the result of its .difference, ti.py:2539).  sizes[q] = the set's size.  With      */
/* members != NULL the labels of set q are written from members[member_offsets[q]] on (the caller's exclusive scan of the     */
/* sizes; members_cap entries in all), in order of first discovery (j ascending, then k ascending).                           */
TIP_API int tip_graph_second_i32(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid,
                                 const uint8_t *type, const int32_t *query, int64_t m, int sel_bit, int sel_positive, int64_t *sizes,
                                 const int64_t *member_offsets, int32_t *members, int64_t members_cap);
TIP_API int tip_graph_second_i32_dev(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid,
                                     const uint8_t *type, const int32_t *query, int64_t m, int sel_bit, int sel_positive,
                                     int64_t *sizes, const int64_t *member_offsets, int32_t *members, int64_t members_cap);
/* Contact lengths per row from the (hi, lo, pixels) triples of tip_contact_pairs_i32[_dev]: an edge of the CSR weighs its     */
/* triple's pixels (0 without one; a triple that is no edge is ignored), sums[q] = the weights of row q's selected neighbours */
/* and n_sel[q] their number -- mode ALL every neighbour, VALID valid == 1, TYPE the type selector alone (ti.py:1857-1866: no  */
/* validity test there, unlike the counts).  With values != NULL the selected neighbours' weights (and labels, value_labels)  */
/* are written from value_offsets[q] on, ascending by label (the caller's exclusive scan of n_sel; values_cap entries).        */
TIP_API int tip_contact_sums_i32(const int32_t *pairs, const int64_t *counts, int64_t n_triples, const int32_t *offsets,
                                 const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid, const uint8_t *type,
                                 const int32_t *query, int64_t m, int mode, int sel_bit, int sel_positive, int64_t *sums,
                                 int64_t *n_sel, const int64_t *value_offsets, int64_t *values, int32_t *value_labels,
                                 int64_t values_cap);
TIP_API int tip_contact_sums_i32_dev(const int32_t *pairs, const int64_t *counts, int64_t n_triples, const int32_t *offsets,
                                     const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *valid, const uint8_t *type,
                                     const int32_t *query, int64_t m, int mode, int sel_bit, int sel_positive, int64_t *sums,
                                     int64_t *n_sel, const int64_t *value_offsets, int64_t *values, int32_t *value_labels,
                                     int64_t values_cap);
/* ---- hexatic order and neighbour correlations (ti.py:2545-2583, 803-843; csrc/tip_order.hip) -------------------------------- */
/* The Delaunay neighbours of n planar points (py, px float64), what scipy.spatial.Voronoi(...).ridge_points pairs up in             */
/* find_nearest_neighbors_using_voroni_tesselation.  Rule: (i, j) is an edge iff the interval of circle centres m + t d (m the      */
/* midpoint, d the perpendicular of p_j - p_i) that no third point enters is non-empty, lo < hi STRICTLY (cocircular quadruples     */
/* keep neither diagonal), and no collinear point lies strictly between the two; float64, explicitly rounded operations on           */
/* coordinates relative to p_i.  Two calls, as tip_graph_second_i32: sizes[i] (int64[n], the degree) with members    */
/* NULL; then, after the caller's exclusive scan of the sizes into member_offsets (int64[n]), members (int32, capacity members_cap)  */
/* = the neighbours' 0-based point positions, ascending within a row.  No degree cap.  n < 2: empty rows.  All points collinear:     */
/* the chain of consecutive points (Qhull raises there).  The host form rejects a non-finite coordinate (TIP_ERR_ARG); in the _dev  */
/* form such a point takes no part and has an empty row.  Coincident points are the caller's to exclude: their rows are             */
/* unspecified (Qhull drops the later twin), though every access stays inside the arrays.                                          */
TIP_API int tip_delaunay_neighbors_f64(const double *py, const double *px, int64_t n, int64_t *sizes, const int64_t *member_offsets,
                                       int32_t *members, int64_t members_cap);
TIP_API int tip_delaunay_neighbors_f64_dev(const double *py, const double *px, int64_t n, int64_t *sizes,
                                           const int64_t *member_offsets, int32_t *members, int64_t members_cap);
/* Tissue.calc_psin (ti.py:2563-2583): per query row q (table row query[q]; query NULL: row q) psi_n over its members               */
/* members[member_offsets[q] .. member_offsets[q + 1]) -- 1-BASED labels looked up in the whole table's cy, cx (n rows) --:          */
/* hypot(sum cos(n theta), sum sin(n theta)) / count, theta = atan2(cy[k] - cy[r], cx[k] - cx[r]), summed in the order given         */
/* (ascending labels from the wrappers); 0 for an empty row.  order in 1..64.  member_offsets has m + 1 entries.                     */
TIP_API int tip_psin_f64(const double *cy, const double *cx, int64_t n, const int32_t *query, int64_t m, const int64_t *member_offsets,
                         const int32_t *members, int64_t n_members, int order, double *out);
TIP_API int tip_psin_f64_dev(const double *cy, const double *cx, int64_t n, const int32_t *query, int64_t m,
                             const int64_t *member_offsets, const int32_t *members, int64_t n_members, int order, double *out);
/* The row loops of calculate_neighbors_correlation_function (ti.py:816-838) on the CSR above: per query row q, over its neighbours  */
/* j with member[j - 1] != 0 (upstream's `neighbor_index - 1 in valid_cells.index`), nb_sum[q] = the sum of state[j - 1] in row      */
/* order (float64 additions) and nb_cnt[q] = their number.  member: uint8[n], state: float64[n].                                   */
TIP_API int tip_graph_neighbor_state_f64(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj, const uint8_t *member,
                                         const double *state, const int32_t *query, int64_t m, double *nb_sum, int64_t *nb_cnt);
TIP_API int tip_graph_neighbor_state_f64_dev(const int32_t *offsets, const int32_t *adj, int64_t n, int64_t n_adj,
                                             const uint8_t *member, const double *state, const int32_t *query, int64_t m,
                                             double *nb_sum, int64_t *nb_cnt);
/* The two above chained on DEVICE arrays for the movie driver (FramePipeline.order_features): degree[i] = the number of Delaunay    */
/* neighbours of point i and psi[i] = psi_order over them; sizes, scan, members and psi stay on the device.  Waits for the stream   */
/* once, to size the member list (4 bytes come back); psi and degree are then written asynchronously, like every _dev entry.        */
TIP_API int tip_order_features_f64_dev(const double *py, const double *px, int64_t n, int order, double *psi, int64_t *degree);
/* Tissue.update_labels (ti.py:2967-2970): negatives take the zero-padded 3x3 maximum              */
TIP_API int tip_update_labels_i32(int32_t *labels, int y, int x);
/* track_cells_iterator's label lookup (ti.py:2081-2090): maximum_filter(labels,(3,3),'constant') sampled at query   */
/* points (host arrays); out[i] = -1 for points outside the frame. labels is a DEVICE pointer.                     */
TIP_API int tip_lookup_max3_i32_dev(const int32_t *labels, int y, int x, const int64_t *qy_host, const int64_t *qx_host,
                                    int64_t n, int32_t *out_host);
/* Tissue.get_trackking_labels (ti.py:4021-4028): out[p] = lut[labels[p]] (lut[0] = 0)              */
TIP_API int tip_lut_gather_i32(const int32_t *labels, const int64_t *lut, int64_t n_lut, int64_t *out, int64_t n);

/* ---- event detection of one frame pair (ti.py:609-789: detect_edge_cells, find_events_iterator; csrc/tip_events.hip) --------- */
/* detect_edge_cells as row flags: flags[r] = 1 when label r + 1 occurs in the first or last row or column of the (y, x) map, 0      */
/* otherwise (uint8[n]; a label above n takes no part).  Only the 2 (y + x) border pixels are read.                                 */
TIP_API int tip_border_rows_i32(const int32_t *labels, int y, int x, int64_t n, uint8_t *flags);
TIP_API int tip_border_rows_i32_dev(const int32_t *labels, int y, int x, int64_t n, uint8_t *flags);
/* The exact-pixel sibling of tip_lookup_max3_i32_dev: out[i] = labels[qy[i], qx[i]], -1 for points outside the frame (the events  */
/* code reads the raw previous map, ti.py:745-760).  labels is a DEVICE pointer, the queries and out are host arrays.              */
TIP_API int tip_lookup_i32_dev(const int32_t *labels, int y, int x, const int64_t *qy_host, const int64_t *qx_host, int64_t n,
                               int32_t *out_host);
/* find_events_iterator's three tests for one frame pair, over ROWS.  Per frame: id (the track label of each row), sel (valid == 1  */
/* and empty_cell == 0), pos (positive for the differentiation type; read on sel rows only) and the neighbour sets as a CSR (offsets */
/* int32[n + 1], adj int32[n_adj]; tip_neighbor_csr_i32's layout).  For the current frame also edge (tip_border_rows_i32 of its map)  */
/* and under (the PREVIOUS map's label under the row's drift-shifted centroid, -1 outside the frame); first_edge_ids: the ids of the  */
/* movie's FIRST frame's border rows.  P / C = the ids of the previous / current frame's sel rows; ids are unique among a frame's    */
/* sel rows (the caller's to ensure; INT64_MIN is reserved).  A neighbour label n is used as a ROW INDEX, without a minus one, as     */
/* upstream does: the row test is 0 <= n < rows and sel[n], and the neighbour's id is then id[n].                                    */
/*   delam[r]    previous row r: id in P \ C and not in first_edge_ids, and every neighbour passes the row test with an id that is   */
/*               neither in P \ C nor in first_edge_ids (an empty row passes).                                                        */
/*   diff[r]     previous row r: id in P and C, positive in the current frame and not in the previous one, same neighbourhood test.  */
/*   division[r] current row r: id in C \ P and no id of an edge row, under[r] != -1, every neighbour passes the row test in the       */
/*               current frame, and at least one matches: its id in P and C and no edge id, under[n] != -1 and under[n] == under[r]  */
/*               (label 0, a watershed line under both, compares equal).  n_match[r] = the matches, mother_row[r] = the matching      */
/*               row with the largest index; 0 and -1 on rows without a division.                                                     */
TIP_API int tip_event_flags_i32(const int64_t *id_prev, const uint8_t *sel_prev, const uint8_t *pos_prev, const int32_t *off_prev,
                                const int32_t *adj_prev, int64_t n_prev, int64_t n_adj_prev, const int64_t *id_cur,
                                const uint8_t *sel_cur, const uint8_t *pos_cur, const int32_t *off_cur, const int32_t *adj_cur,
                                int64_t n_cur, int64_t n_adj_cur, const uint8_t *edge_cur, const int32_t *under_cur,
                                const int64_t *first_edge_ids, int64_t n_first_edge, uint8_t *delam, uint8_t *diff, uint8_t *division,
                                int32_t *n_match, int32_t *mother_row);
TIP_API int tip_event_flags_i32_dev(const int64_t *id_prev, const uint8_t *sel_prev, const uint8_t *pos_prev, const int32_t *off_prev,
                                    const int32_t *adj_prev, int64_t n_prev, int64_t n_adj_prev, const int64_t *id_cur,
                                    const uint8_t *sel_cur, const uint8_t *pos_cur, const int32_t *off_cur, const int32_t *adj_cur,
                                    int64_t n_cur, int64_t n_adj_cur, const uint8_t *edge_cur, const int32_t *under_cur,
                                    const int64_t *first_edge_ids, int64_t n_first_edge, uint8_t *delam, uint8_t *diff,
                                    uint8_t *division, int32_t *n_match, int32_t *mother_row);

/* ---- window statistics and spatial feature maps (ti.py:1200-1266: calculate_spatial_data, the windows of get_frame_data) ---- */
/* For each of m centres (qy, qx) and a table of n rows (cy, cx float64, area int64, type uint8, feat float64 or NULL = zeros):   */
/* n_in = rows with (cx - qx)^2 + (cy - qy)^2 < r2 -- two subtractions, two squarings, one addition, each rounded to float64, a  */
/* strict <, as numpy evaluates upstream's query (ti.py:1266); area_in = the exact sum of their areas; n_sel = those that also   */
/* pass the type selector; sum_sel = the sum of feat over the selected ones, in table order.  Selector: sel_bit -1 = every row, */
/* else is_positive_for_type(type, sel_bit) (bit set and type != 255, ti.py:146-176) when sel_positive != 0 and its negation    */
/* otherwise.  r2 = +inf takes every row with finite coordinates.  m = 0 and n = 0 are valid.  The caller applies upstream's   */
/* "%f" rounding of the centres and of r2 (ti.py:1266) before the call.                                                         */
TIP_API int tip_window_stats_f64(const double *qy, const double *qx, int64_t m, double r2, const double *cy, const double *cx,
                                 const int64_t *area, const uint8_t *type, const double *feat, int64_t n, int sel_bit,
                                 int sel_positive, int64_t *n_in, int64_t *area_in, int64_t *n_sel, double *sum_sel);
TIP_API int tip_window_stats_f64_dev(const double *qy, const double *qx, int64_t m, double r2, const double *cy, const double *cx,
                                     const int64_t *area, const uint8_t *type, const double *feat, int64_t n, int sel_bit,
                                     int sel_positive, int64_t *n_in, int64_t *area_in, int64_t *n_sel, double *sum_sel);
/* Tissue.calculate_spatial_data (ti.py:1239-1258): the statistics above at the grid points (s/2 + i s, s/2 + j s) below (y, x),  */
/* s = step; per point the value of `mode` -- 0 density: n_sel / area_in (0 when n_sel == 0 or area_in <= 0), 1 type fraction:  */
/* n_sel / n_in (0 when n_sel == 0), 2 mean: sum_sel / n_sel (NaN when n_sel == 0) -- and the (y, x) float64 map: zero, with the */
/* block [py - s/2, py + s/2) x [px - s/2, px + s/2) of each point set to its value (an odd s leaves one-pixel seams, s = 1 an  */
/* empty map, the frame clips the last block: upstream's slices).  n_sel_grid: NULL, or ceil((y - s/2) / s) x ceil((x - s/2) /  */
/* s) counts, row-major -- a mean-mode caller finds there the windows that selected no cell.  The _dev form takes device       */
/* pointers and leaves map (and n_sel_grid) in the caller's device buffers.                                                    */
TIP_API int tip_spatial_map_f64(int y, int x, int step, double r2, const double *cy, const double *cx, const int64_t *area,
                                const uint8_t *type, const double *feat, int64_t n, int sel_bit, int sel_positive, int mode,
                                double *map, int64_t *n_sel_grid);
TIP_API int tip_spatial_map_f64_dev(int y, int x, int step, double r2, const double *cy, const double *cx, const int64_t *area,
                                    const uint8_t *type, const double *feat, int64_t n, int sel_bit, int sel_positive, int mode,
                                    double *map, int64_t *n_sel_grid);

/* ---- drift: skimage.registration.phase_cross_correlation(ref, mov, upsample_factor) ---------------------------- */
/* (ti.py:1976-1977, 2029-2030 update_drift / calculate_refine_drift; bim.py:522-536 calculate_drift).               */
/* dtype: 0 float32, 1 float64, 3 uint16; extents in [2, 4096] (powers of two: radix-2 FFT rows; anything else: Bluestein).  out4 = whole-pixel peak (row, col) of       */
/* |ifft2(F1 conj F2)| and the peak (row, col) on the ceil(1.5*upsample)^2 upsampled grid; the caller forms the shift  */
/* exactly as skimage does (wrap past the midpoint, round to the grid, add (fine - floor(region/2)) / upsample).       */
/* Both are the windowed correlation below with ONE window of the frame's extent at the origin: one body, one stream wait. */
TIP_API int tip_phase_correlation(const void *ref, const void *mov, int dtype, int y, int x, int upsample, int64_t *out4);
TIP_API int tip_phase_correlation_dev(const void *ref, const void *mov, int dtype, int y, int x, int upsample,
                                      int64_t *out4_host);
/* The correlation on n windows of one DEVICE frame pair at once (the local-drift map, ti.py:2149-2173): ref and mov are  */
/* (frame_y, frame_x) planes of `dtype`; window w is the ny x nx block at (origins[4w], origins[4w+1]) of ref and at             */
/* (origins[4w+2], origins[4w+3]) of mov (origins: HOST int32, n x 4).  out4n_host (n x 4) receives per window exactly the four */
/* integers tip_phase_correlation_dev returns on the two cropped windows: a window's result does not depend on the windows      */
/* beside it -- one crop-and-convert kernel that reads the frames through their pitch, one plan per extent, the rows of all      */
/* windows of a chunk in one row launch, the window as a grid dimension everywhere else, each window's upsampled-DFT offsets     */
/* taken from its coarse peak on the device.  Windows go through in chunks of max_batch (0: as many as fit a fixed 2 GiB      */
/* workspace budget), one stream wait per chunk; results do not depend on the chunking.  ny, nx outside [2, 4096]:               */
/* TIP_ERR_UNSUPPORTED; a window that leaves its frame, a null pointer, n < 0, max_batch < 0, another dtype: TIP_ERR_ARG;        */
/* n == 0: TIP_OK, nothing is touched.                                                                                          */
TIP_API int tip_phase_correlation_windows_dev(const void *ref, const void *mov, int dtype, int frame_y, int frame_x, int n,
                                              const int32_t *origins, int ny, int nx, int upsample, int max_batch,
                                              int64_t *out4n_host);
/* diagnostics (tests): the 2-D transform tip_phase_correlation runs, by itself.  in / out: host complex128 (y, x),    */
/* interleaved re, im; inverse != 0: conjugate twiddles, no scaling (= y * x * ifft2).  Extents as tip_phase_correlation. */
TIP_API int tip_fft2_c128(const double *in, double *out, int y, int x, int inverse);

/* ---- PIV drift: skimage.registration.optical_flow_tvl1(ref, mov, attachment, tightness, num_warp, num_iter, tol) --- */
/* (ti.py:2061-2070 track_cells_iterator(use_piv=True)); scikit-image 0.18.3, 2-D, float32, prefilter=False.           */
/* dtype: 0 float32, 1 float64, 3 uint16, 4 uint8 (integers scaled to [0, 1] like skimage's _convert); y, x >= 2.       */
/* flow_out: (2, y, x) float32, row displacement then column displacement.  warps_per_level: the warps each pyramid    */
/* level ran, coarse to fine (skimage's early stop), `cap` entries (at most 10 levels).  The _dev variant takes device */
/* ref / mov / flow_out; warps_per_level stays a host array there, and when it is not NULL the call waits for the      */
/* stream (without it the call is asynchronous like every _dev entry).                                                */
TIP_API int tip_optical_flow_tvl1(const void *ref, const void *mov, int dtype, int y, int x, float attachment, float tightness,
                                  int num_warp, int num_iter, double tol, float *flow_out, int32_t *warps_per_level, int cap);
TIP_API int tip_optical_flow_tvl1_dev(const void *ref, const void *mov, int dtype, int y, int x, float attachment,
                                      float tightness, int num_warp, int num_iter, double tol, float *flow_out,
                                      int32_t *warps_per_level, int cap);
/* The PIV step of the sharded movie tracker (movie.process_movie(use_piv=True); ti.py:2061-2106, frame t against t-1):  */
/* the flow above from prev_plane to cur_plane -- DEVICE (y, x) float64 reference-channel projections, each truncated to  */
/* uint16 first (astype, as the GUI loads the movie) and then scaled like dtype 3 -- sampled at the n rows of frame t-1's  */
/* table with upstream's transposed indexing: rows = round(cx), cols = round(cy) (half to even; an index in [-size, 0)    */
/* wraps), cx -= flow_row[rows, cols], cy -= flow_col[rows, cols] in float64; then hit_host[i] = maximum_filter(labels,    */
/* (3,3), 'constant') at (round(cy), round(cx)), -1 outside the frame or where present_host[i] == 0.  labels is a DEVICE */
/* int32 map; cy/cx/present/hit are host arrays.  An index that numpy would reject gives TIP_ERR_INDEX with numpy's text */
/* ("index I is out of bounds for axis A with size S", the first failing row, axis 0 before axis 1).  The flow stays in  */
/* the workspace unless flow_dev (device, (2, y, x) float32) is given; with n == 0 and no flow_dev nothing is computed.  */
/* Waits for the stream when n > 0.                                                                                      */
TIP_API int tip_piv_lookup_max3_i32_dev(const double *prev_plane, const double *cur_plane, const int32_t *labels, int y, int x,
                                        const double *cy_host, const double *cx_host, const uint8_t *present_host, int64_t n,
                                        float attachment, float tightness, int num_warp, int num_iter, double tol,
                                        float *flow_dev, int32_t *hit_host);
/* Its sampling-and-lookup step alone on a given DEVICE (2, y, x) float32 flow (same rules, same errors; waits).          */
TIP_API int tip_piv_sample_max3_i32_dev(const float *flow, const int32_t *labels, int y, int x, const double *cy_host,
                                        const double *cx_host, const uint8_t *present_host, int64_t n, int32_t *hit_host);

/* ---- track linking: trackpy.link_df_iter's model for one frame (csrc/tip_link.hip; ti.py:1881-1938) ---------------------- */
/* linking.link_candidates + _solve_subnet on the device.  track_pos (n_tracks, 3) and points (n, 3): row-major embedded      */
/* features (cy, cx, sqrt(area / 2)), linking.embed.  A candidate link joins a track and a feature with                       */
/* d = sqrt(dy dy + dx dx + da da) <= search_range (each operation rounded, left to right).  Tracks and features connected     */
/* through live links form a subnet; one with at most max_subnet tracks and features is solved -- the links minimising          */
/* sum(d^2) + range^2 per unlinked track and per unlinked feature, range = the current one -- and its links die; while         */
/* larger ones remain, range *= adaptive_step (in double, repeatedly) and links longer than that die.  track_of_feature[j]:    */
/* the track feature j continues, -1 when it starts a new one.  stats (6 entries, may be NULL): candidate links, rounds,        */
/* subnets solved, the largest solved subnet's larger side, the last range as the BIT PATTERN of the double, oversize flag:     */
/* 0 none; 1: a subnet exceeds max_subnet and adaptive_stop < 0 (no adaptive search); 2: the range fell below adaptive_stop   */
/* (or reached 0) with a subnet still too large.  With the flag set the call still returns TIP_OK and track_of_feature is      */
/* unspecified.  TIP_ERR_ARG: a null pointer, a negative count, more than 2^31 - 24 tracks + features, search_range <= 0 or    */
/* not finite, adaptive_step outside (0, 1), adaptive_stop NaN, and in the host form a non-finite coordinate (the device form   */
/* leaves such a row unlinked); TIP_ERR_UNSUPPORTED: max_subnet outside [1, 30] (the LDS budget of the solver);                */
/* TIP_ERR_OVERFLOW: more than 2^31 - 1 candidate links.  n == 0 or n_tracks == 0: TIP_OK, all -1, nothing is read.  The _dev   */
/* form takes device pointers (stats too) and, unlike most _dev entries, waits for the stream: once for the link count and      */
/* once per round.                                                                                                              */
TIP_API int tip_link_frame_f64(const double *track_pos, int64_t n_tracks, const double *points, int64_t n, double search_range,
                               double adaptive_stop, double adaptive_step, int max_subnet, int32_t *track_of_feature,
                               int64_t *stats);
TIP_API int tip_link_frame_f64_dev(const double *track_pos, int64_t n_tracks, const double *points, int64_t n,
                                   double search_range, double adaptive_stop, double adaptive_step, int max_subnet,
                                   int32_t *track_of_feature, int64_t *stats);

/* ---- deflate of a map: runs, or runs and row matches (csrc/tip_deflate.hip; movie.save_seg's label and type maps) -------- */
/* The most bytes the encoder below writes for nbytes of input -- the one place the bound is written: per chunk of 65536     */
/* input bytes 3 + 9 n + 7 + 3 bits (headers, the longest literal for every byte, end of block), padded to a byte, + 4.      */
/* Touches no device.                                                                                                         */
TIP_API int tip_deflate_runs_bound(int64_t nbytes, int64_t *bound_out);
/* A raw deflate stream (RFC 1951) of the nbytes at src_dev into dst_dev (DEVICE buffers; cap: dst's bytes, at least the      */
/* bound) and the CRC-32 (zip / zlib) of the input; size and CRC arrive in host words after ONE wait for the stream.  The     */
/* stream is a sequence of byte-aligned NON-final blocks: per chunk of 65536 input bytes one fixed-Huffman block of literals  */
/* and matches of distance elem_bytes (1, 2 or 4; no match reaches before its chunk) and one empty stored block, so the caller*/
/* may put a stored block in front and must put a final block behind (01 00 00 FF FF).  The token rule: tip_deflate.hip's     */
/* head, restated in tests/deflate_restate.py.  TIP_ERR_ARG: a null pointer, another elem_bytes, nbytes not a multiple of it, */
/* cap below the bound.  nbytes == 0 gives the empty stream and CRC 0.                                                        */
TIP_API int tip_deflate_runs_dev(const void *src_dev, int64_t nbytes, int elem_bytes, void *dst_dev, int64_t cap,
                                 int64_t *out_bytes_host, uint32_t *crc32_host);
/* The same on host arrays, staged through the calling thread's workspaces.                                                   */
TIP_API int tip_deflate_runs(const void *src, int64_t nbytes, int elem_bytes, void *dst, int64_t cap, int64_t *out_bytes,
                             uint32_t *crc32);
/* The same stream framing, contracts and bound (tip_deflate_runs_bound) with matches to the ROW ABOVE beside the runs: the    */
/* buffer is a map whose rows are row_bytes long (a positive multiple of elem_bytes; it need not divide nbytes), and an element */
/* may also match the one row_bytes, row_bytes + elem_bytes or row_bytes - elem_bytes before it in the buffer -- each distance */
/* used when it is above elem_bytes and at most 32768; such a match is at least 4 bytes long, may reach into an earlier chunk  */
/* and never before the buffer.  The rule: tip_deflate.hip's head, restated in tests/deflate_rows_restate.py.  With no usable  */
/* distance (row_bytes > 32768 + elem_bytes) the stream is tip_deflate_runs'.  TIP_ERR_ARG additionally: row_bytes <= 0 or not */
/* a multiple of elem_bytes.                                                                                                    */
TIP_API int tip_deflate_rows_dev(const void *src_dev, int64_t nbytes, int elem_bytes, int64_t row_bytes, void *dst_dev, int64_t cap,
                                 int64_t *out_bytes_host, uint32_t *crc32_host);
TIP_API int tip_deflate_rows(const void *src, int64_t nbytes, int elem_bytes, int64_t row_bytes, void *dst, int64_t cap,
                             int64_t *out_bytes, uint32_t *crc32);
/* The same tokens, framing, contracts, error codes and bound with DYNAMIC Huffman codes: per chunk the tokens become either the */
/* fixed-Huffman block of the entries above or one dynamic-Huffman block with the chunk's own literal/length and distance codes   */
/* (optimal lengths limited to 15 bits, a constant code-length code), whichever is fewer bytes -- a tie gives the fixed form --,  */
/* so no chunk is longer than the entries above write it.  row_bytes == 0 selects the run-only token rule (tip_deflate_runs'),    */
/* row_bytes > 0 the rows rule (tip_deflate_rows'); TIP_ERR_ARG for a negative row_bytes or one that is no multiple of elem_bytes.*/
/* The stream: tip_deflate.hip's dynamic section, specified in tests/deflate_dynamic_restate.py.                                  */
TIP_API int tip_deflate_dynamic_dev(const void *src_dev, int64_t nbytes, int elem_bytes, int64_t row_bytes, void *dst_dev, int64_t cap,
                                    int64_t *out_bytes_host, uint32_t *crc32_host);
TIP_API int tip_deflate_dynamic(const void *src, int64_t nbytes, int elem_bytes, int64_t row_bytes, void *dst, int64_t cap,
                                int64_t *out_bytes, uint32_t *crc32);
/* STRIPS: n_pages planes of rows x row_bytes, each cut into strips of rows_per_strip rows (the last one of a page may be shorter), */
/* every strip a zlib stream of its own (RFC 1950) -- what a TIFF with Compression 8 holds per strip: 78 01, the body, the final    */
/* empty stored block 01 00 00 FF FF and the strip's Adler-32, most significant byte first.  The body is byte for byte what          */
/* tip_deflate_rows (codes 0) or tip_deflate_dynamic with this row_bytes (codes 1) writes for THAT STRIP AS A WHOLE BUFFER, so no     */
/* match reaches before the strip; tests/deflate_strips_restate.py is the framing.  The streams are compacted into dst in            */
/* page-major order, every one at an even offset (one zero byte behind a stream of odd size); table: (offset, size) per strip as     */
/* int64 pairs, size without the pad byte; *out_bytes: the bytes written, pad bytes included.  Sizes, table and total arrive in host */
/* memory after ONE wait for the stream.  _bound: the most bytes written (per strip of n bytes 2 + the chunk bound of n + 9, made    */
/* even); touches no device.  TIP_ERR_UNSUPPORTED: rows_per_strip * row_bytes > 65536 (a strip is one chunk).  TIP_ERR_ARG: a null   */
/* pointer, elem_bytes not 1 or 2, row_bytes not a positive multiple of it, rows_per_strip < 1, another codes, a negative extent, cap */
/* below the bound.  n_pages == 0 or rows == 0: TIP_OK, zero bytes, nothing is read.                                                  */
TIP_API int tip_deflate_strips_bound(int64_t n_pages, int64_t rows, int64_t row_bytes, int64_t rows_per_strip, int64_t *bound_out);
TIP_API int tip_deflate_strips_dev(const void *src_dev, int64_t n_pages, int64_t rows, int64_t row_bytes, int elem_bytes,
                                   int64_t rows_per_strip, int codes, void *dst_dev, int64_t cap, int64_t *table_host,
                                   int64_t *out_bytes_host);
TIP_API int tip_deflate_strips(const void *src, int64_t n_pages, int64_t rows, int64_t row_bytes, int elem_bytes, int64_t rows_per_strip,
                               int codes, void *dst, int64_t cap, int64_t *table, int64_t *out_bytes);

/* ---- inflate of many deflate streams, and the 16-bit TIFF row pass (csrc/tip_inflate.hip, csrc/tip_inflate_core.h; the     */
/* ---- strips of a deflate-compressed TIFF: movie.tiff_frame_source) --------------------------------------------------------- */
/* One status word per strip.  A strip that fails is not an error of the call: the call returns TIP_OK and counts it.          */
enum tip_inflate_status {
    TIP_INFLATE_OK = 0,
    TIP_INFLATE_BAD_HEADER = 1,      /* zlib wrapper: CM != 8, CINFO > 7, FCHECK fails, or FDICT set */
    TIP_INFLATE_BAD_BLOCK_TYPE = 2,  /* BTYPE 3 */
    TIP_INFLATE_BAD_STORED = 3,      /* a stored block's LEN and NLEN are not complements */
    TIP_INFLATE_BAD_LENGTHS = 4,     /* code lengths over-subscribed, or incomplete other than the one-distance-code (or no-distance-code) */
                                     /* set zlib accepts; repeat code 16 first; a repeat past HLIT + HDIST; no end-of-block code;         */
                                     /* HLIT > 286 or HDIST > 30                                                                          */
    TIP_INFLATE_BAD_SYMBOL = 5,      /* literal/length 286 or 287, distance 30 or 31, or bits that are no code of an incomplete set */
    TIP_INFLATE_BAD_DISTANCE = 6,    /* a match reaches before the start of this strip's output */
    TIP_INFLATE_INPUT_END = 7,       /* the strip's bytes end inside the stream */
    TIP_INFLATE_OUTPUT_FULL = 8,     /* the stream holds more than dst_len bytes (nothing beyond dst_len is written) */
    TIP_INFLATE_OUTPUT_SHORT = 9,    /* the final block ends before dst_len bytes */
    TIP_INFLATE_BAD_ADLER = 10       /* zlib wrapper: the Adler-32 of the output is not the stream's */
};
/* n_strips independent streams, RFC 1951 (wrapper 0) or RFC 1950 (wrapper 1: zlib header and Adler-32), from one source buffer */
/* into one destination buffer.  strips: four int64 per strip -- src_off, src_len, dst_off, dst_len; a strip's window is its    */
/* own output, so no match reaches before dst_off, and dst_len is the exact size the stream must give.  Every read stays inside */
/* [src_off, src_off + src_len) and every write inside [dst_off, dst_off + dst_len), whatever the bytes; destination bytes      */
/* outside every strip are left as they are.  status: one int32 per strip (tip_inflate_status); *n_bad: how many are non-zero,  */
/* in a host word after one wait for the stream.  Before anything is launched the table is checked on the host (the _dev form   */
/* downloads it: 32 bytes a strip): a range outside src_bytes / dst_bytes, or two non-empty destinations that overlap, give      */
/* TIP_ERR_ARG and no device memory is written; so do a null pointer, a negative size and another wrapper.  _dev: src, strips,  */
/* dst and status are DEVICE buffers, on the calling thread's stream.  _host: the same decoder (tip_inflate_core.h) compiled    */
/* for the CPU, no device touched -- the reference the device form is tested against.                                           */
TIP_API int tip_inflate_strips_dev(const void *src_dev, int64_t src_bytes, const int64_t *strips_dev, int64_t n_strips, int wrapper,
                                   void *dst_dev, int64_t dst_bytes, int32_t *status_dev, int32_t *n_bad_host);
TIP_API int tip_inflate_strips(const void *src, int64_t src_bytes, const int64_t *strips, int64_t n_strips, int wrapper, void *dst,
                               int64_t dst_bytes, int32_t *status, int32_t *n_bad);
TIP_API int tip_inflate_strips_host(const void *src, int64_t src_bytes, const int64_t *strips, int64_t n_strips, int wrapper, void *dst,
                                    int64_t dst_bytes, int32_t *status, int32_t *n_bad);
/* In place on a DEVICE buffer of n_rows rows of row_elems 16-bit samples, asynchronous: with swap_bytes the two bytes of every */
/* sample change places (the file's byte order is not the host's), then with predictor 2 every row becomes its running sum      */
/* modulo 2^16 (TIFF horizontal differencing undone; libtiff's order: swap, then accumulate).  Rows are independent.  predictor */
/* 1: no sum; another predictor: TIP_ERR_UNSUPPORTED.                                                                            */
TIP_API int tip_tiff_finish_u16_dev(void *stack_dev, int64_t n_rows, int64_t row_elems, int predictor, int swap_bytes);

/* ---- a frame's maps as uint16 TIFF pages (csrc/tip_export.hip; movie.export_tiff) ------------------------------------------- */
/* Plane 0 of out_dev (n_pix uint16): ids_host[labels - 1], 0 on label 0 -- Tissue.get_trackking_labels cast to uint16; plane 1,    */
/* only when types_dev is given (out_dev then holds 2 n_pix): the type byte with 0 -> 2, 255 -> 0, others as they are              */
/* (export_segmentation_and_cell_types_to_tiff's map).  labels_dev, types_dev, out_dev are DEVICE buffers; ids_host is n_ids int64   */
/* on the host.  A label outside [0, n_ids] is written as 0 and counted in *n_bad_host (a host word, after one wait).  TIP_ERR_ARG:   */
/* a null pointer, a negative count, or an id outside [0, 65535] -- checked before anything is launched.                             */
TIP_API int tip_export_maps_u16_dev(const int32_t *labels_dev, const uint8_t *types_dev, int64_t n_pix, const int64_t *ids_host,
                                    int64_t n_ids, uint16_t *out_dev, int32_t *n_bad_host);

/* ---- the projected movie as uint16 TIFF pages and its z-maps (csrc/tip_export.hip; movie.export_projection) ----------------- */
/* Every _dev entry takes DEVICE buffers on the calling thread's stream; its twin without the suffix takes host arrays, touches no   */
/* device and is compiled from the same per-sample function (the reference the device form is tested against).                      */
/* tip_max_f64: the maximum of n doubles -- a frame's part of the normalisation save_tiff applies to the whole movie.  A NaN is       */
/* never taken (numpy's max would return it); all NaN gives -inf.  _dev waits ONCE, *max_host is a host word.  TIP_ERR_ARG: a null   */
/* pointer, n < 1.                                                                                                                 */
TIP_API int tip_max_f64_dev(const double *src_dev, int64_t n, double *max_host);
TIP_API int tip_max_f64(const double *src, int64_t n, double *max_out);
/* n_pages pages of rows x cols float64 samples as uint16: u = (uint16) rint((v / scale_max) * 65535), the division and the product  */
/* each rounded to nearest, no reciprocal and no fused step -- np.round((image / np.max(image)) * 65535).astype("uint16") of         */
/* bim.py:183-186 when scale_max is the image's maximum.  predictor 1 stores u; predictor 2 (TIFF horizontal differencing) stores     */
/* u[x] - u[x - 1] modulo 2^16 for x > 0 and u[0] at every row start.  scale_max == 0, an all-zero movie, writes zeros: what numpy's  */
/* 0 / 0 -> NaN -> cast gives on x86-64.  A sample outside [0, scale_max] wraps modulo 2^16 as numpy's cast does there, a NaN gives   */
/* 0.  _dev is asynchronous.  TIP_ERR_ARG: a null pointer, a negative extent, cols above 2^31 - 1, more than 10^12 samples,           */
/* scale_max negative or not finite.  TIP_ERR_UNSUPPORTED: another predictor.  No samples: TIP_OK, nothing is read.                  */
TIP_API int tip_projection_pages_u16_dev(const double *src_dev, int64_t n_pages, int64_t rows, int64_t cols, double scale_max,
                                         int predictor, uint16_t *out_dev);
TIP_API int tip_projection_pages_u16(const double *src, int64_t n_pages, int64_t rows, int64_t cols, double scale_max, int predictor,
                                     uint16_t *out);
/* astype("uint16") of n int64 (the z-map as sp.py:229-230 saves it): modulo 2^16.  _dev is asynchronous.  TIP_ERR_ARG: a null       */
/* pointer, n negative (or above 10^12 for _dev).                                                                                   */
TIP_API int tip_zmap_u16_dev(const int64_t *src_dev, int64_t n, uint16_t *out_dev);
TIP_API int tip_zmap_u16(const int64_t *src, int64_t n, uint16_t *out);

/* ---- the sensory-region filter (ti.py:614-620 detect_non_sensory_region_cells, 2781-2792                                          */
/* remove_cells_outside_of_sensory_region; csrc/tip_hull.hip) ---------------------------------------------------- */
/* Every geometric decision below is the exact sign of (b - a) x (p - a) on the float64 coordinates (csrc/tip_orient.h: a floating     */
/* filter, then error-free transformations), on the device and on the host alike: no tolerance enters a hull or an outside flag.       */
/* The convex hull of n planar points (px, py float64): the 0-based positions of its vertices, counter-clockwise in the (x, y) plane    */
/* from the lexicographically smallest (x, then y) vertex.  A point on an edge between two vertices is no vertex; among coincident      */
/* points the lowest position stands for all.  hull has room for cap entries; *n_hull = the vertices found, TIP_ERR_OVERFLOW when that   */
/* exceeds cap (nothing is written to hull then), TIP_ERR_DEGENERATE when there are fewer than three -- fewer than three distinct        */
/* points, or all on one line (*n_hull is then 0, 1 or 2).  n up to 2^30, of which at most 65 536 may SURVIVE the octagon filter --    */
/* the points not strictly inside the octagon of the eight extremes of x, y, x + y, x - y: a few hundred of 10^6 uniform points, but     */
/* all points of a circle --, because the vertex test is quadratic in them; more give TIP_ERR_UNSUPPORTED and nothing is written       */
/* (tip_sensory_region_i32_dev alike; tip_sensory_region_host has no such limit).  The host form rejects a non-finite coordinate (ARG);  */
/* in the _dev form such a point takes no part.  _dev: px, py, hull are DEVICE arrays, *n_hull_host a host word; the call waits for      */
/* the stream (once to size its sort, once for the count).                                                                              */
TIP_API int tip_convex_hull_f64(const double *px, const double *py, int64_t n, int32_t *hull, int64_t cap, int64_t *n_hull);
TIP_API int tip_convex_hull_f64_dev(const double *px, const double *py, int64_t n, int32_t *hull, int64_t cap, int64_t *n_hull_host);
/* outside[q] = 1 when query (qx[q], qy[q]) lies STRICTLY outside the convex polygon hull[0 .. h) (positions into px, py; counter-      */
/* clockwise, strictly convex, h >= 3: what tip_convex_hull_f64 returns), 0 on its boundary and inside.  m = 0 is valid.  The host form  */
/* checks the positions and rejects non-finite coordinates; the _dev form (device arrays, asynchronous) answers 0 for a query whose     */
/* search meets a position outside 0 .. n - 1, and its answer for a non-finite query is unspecified.                                    */
TIP_API int tip_points_outside_hull_f64(const double *px, const double *py, int64_t n, const int32_t *hull, int64_t h, const double *qx,
                                        const double *qy, int64_t m, uint8_t *outside);
TIP_API int tip_points_outside_hull_f64_dev(const double *px, const double *py, int64_t n, const int32_t *hull, int64_t h,
                                            const double *qx, const double *qy, int64_t m, uint8_t *outside);
/* types[p] = 255 where 1 <= labels[p] <= n and outside[labels[p] - 1] != 0; every other byte is left as it is -- the np.isin write of    */
/* ti.py:2791.  labels (int32), types (uint8), outside (uint8[n]) are DEVICE arrays; asynchronous.                                      */
TIP_API int tip_invalidate_cells_u8_dev(const int32_t *labels, uint8_t *types, int64_t n_pix, const uint8_t *outside_dev, int64_t n);
/* The movie driver's one call per frame.  Host rows over labels 1..n: centroids cx, cy, and the bytes type, valid, empty (empty NULL:   */
/* no empty row).  The hull points are the rows with type == 1, valid == 1 and empty == 0 -- equalities, not bit tests; type and valid  */
/* both NULL: every row.  outside[r] (host, uint8[n]) = 1 where row r lies strictly outside their hull -- EVERY row is tested, also the  */
/* invalid and empty ones --, hull (host, capacity hull_cap) = the hull's row positions as tip_convex_hull_f64 orders them, *n_hull      */
/* their number; with labels / types (DEVICE maps of n_pix pixels, both or neither) the type map gets 255 on the outside rows' pixels.   */
/* One upload of the rows, one download of flags and hull, on the calling thread's stream; returns when both are in place.              */
/* TIP_ERR_DEGENERATE (no hull) and TIP_ERR_OVERFLOW leave outside, hull and the map untouched; TIP_ERR_ARG: a non-finite centroid, a    */
/* null pointer, a negative count.                                                                                                    */
TIP_API int tip_sensory_region_i32_dev(const int32_t *labels, uint8_t *types, int64_t n_pix, const double *cx, const double *cy,
                                       const uint8_t *type, const uint8_t *valid, const uint8_t *empty, int64_t n, uint8_t *outside,
                                       int32_t *hull, int64_t hull_cap, int64_t *n_hull);
/* The same selection, hull and test on plain host arrays: touches no device, has no map, shares the predicate with the kernels but not  */
/* their algorithms (monotone chain; edge-by-edge test) -- the reference the device forms are tested against.  outside NULL: the hull     */
/* alone.                                                                                                                             */
TIP_API int tip_sensory_region_host(const double *cx, const double *cy, const uint8_t *type, const uint8_t *valid, const uint8_t *empty,
                                    int64_t n, uint8_t *outside, int32_t *hull, int64_t hull_cap, int64_t *n_hull);

#ifdef __cplusplus
}
#endif
#endif
