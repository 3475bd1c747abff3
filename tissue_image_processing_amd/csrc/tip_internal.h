// tip_internal.h -- shared plumbing of libtissue_hip.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/tissue_hip.h"

namespace tip {

struct ProfRec { const char *name; hipEvent_t e0, e1; };

// One context per calling thread: the reference is driven from Qt worker threads (gui.py:1821-2137),
// ctypes releases the GIL, so entry points must be re-entrant.
struct Ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    std::string err;
    // workspace pool: cached device blocks, best-fit reuse
    struct Block { void *p; size_t bytes; bool used; };
    std::vector<Block> pool;
    int last_ws_labels = 0;   // marker count of this thread's last watershed (tip_last_watershed_labels)
    long last_ws_other = 0;   // ... and its number of pixels that are neither the image's minimum nor its maximum
    hipEvent_t edge_event = nullptr;   // tip_wait_stream / tip_stream_wait_tip
    void *prep_ws = nullptr;           // order-statistic state of tip_unet_prepare_f64_dev (used on the caller's stream only)
    unsigned *unet_status = nullptr;   // 4-byte device word, bit 0: an fp16-piece U-Net launch of this thread met a value beyond fp16's range
    int *unet_status_host = nullptr;   // ... and the pinned word tip_unet_range_read copies it to (tip_unet.hip: unet_status_word)
    void *pin_buf = nullptr;           // pinned host staging (the watershed's marker-order stage: counts down, pop order up)
    size_t pin_bytes = 0;
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> free_events;
};

Ctx &ctx();                       // lazily initialised for device 0 unless tip_init() chose another
int fail(int code, const char *fmt, ...);
int launch_check(const char *what);   // hipGetLastError() behind launches on a caller's stream: TIP_OK, or TIP_ERR_HIP with "launch <what>: ..."
void *ws_alloc(size_t bytes);     // nullptr on failure (error text set)
void *pinned_scratch(size_t bytes);   // this thread's pinned host staging buffer, grown as needed (nullptr on failure)
void ws_free(void *p);

struct WsGuard {                  // frees workspaces at scope exit
    std::vector<void *> ptrs;
    template <typename T> T *get(size_t count) {
        void *p = ws_alloc(count * sizeof(T) ? count * sizeof(T) : 16);
        if (p) ptrs.push_back(p);
        return (T *)p;
    }
    ~WsGuard() { for (void *p : ptrs) ws_free(p); }
};

// The device side of one host-form call (host arrays in and out): uploads, output buffers and scratch on the context stream.
// The first failure -- an allocation or a HIP call -- stays in rc and turns every later call into a no-op, so a host form tests
// rc once before it launches.  finish() queues the downloads of the registered outputs and waits for the stream; a form that
// returns early never reaches it, and nothing is written to the caller's arrays.
struct Staging {
    WsGuard ws;
    int rc = TIP_OK;
    struct Out { void *host; const void *dev; size_t bytes; };
    std::vector<Out> outs;

    bool hip(hipError_t e, const char *what)
    {
        if (e != hipSuccess && !rc) rc = fail(TIP_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
        return !rc;
    }
    template <typename T> T *scratch(size_t count)
    {
        if (rc) return nullptr;
        T *d = ws.get<T>(count);
        if (!d) rc = TIP_ERR_NOMEM;
        return d;
    }
    // the device copy of a host array; a NULL host array stays NULL
    template <typename T> T *in(const T *host, size_t count)
    {
        T *d = host ? scratch<T>(count) : nullptr;
        if (d && count) hip(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, ctx().stream), "hipMemcpyAsync (upload)");
        return d;
    }
    // a device buffer that finish() copies to the host array; a NULL host array gives NULL and no copy
    template <typename T> T *out(T *host, size_t count, bool zero = false)
    {
        T *d = host ? scratch<T>(count) : nullptr;
        if (d && zero && count) hip(hipMemsetAsync(d, 0, count * sizeof(T), ctx().stream), "hipMemsetAsync");
        if (d) outs.push_back({host, d, count * sizeof(T)});
        return d;
    }
    // an output whose element count is known only after the launch: finish() copies the first `count` (at most what out() took)
    template <typename T> void set_count(const T *dev, size_t count)
    {
        for (Out &o : outs)
            if (o.dev == dev && count * sizeof(T) < o.bytes) o.bytes = count * sizeof(T);
    }
    int finish()
    {
        for (const Out &o : outs)
            if (o.bytes && !hip(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, ctx().stream), "hipMemcpyAsync (download)")) break;
        if (!rc) hip(hipStreamSynchronize(ctx().stream), "hipStreamSynchronize");
        return rc;
    }
};

void prof_begin(const char *name);
void prof_end();

// Process-wide tuning / test hooks.  Filled ONCE from the environment (TIP_* variables) when the library is loaded and
// changed afterwards only through tip_set_tuning(): entry points read plain ints, never the environment.
struct Tuning {
    int ws_ties = 1;            // TIP_WS_TIES: 1 = exact (serial (value, age) replay on tie landscapes), 0 = fast (device order)
    int ws_open_a = -1, ws_open_b = -1;   // TIP_WS_OPEN=a,b
    int ws_no_skip = 0;         // TIP_WS_NO_SKIP
    int ws_debug = 0;           // TIP_WS_DEBUG
    int ws_no_endgame = 0, ws_no_wide = 0;   // TIP_WS_NO_ENDGAME / TIP_WS_NO_WIDE (exercise the stall machinery)
    int project_generic = 0, project_unfused_preblur = 0, project_unfused_mask = 0;
    int project_exact_score = 0, project_debug = 0;
    int unet_tail_unfused = 0;  // TIP_UNET_TAIL_UNFUSED: the tail's morphology as separate rank-filter launches (tests)
    int unet_xcd_map = 1;       // TIP_UNET_XCD_MAP: the channel blocks of one pixel tile side by side on one XCD (0: all workgroups in flight on one channel block)
    int unet_spb = 3;           // TIP_UNET_SPB: steps per barrier of the 3x3 16-row convolution kernel (1 or 3; above 1 means 3)
    int unet_mfma = 32;         // TIP_UNET_MFMA: K of the MFMA of the f16x3 16-row convolutions with >= 4 taps (32: 16x16x32; anything else: 16 = 32x32x16)
    int unet_first_mfma = 1;    // TIP_UNET_FIRST: mode f16x3's first layer, 1 (mfma) = k_unet_conv_first_mfma, 0 (valu) = the float32 vector kernel; n > 1: mfma with n workgroups per CU
    int uf_one_level = 0;       // TIP_UF_ONE_LEVEL: the one-level union-find (global atomics only) instead of tiles in LDS + borders (tests)
    int mb_small = -1;          // TIP_MB_SMALL: generations of the two-valued flood of at most this many pixels run in one workgroup (0: never; -1: the built-in default)
    int mb_batch = -1;          // TIP_MB_BATCH: generations queued between two looks at the device state (-1: the built-in default)
    int unet_tile8 = -1;        // TIP_UNET_TILE8: the U-Net convolution's tile rows: 1 = 8 everywhere, 0 = 16 where the grid allows, -1 (default) = 16 except for 3x3 layers with <= 128 input channels
};
const Tuning &tuning();

#define TIP_HIP(call)                                                                             \
    do {                                                                                          \
        hipError_t e__ = (call);                                                                  \
        if (e__ != hipSuccess)                                                                    \
            return tip::fail(TIP_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                             __FILE__, __LINE__);                                                 \
    } while (0)

// launch a kernel on the context stream, timed with HIP events when profiling is on
#define TIP_LAUNCH(name, kernel, grid, block, shmem, ...)                                  \
    do {                                                                                   \
        tip::prof_begin(name);                                                             \
        hipLaunchKernelGGL(kernel, grid, block, shmem, tip::ctx().stream, __VA_ARGS__);    \
        tip::prof_end();                                                                   \
        hipError_t e__ = hipGetLastError();                                                \
        if (e__ != hipSuccess)                                                             \
            return tip::fail(TIP_ERR_HIP, "launch %s: %s", name, hipGetErrorString(e__));  \
    } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Gaussian taps passed by value in the kernel-argument segment (scalar loads, no device copy).
struct Taps {
    double w[256];
    int n;
};
struct TapsF {   // float32 copy for the certified fast score passes
    float w[256];
    int n;
};

int make_taps(Taps &t, const double *w, int n);  // validates odd + symmetric (scipy's symmetric branch)
int libm_taps(double sigma, double truncate, double *w, int cap);
// tip_gauss.hip: one scipy-order correlate pass on device volumes.  dtype 0 = f32, 1 = f64.  force: 0 auto, 1 generic, 2 long
int correlate1d_dev(const void *in, void *out, int dtype, int Z, int Y, int X, int axis, const Taps &t, int force);

// tip_optflow.hip: the TV-L1 flow on device planes, asynchronous unless warps_host is given; returns the pyramid's level
// count or an error code.  dtype: the public codes of tip_optical_flow_tvl1 or OF_F64_AS_U16, a float64 plane truncated to
// uint16 and then scaled as code 3 (tip_piv.hip: the projection as the GUI tracks it) -- one read of each plane.
constexpr int OF_F64_AS_U16 = 5;
int optical_flow_tvl1_dev(const void *ref, const void *mov, int dtype, int y, int x, float attachment, float tightness,
                          int num_warp, int num_iter, double tol, float *flow_out, int32_t *warps_host, int cap);

// tip_label.hip: exclusive scans of int32 on device arrays, asynchronous.  exclusive_scan_i32: out[i] = in[0] + ... + in[i - 1] for
// i < n device-wide, the sum to *total_dev (may be NULL).  scan_i32_dev: the same by one workgroup, for the small tables; out
// has n + 1 entries and out[n] is the sum.
int exclusive_scan_i32(const int *in, int *out, long n, int *total_dev);
int scan_i32_dev(const int32_t *in, int32_t *out, int n);

// the device forms one unit borrows from another (their arguments are described where they are defined)
int regionprops_dev(const int32_t *labels, const double *intensity, int Y, int X, int n, int64_t *area, int64_t *bbox4, int64_t *sumy,
                    int64_t *sumx, int64_t *pc3, double *isum);                                                          // tip_props.hip
int order_stats_dev(const int32_t *labels, const double *img, long n, int nlab, long long *rank, const long long *rank0, double *lo,
                    double *hi);                                                                                         // tip_select.hip
int gaussian3d_dev(const void *in, void *out, int dtype, int Z, int Y, int X, const double *tz, int nz, const double *ty, int ny,
                   const double *tx, int nx);                                                                            // tip_gauss.hip
int rankfilter2d_dev(const void *in, void *out, int dtype, int Y, int X, int ky, int kx, int fp, int border, int is_max);   // tip_label.hip
int watershed_dev(const double *img, int32_t *labels, int Y, int X, int wsl, int32_t *flags_host);                          // tip_watershed.hip

}  // namespace tip

#include "tip_wave.h"   // wave_combine, wave_reduce, wave_inclusive_scan, block_exclusive_scan, block_reduce: the device primitives
