// tip_fft.hip -- global drift between two frames: skimage.registration.phase_cross_correlation(upsample_factor)
// (reference call sites ti.py:1976-1977, 2029-2030 via update_drift / calculate_refine_drift, and bim.py:522-536).
//
//   F1 = fft2(ref), F2 = fft2(mov); P = F1 * conj(F2); whole-pixel peak = argmax |ifft2(P)|;
//   refinement = matrix-multiply upsampled DFT of conj(P) on a ceil(1.5*upsample)^2 grid around the peak
//   (skimage/registration/_phase_cross_correlation.py:11-76, 196-262; skimage 0.18.3 applies no normalisation).
// Everything in float64 (the reference hands uint16 / float64 frames to scipy.fft -> complex128).  The library returns
// the two integer peaks; the host turns them into the shift with numpy's own arithmetic.  Hand-written radix-2 FFT:
// power-of-two extents up to 4096 (one block per row, the row in LDS), columns through a tiled transpose.
// There is ONE correlation body (correlate_windows): n windows of a frame pair, a chunk of windows per pass.  The whole
// plane (phase_correlation_dev) is the batch of one window that covers the frame.
#include "tip_internal.h"

namespace tip {

typedef double2 cplx;

__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// window w = blockIdx.y is the Ny x Nx block at (org[4w + side], org[4w + side + 1]) of a frame with rows of frame_x
// elements (side 0: reference, 2: moving frame), cropped, converted and laid out contiguously (window w at out + w * Ny * Nx)
template <typename T>
__global__ void __launch_bounds__(256) k_load_windows(const T *__restrict__ frame, int frame_x, const int *__restrict__ org, int side,
                                                      cplx *__restrict__ out, int Ny, int Nx)
{
    const long n = (long)Ny * Nx;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int w = blockIdx.y, y = (int)(i / Nx), x = (int)(i - (long)y * Nx);
    const long r0 = org[4 * w + side], c0 = org[4 * w + side + 1];
    out[(long)w * n + i] = make_double2((double)frame[(r0 + y) * frame_x + c0 + x], 0.0);
}

__global__ void __launch_bounds__(256) k_twiddles(cplx *__restrict__ w, int N)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < N / 2) {
        double s, c;
        sincospi(-2.0 * (double)k / (double)N, &s, &c);
        w[k] = make_double2(c, s);
    }
}

// in-place FFT of every row (length N, power of two, N <= 4096); inverse = conjugate twiddles (no scaling)
__global__ void __launch_bounds__(256) k_fft_rows(cplx *__restrict__ data, const cplx *__restrict__ tw, int N, int logN, int inverse)
{
    extern __shared__ __attribute__((aligned(16))) double2 row[];
    cplx *p = data + (long)blockIdx.x * N;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const int j = (int)(__brev((unsigned)i) >> (32 - logN));
        row[j] = p[i];
    }
    __syncthreads();
    for (int s = 1; s <= logN; ++s) {
        const int half = 1 << (s - 1);
        const int step = N >> s;  // twiddle stride
        for (int t = threadIdx.x; t < N / 2; t += blockDim.x) {
            const int grp = t / half, pos = t - grp * half;
            const int i0 = grp * (half << 1) + pos, i1 = i0 + half;
            cplx w = tw[pos * step];
            if (inverse) w.y = -w.y;
            const cplx a = row[i0], b = cmul(row[i1], w);
            row[i0] = make_double2(a.x + b.x, a.y + b.y);
            row[i1] = make_double2(a.x - b.x, a.y - b.y);
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < N; i += blockDim.x) p[i] = row[i];
}

// ---- arbitrary lengths: Bluestein's chirp-z on top of the power-of-two butterflies --------------------------------------
// X[k] = b[k] * sum_n (x[n] b[n]) conj(b[k-n]),  b[n] = exp(-i pi n^2 / N): a length-N DFT as a circular convolution of
// length M = 2^ceil(log2(2N-1)), done in LDS per row: forward DIF (natural in, bit-reversed out), pointwise product with
// the chirp's transform (stored in the same bit-reversed order), inverse DIT (bit-reversed in, natural out).
__global__ void __launch_bounds__(256) k_chirp(cplx *__restrict__ b, int N)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const long r = ((long)n * n) % (2L * N);          // n^2 mod 2N exactly: the phase only matters modulo 2 pi
    double sn, cs;
    sincospi(-(double)r / (double)N, &sn, &cs);
    b[n] = make_double2(cs, sn);
}

__device__ __forceinline__ void lds_dif(cplx *row, const cplx *__restrict__ tw, int M, int logM)
{
    for (int s = logM; s >= 1; --s) {
        const int half = 1 << (s - 1), step = M >> s;
        for (int t = threadIdx.x; t < M / 2; t += blockDim.x) {
            const int grp = t / half, pos = t - grp * half;
            const int i0 = grp * (half << 1) + pos, i1 = i0 + half;
            const cplx a = row[i0], c = row[i1];
            row[i0] = make_double2(a.x + c.x, a.y + c.y);
            row[i1] = cmul(make_double2(a.x - c.x, a.y - c.y), tw[pos * step]);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void lds_dit_inverse(cplx *row, const cplx *__restrict__ tw, int M, int logM)
{
    for (int s = 1; s <= logM; ++s) {
        const int half = 1 << (s - 1), step = M >> s;
        for (int t = threadIdx.x; t < M / 2; t += blockDim.x) {
            const int grp = t / half, pos = t - grp * half;
            const int i0 = grp * (half << 1) + pos, i1 = i0 + half;
            cplx w = tw[pos * step];
            w.y = -w.y;
            const cplx a = row[i0], c = cmul(row[i1], w);
            row[i0] = make_double2(a.x + c.x, a.y + c.y);
            row[i1] = make_double2(a.x - c.x, a.y - c.y);
        }
        __syncthreads();
    }
}

// transform of the wrapped conjugate chirp, left in DIF (bit-reversed) order
__global__ void __launch_bounds__(256) k_bluestein_filter(cplx *__restrict__ cf, const cplx *__restrict__ b, const cplx *__restrict__ tw,
                                                          int N, int M, int logM)
{
    extern __shared__ __attribute__((aligned(16))) double2 row[];
    for (int m = threadIdx.x; m < M; m += blockDim.x) {
        cplx v = make_double2(0.0, 0.0);
        if (m < N) v = make_double2(b[m].x, -b[m].y);
        else if (m > M - N) v = make_double2(b[M - m].x, -b[M - m].y);
        row[m] = v;
    }
    __syncthreads();
    lds_dif(row, tw, M, logM);
    for (int m = threadIdx.x; m < M; m += blockDim.x) cf[m] = row[m];
}

// in-place DFT of every row of length N (any N with 2N-1 <= M); inverse = conjugate in, conjugate out (no scaling)
__global__ void __launch_bounds__(256) k_fft_rows_bluestein(cplx *__restrict__ data, const cplx *__restrict__ tw,
                                                            const cplx *__restrict__ b, const cplx *__restrict__ cf, int N, int M,
                                                            int logM, int inverse)
{
    extern __shared__ __attribute__((aligned(16))) double2 row[];
    cplx *p = data + (long)blockIdx.x * N;
    for (int i = threadIdx.x; i < M; i += blockDim.x) {
        cplx v = make_double2(0.0, 0.0);
        if (i < N) {
            v = p[i];
            if (inverse) v.y = -v.y;
            v = cmul(v, b[i]);
        }
        row[i] = v;
    }
    __syncthreads();
    lds_dif(row, tw, M, logM);
    for (int i = threadIdx.x; i < M; i += blockDim.x) row[i] = cmul(row[i], cf[i]);
    __syncthreads();
    lds_dit_inverse(row, tw, M, logM);
    const double sc = 1.0 / (double)M;
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        cplx v = cmul(row[k], b[k]);
        v.x *= sc; v.y *= sc;
        if (inverse) v.y = -v.y;
        p[k] = v;
    }
}

// (blockIdx.z: the window of a batch, rows * cols elements each)
__global__ void __launch_bounds__(256) k_transpose_c(const cplx *__restrict__ in, cplx *__restrict__ out, int rows, int cols)
{
    __shared__ double2 t[16][17];
    in += (long)blockIdx.z * rows * cols;
    out += (long)blockIdx.z * rows * cols;
    const int bx = blockIdx.x * 16, by = blockIdx.y * 16;
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    if (by + ly < rows && bx + lx < cols) t[ly][lx] = in[(long)(by + ly) * cols + bx + lx];
    __syncthreads();
    if (bx + ly < cols && by + lx < rows) out[(long)(bx + ly) * rows + by + lx] = t[lx][ly];
}

__global__ void __launch_bounds__(256) k_cmul_conj(const cplx *__restrict__ a, const cplx *__restrict__ b, cplx *__restrict__ out, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const cplx x = a[i], y = b[i]; out[i] = make_double2(x.x * y.x + x.y * y.y, x.y * y.x - x.x * y.y); }
}

// first maximum of |z| in raster order (np.argmax): pack (|z|^2 bits, ~index) and take the max.  Segmented over a batch: window
// blockIdx.y has its n elements at z + blockIdx.y * n and its own best_v / best_i entry (indices within the window)
__global__ void __launch_bounds__(256) k_absargmax(const cplx *__restrict__ z, long n, unsigned long long *__restrict__ best_v,
                                                   unsigned long long *__restrict__ best_i)
{
    z += (long)blockIdx.y * n;
    best_v += blockIdx.y;
    // two passes would be cleaner; a single one with a (value, index) lexicographic atomic is enough here:
    // |z|^2 >= 0, so its IEEE bits order like the value
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = 0;
    if (i < n) {
        const double m = hypot(z[i].x, z[i].y);   // np.abs of complex128 is hypot
        key = (unsigned long long)__double_as_longlong(m);
    }
    const unsigned long long wmax = wave_max(key);
    if ((threadIdx.x & 63) == 0) atomicMax(best_v, wmax);
    (void)best_i;
}
__global__ void __launch_bounds__(256) k_absargmax2(const cplx *__restrict__ z, long n, const unsigned long long *__restrict__ best_v,
                                                    unsigned long long *__restrict__ best_i)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    z += (long)blockIdx.y * n;
    const double m = hypot(z[i].x, z[i].y);
    if ((unsigned long long)__double_as_longlong(m) == best_v[blockIdx.y]) atomicMin(best_i + blockIdx.y, (unsigned long long)i);
}

// K[u][k] = exp(-2 pi i (u - off) * fftfreq(N, ups)[k])   (skimage _upsampled_dft kernel)
__device__ __forceinline__ cplx dft_kernel_entry(long i, int N, double off, double ups)
{
    const int u = (int)(i / N), k = (int)(i - (long)u * N);
    const int kk = k < (N + 1) / 2 ? k : k - N;                 // numpy fftfreq ordering
    const double val = 1.0 / ((double)N * ups);                 // numpy.fft.fftfreq: integer results * (1 / (n * d))
    const double f = (double)kk * val;
    const double arg = ((double)u - off) * f;                    // kernel = (arange - off)[:, None] * fftfreq
    double s, c;
    sincos(-2.0 * 3.141592653589793 * arg, &s, &c);              // np.exp(-1j * 2 * pi * kernel)
    return make_double2(c, s);
}

// Window blockIdx.y takes its offset from its own coarse peak (peak[w], raster index in the Ny x Nx window) on the device, so
// the host never waits for the coarse peak; axis 0: the row kernel (N = Ny), 1: the column kernel (N = Nx).  The signed
// whole-pixel shift s is an integer and so is ups, so s * ups, its rounding onto the upsampled grid (np.round(s * ups) / ups
// = s) and dftshift - s * ups are all exact in double, whatever the order or contraction of the operations: the offset is the
// number skimage forms on the host.
__global__ void __launch_bounds__(256) k_dft_kernel_windows(cplx *__restrict__ K, int region, int N, const unsigned long long *__restrict__ peak,
                                                            int Nx, int axis, double dftshift, double ups)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)region * N) return;
    const long p = (long)peak[blockIdx.y];
    double s = axis == 0 ? (double)(p / Nx) : (double)(p % Nx);
    if (s > floor(N / 2.0)) s -= N;
    K[(long)blockIdx.y * region * N + i] = dft_kernel_entry(i, N, dftshift - s * ups, ups);
}

// C1[u][j] = sum_k Kx[u][k] * conj(conj(PT[k][j])) ... data = conj(P): C1[u][j] = sum_k Kx[u][k] * conj(P[j][k]);
// PT is P transposed (Nx rows of Ny), so the k loop walks rows of PT and j is contiguous.
__global__ void __launch_bounds__(256) k_updft1(const cplx *__restrict__ Kx, const cplx *__restrict__ PT, cplx *__restrict__ C1, int region,
                                                int Nx, int Ny)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, u = blockIdx.y;
    if (j >= Ny) return;
    Kx += (long)blockIdx.z * region * Nx;                       // (blockIdx.z: the window of a batch)
    PT += (long)blockIdx.z * Nx * Ny;
    C1 += (long)blockIdx.z * region * Ny;
    double ax = 0.0, ay = 0.0;
    const cplx *kr = Kx + (long)u * Nx;
    for (int k = 0; k < Nx; ++k) {
        const cplx w = kr[k];
        cplx d = PT[(long)k * Ny + j];
        d.y = -d.y;                                             // conj(P)
        ax += w.x * d.x - w.y * d.y;
        ay += w.x * d.y + w.y * d.x;
    }
    C1[(long)u * Ny + j] = make_double2(ax, ay);
}

// out[v][u] = conj( sum_j Ky[v][j] * C1[u][j] )
__global__ void __launch_bounds__(64) k_updft2(const cplx *__restrict__ Ky, const cplx *__restrict__ C1, cplx *__restrict__ out, int region,
                                               int Ny)
{
    const int u = blockIdx.x, v = blockIdx.y;
    Ky += (long)blockIdx.z * region * Ny;                       // (blockIdx.z: the window of a batch)
    C1 += (long)blockIdx.z * region * Ny;
    out += (long)blockIdx.z * region * region;
    double ax = 0.0, ay = 0.0;
    for (int j = threadIdx.x; j < Ny; j += 64) {
        const cplx w = Ky[(long)v * Ny + j], d = C1[(long)u * Ny + j];
        ax += w.x * d.x - w.y * d.y;
        ay += w.x * d.y + w.y * d.x;
    }
    ax = wave_sum(ax); ay = wave_sum(ay);
    if (threadIdx.x == 0) out[(long)v * region + u] = make_double2(ax, -ay);
}

static int ilog2(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }

// per-length tables: power of two -> twiddles only; any other length -> Bluestein (chirp, filter transform, twiddles of M)
struct RowPlan {
    int N = 0, M = 0, logM = 0;
    bool pow2 = true;
    cplx *tw = nullptr, *chirp = nullptr, *cf = nullptr;
};

static int make_plan(RowPlan &pl, int N, WsGuard &ws)
{
    pl.N = N;
    pl.pow2 = (N & (N - 1)) == 0;
    pl.M = N;
    if (!pl.pow2) { pl.M = 1; while (pl.M < 2 * N - 1) pl.M <<= 1; }
    pl.logM = ilog2(pl.M);
    pl.tw = ws.get<cplx>(pl.M / 2 + 1);
    if (!pl.tw) return TIP_ERR_NOMEM;
    TIP_LAUNCH("twiddles", k_twiddles, dim3(cdiv(pl.M / 2, 256)), dim3(256), 0, pl.tw, pl.M);
    if (!pl.pow2) {
        pl.chirp = ws.get<cplx>(N);
        pl.cf = ws.get<cplx>(pl.M);
        if (!pl.chirp || !pl.cf) return TIP_ERR_NOMEM;
        TIP_LAUNCH("chirp", k_chirp, dim3(cdiv(N, 256)), dim3(256), 0, pl.chirp, N);
        TIP_HIP(hipFuncSetAttribute((const void *)k_bluestein_filter, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
        TIP_LAUNCH("bluestein_filter", k_bluestein_filter, dim3(1), dim3(256), (size_t)pl.M * sizeof(cplx), pl.cf, (const cplx *)pl.chirp,
                   (const cplx *)pl.tw, N, pl.M, pl.logM);
    }
    return TIP_OK;
}

static int fft_rows(cplx *data, int nrows, const RowPlan &pl, int inverse)
{
    if (pl.pow2) {
        TIP_HIP(hipFuncSetAttribute((const void *)k_fft_rows, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
        TIP_LAUNCH("fft_rows", k_fft_rows, dim3(nrows), dim3(256), (size_t)pl.N * sizeof(cplx), data, (const cplx *)pl.tw, pl.N, pl.logM,
                   inverse);
    } else {
        TIP_HIP(hipFuncSetAttribute((const void *)k_fft_rows_bluestein, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
        TIP_LAUNCH("fft_rows_bluestein", k_fft_rows_bluestein, dim3(nrows), dim3(256), (size_t)pl.M * sizeof(cplx), data,
                   (const cplx *)pl.tw, (const cplx *)pl.chirp, (const cplx *)pl.cf, pl.N, pl.M, pl.logM, inverse);
    }
    return TIP_OK;
}

// 2-D transform of nb windows (Ny rows of Nx each, window after window in a): rows over all nb * Ny rows, transpose per
// window, rows over all nb * Nx rows -> every window's transform TRANSPOSED (Nx rows of Ny) in tmp.  The inverse of such a
// transposed transform is the same call with the two extents and plans swapped.
static int fft2_windows(cplx *a, cplx *tmp, int nb, int Ny, int Nx, const RowPlan &px, const RowPlan &py, int inverse)
{
    int rc;
    if ((rc = fft_rows(a, nb * Ny, px, inverse))) return rc;
    TIP_LAUNCH("transpose_c", k_transpose_c, dim3(cdiv(Nx, 16), cdiv(Ny, 16), nb), dim3(256), 0, (const cplx *)a, tmp, Ny, Nx);
    return fft_rows(tmp, nb * Nx, py, inverse);
}

// ---- the correlation: n windows of one frame pair, a chunk of windows per pass --------------------------------------------
// The rows of all windows of a chunk are more rows for the row kernels, every other kernel takes the window as a grid
// dimension, so a window's four integers do not depend on the windows beside it.  Per chunk: one load kernel per frame, the
// launches of one correlation, ONE stream wait.

// Workspace a chunk may take when the caller leaves the chunk size open: the four complex planes plus the upsampled-DFT
// matrices of its windows (58 windows of 700 x 700 with upsample 100, about 40 000 rows per row launch).  From this arithmetic,
// not from a measurement.
constexpr size_t WINDOW_BATCH_BYTES = (size_t)2 << 30;
constexpr int WINDOW_BATCH_MAX = 65535;    // a window is a grid's y or z index

template <typename T>
static int load_windows(const void *frame, int frame_x, const int *org, int side, cplx *out, int nb, int Ny, int Nx)
{
    TIP_LAUNCH("load_windows", k_load_windows<T>, dim3(cdiv((long)Ny * Nx, 256), nb), dim3(256), 0, (const T *)frame, frame_x, org, side,
               out, Ny, Nx);
    return TIP_OK;
}

// dtype: 0 f32, 1 f64, 3 u16.  origins (host): n x (ref row, ref col, mov row, mov col); null: every window at (0, 0, 0, 0),
// which costs no upload.  out4n (host): per window the coarse peak (row, col) and the fine peak (row, col) on the upsampled
// grid.  who: the entry's name for the messages.
static int correlate_windows(const char *who, const void *ref, const void *mov, int dtype, int frame_y, int frame_x, int n,
                             const int32_t *origins, int Ny, int Nx, int upsample, int max_batch, int64_t *out4n_host)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!ref || !mov || !out4n_host) return fail(TIP_ERR_ARG, "%s: null pointer", who);
    if (n < 0 || max_batch < 0) return fail(TIP_ERR_ARG, "%s: n %d, max_batch %d", who, n, max_batch);
    if (Ny < 2 || Nx < 2 || Ny > 4096 || Nx > 4096)
        return fail(TIP_ERR_UNSUPPORTED, "%s: extents must lie in [2, 4096] (got %dx%d)", who, Ny, Nx);
    if (upsample < 1 || upsample > 1000) return fail(TIP_ERR_ARG, "%s: upsample_factor %d", who, upsample);
    if (dtype != 0 && dtype != 1 && dtype != 3) return fail(TIP_ERR_ARG, "%s: dtype %d (0 f32, 1 f64, 3 u16)", who, dtype);
    if (frame_y < Ny || frame_x < Nx) return fail(TIP_ERR_ARG, "%s: %dx%d windows in a %dx%d frame", who, Ny, Nx, frame_y, frame_x);
    for (int w = 0; origins && w < n; ++w)
        for (int side = 0; side < 4; side += 2) {
            const int r0 = origins[4 * w + side], c0 = origins[4 * w + side + 1];
            if (r0 < 0 || c0 < 0 || r0 > frame_y - Ny || c0 > frame_x - Nx)
                return fail(TIP_ERR_ARG, "%s: window %d (%dx%d at %d, %d) leaves its %dx%d frame", who, w, Ny, Nx, r0, c0, frame_y, frame_x);
        }
    const size_t nw = (size_t)Ny * Nx;
    const int region = upsample > 1 ? (int)ceil(upsample * 1.5) : 0;
    const size_t per_window = sizeof(cplx) * (4 * nw + (size_t)region * Nx + 2 * (size_t)region * Ny + (size_t)region * region);
    long cap = max_batch > 0 ? max_batch : (long)(WINDOW_BATCH_BYTES / per_window);
    if (cap < 1) cap = 1;
    if (cap > WINDOW_BATCH_MAX) cap = WINDOW_BATCH_MAX;
    const int nbmax = n < cap ? n : (int)cap;
    WsGuard ws;
    cplx *A = ws.get<cplx>(nbmax * nw), *B = ws.get<cplx>(nbmax * nw), *T1 = ws.get<cplx>(nbmax * nw), *T2 = ws.get<cplx>(nbmax * nw);
    unsigned long long *best = ws.get<unsigned long long>(4 * (size_t)nbmax);   // coarse value, fine value | coarse index, fine index
    int *org = ws.get<int>(4 * (size_t)n);
    if (!A || !B || !T1 || !T2 || !best || !org) return TIP_ERR_NOMEM;
    cplx *Kx = nullptr, *Ky = nullptr, *C1 = nullptr, *O = nullptr;
    if (region) {
        Kx = ws.get<cplx>((size_t)nbmax * region * Nx); Ky = ws.get<cplx>((size_t)nbmax * region * Ny);
        C1 = ws.get<cplx>((size_t)nbmax * region * Ny); O = ws.get<cplx>((size_t)nbmax * region * region);
        if (!Kx || !Ky || !C1 || !O) return TIP_ERR_NOMEM;
    }
    int rc;
    RowPlan plx, ply;                                                        // one plan per extent for the whole call
    if ((rc = make_plan(plx, Nx, ws)) || (rc = make_plan(ply, Ny, ws))) return rc;
    if (origins) TIP_HIP(hipMemcpyAsync(org, origins, 4 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, c.stream));
    else TIP_HIP(hipMemsetAsync(org, 0, 4 * (size_t)n * sizeof(int), c.stream));
    std::vector<unsigned long long> h(2 * (size_t)nbmax);
    const double uf = (double)upsample, dftshift = floor(region / 2.0);
    const long nr = (long)region * region;
    for (int w0 = 0; w0 < n; w0 += nbmax) {
        const int nb = n - w0 < nbmax ? n - w0 : nbmax;
        const long tot = (long)nb * (long)nw;
        unsigned long long *bv = best, *bi = best + 2 * (size_t)nbmax;       // [0, nb): coarse, [nbmax, nbmax + nb): fine
        for (int side = 0; side < 4; side += 2) {
            const void *src = side == 0 ? ref : mov;
            cplx *dst = side == 0 ? A : B;
            if (dtype == 0) rc = load_windows<float>(src, frame_x, org + 4 * w0, side, dst, nb, Ny, Nx);
            else if (dtype == 1) rc = load_windows<double>(src, frame_x, org + 4 * w0, side, dst, nb, Ny, Nx);
            else rc = load_windows<uint16_t>(src, frame_x, org + 4 * w0, side, dst, nb, Ny, Nx);
            if (rc) return rc;
        }
        if ((rc = fft2_windows(A, T1, nb, Ny, Nx, plx, ply, 0))) return rc;  // T1 = F1^T
        if ((rc = fft2_windows(B, T2, nb, Ny, Nx, plx, ply, 0))) return rc;  // T2 = F2^T
        cplx *PT = A;                                                        // P^T = F1^T * conj(F2^T), window after window
        TIP_LAUNCH("cmul_conj", k_cmul_conj, dim3(cdiv(tot, 256)), dim3(256), 0, (const cplx *)T1, (const cplx *)T2, PT, tot);
        // cross-correlation = ifft2(P): the inverse transform of P^T (Nx rows of Ny) lands untransposed (Ny rows of Nx) in T1
        TIP_HIP(hipMemcpyAsync(B, PT, tot * sizeof(cplx), hipMemcpyDeviceToDevice, c.stream));
        if ((rc = fft2_windows(B, T1, nb, Nx, Ny, ply, plx, 1))) return rc;
        TIP_HIP(hipMemsetAsync(bv, 0, 2 * (size_t)nbmax * 8, c.stream));
        TIP_HIP(hipMemsetAsync(bi, 0xff, 2 * (size_t)nbmax * 8, c.stream));
        TIP_LAUNCH("absargmax", k_absargmax, dim3(cdiv((long)nw, 256), nb), dim3(256), 0, (const cplx *)T1, (long)nw, bv, bi);
        TIP_LAUNCH("absargmax2", k_absargmax2, dim3(cdiv((long)nw, 256), nb), dim3(256), 0, (const cplx *)T1, (long)nw,
                   (const unsigned long long *)bv, bi);
        if (region) {
            TIP_LAUNCH("dft_kernel", k_dft_kernel_windows, dim3(cdiv((long)region * Nx, 256), nb), dim3(256), 0, Kx, region, Nx,
                       (const unsigned long long *)bi, Nx, 1, dftshift, uf);
            TIP_LAUNCH("dft_kernel", k_dft_kernel_windows, dim3(cdiv((long)region * Ny, 256), nb), dim3(256), 0, Ky, region, Ny,
                       (const unsigned long long *)bi, Nx, 0, dftshift, uf);
            TIP_LAUNCH("updft1", k_updft1, dim3(cdiv(Ny, 256), region, nb), dim3(256), 0, (const cplx *)Kx, (const cplx *)PT, C1, region, Nx,
                       Ny);
            TIP_LAUNCH("updft2", k_updft2, dim3(region, region, nb), dim3(64), 0, (const cplx *)Ky, (const cplx *)C1, O, region, Ny);
            TIP_LAUNCH("absargmax", k_absargmax, dim3(cdiv(nr, 256), nb), dim3(256), 0, (const cplx *)O, nr, bv + nbmax, bi + nbmax);
            TIP_LAUNCH("absargmax2", k_absargmax2, dim3(cdiv(nr, 256), nb), dim3(256), 0, (const cplx *)O, nr,
                       (const unsigned long long *)(bv + nbmax), bi + nbmax);
        }
        TIP_HIP(hipMemcpyAsync(h.data(), bi, 2 * (size_t)nbmax * 8, hipMemcpyDeviceToHost, c.stream));
        TIP_HIP(hipStreamSynchronize(c.stream));                             // the chunk's one wait
        for (int w = 0; w < nb; ++w) {
            int64_t *o = out4n_host + 4 * (size_t)(w0 + w);
            const long peak = (long)h[w];
            o[0] = peak / Nx; o[1] = peak % Nx; o[2] = 0; o[3] = 0;
            if (region) { o[2] = (int64_t)(h[nbmax + w] / region); o[3] = (int64_t)(h[nbmax + w] % region); }
        }
    }
    return TIP_OK;
}

// the whole plane: one window of the frame's extent at the origin
int phase_correlation_dev(const void *ref, const void *mov, int dtype, int Ny, int Nx, int upsample, int64_t *out4_host)
{
    return correlate_windows("phase_correlation", ref, mov, dtype, Ny, Nx, 1, nullptr, Ny, Nx, upsample, 0, out4_host);
}

int phase_correlation_windows_dev(const void *ref, const void *mov, int dtype, int frame_y, int frame_x, int n, const int32_t *origins,
                                  int Ny, int Nx, int upsample, int max_batch, int64_t *out4n_host)
{
    if (n == 0) return TIP_OK;
    if (!origins) return fail(TIP_ERR_ARG, "phase_correlation_windows: null pointer");      // (null is the whole plane's form)
    return correlate_windows("phase_correlation_windows", ref, mov, dtype, frame_y, frame_x, n, origins, Ny, Nx, upsample, max_batch,
                             out4n_host);
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_phase_correlation_dev(const void *ref, const void *mov, int dtype, int y, int x, int upsample, int64_t *out4_host)
{
    return phase_correlation_dev(ref, mov, dtype, y, x, upsample, out4_host);
}

int tip_phase_correlation_windows_dev(const void *ref, const void *mov, int dtype, int frame_y, int frame_x, int n, const int32_t *origins,
                                      int ny, int nx, int upsample, int max_batch, int64_t *out4n_host)
{
    return phase_correlation_windows_dev(ref, mov, dtype, frame_y, frame_x, n, origins, ny, nx, upsample, max_batch, out4n_host);
}

int tip_phase_correlation(const void *ref, const void *mov, int dtype, int y, int x, int upsample, int64_t *out4)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!ref || !mov || !out4 || y < 1 || x < 1) return fail(TIP_ERR_ARG, "tip_phase_correlation: bad arguments");
    const size_t es = dtype == 0 ? 4 : (dtype == 1 ? 8 : 2);
    const size_t bytes = (size_t)y * x * es;
    WsGuard ws;
    char *da = ws.get<char>(bytes), *db = ws.get<char>(bytes);
    if (!da || !db) return TIP_ERR_NOMEM;
    TIP_HIP(hipMemcpyAsync(da, ref, bytes, hipMemcpyHostToDevice, c.stream));
    TIP_HIP(hipMemcpyAsync(db, mov, bytes, hipMemcpyHostToDevice, c.stream));
    return phase_correlation_dev(da, db, dtype, y, x, upsample, out4);
}

// diagnostics (tests): the plan, row and transpose kernels the correlation runs, on one host complex128 array
int tip_fft2_c128(const double *in, double *out, int y, int x, int inverse)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !out) return fail(TIP_ERR_ARG, "tip_fft2_c128: null pointer");
    if (y < 2 || x < 2 || y > 4096 || x > 4096)
        return fail(TIP_ERR_UNSUPPORTED, "tip_fft2_c128: extents must lie in [2, 4096] (got %dx%d)", y, x);
    const long n = (long)y * x;
    WsGuard ws;
    cplx *A = ws.get<cplx>(n), *T = ws.get<cplx>(n);
    if (!A || !T) return TIP_ERR_NOMEM;
    int rc;
    RowPlan plx, ply;
    if ((rc = make_plan(plx, x, ws)) || (rc = make_plan(ply, y, ws))) return rc;
    TIP_HIP(hipMemcpyAsync(A, in, n * sizeof(cplx), hipMemcpyHostToDevice, c.stream));
    if ((rc = fft2_windows(A, T, 1, y, x, plx, ply, inverse ? 1 : 0))) return rc;            // T = the transform transposed
    TIP_LAUNCH("transpose_c", k_transpose_c, dim3(cdiv(y, 16), cdiv(x, 16)), dim3(256), 0, (const cplx *)T, A, x, y);
    TIP_HIP(hipMemcpyAsync(out, A, n * sizeof(cplx), hipMemcpyDeviceToHost, c.stream));
    TIP_HIP(hipStreamSynchronize(c.stream));
    return TIP_OK;
}

}  // extern "C"
