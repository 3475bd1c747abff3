// tip_transpose.hip -- out[c][r] = in[r][c] for a plane of 4- or 8-byte elements on device buffers, asynchronous on the calling
// thread's stream: SegmentationPredictor.predict works on the transposed image and returns its int32 labels and float64 HC map
// as (X, Y) for a (C, Y, X) image (pl.py:102, 194); a caller that keeps them on the device turns them back with this entry
// instead of a host `.T`.  (FramePipeline.segment_unet hands predict the transposed planes, so ITS results need no transpose.)
//
//   one workgroup (4 waves, 64 x 4 threads) per 64 x 64 tile: a wave loads one tile row -- 64 consecutive elements, 256 or
//   512 contiguous bytes -- into LDS, and after the barrier stores one row of the TRANSPOSED tile, again 64 consecutive
//   elements: both global directions are coalesced along the fast axis.
//   LDS row stride 65 elements.  The transposed read walks a tile column: lane l reads element 65 l + k.  4-byte elements
//   (ds_read_b32, bank = dword mod 32, lanes conflict within a 32-lane half): dword 65 l -> bank l mod 32, all distinct.  8-byte
//   elements (ds_read_b64, bank = dword mod 64, two banks per lane): dwords 130 l, 130 l + 1 -> banks 2 l, 2 l + 1 mod 64, all
//   distinct within a half.  The row-wise writes are contiguous.  33 KiB of LDS at 8 bytes: four workgroups per CU.
//   A bit copy through unsigned integers: no arithmetic touches the values (NaN payloads, -0.0).
#include "tip_internal.h"

namespace tip {

constexpr int TR_TILE = 64, TR_ROWS = 4, TR_LD = TR_TILE + 1;

template <typename T>
__global__ __launch_bounds__(TR_TILE * TR_ROWS) void transpose2d_kernel(const T *__restrict__ in, T *__restrict__ out, int rows,
                                                                        int cols, long tiles_x, long tiles)
{
    __shared__ T tile[TR_TILE * TR_LD];
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long r0 = (t / tiles_x) * TR_TILE, c0 = (t % tiles_x) * TR_TILE;
        if (r0 + TR_TILE <= rows && c0 + TR_TILE <= cols) {      // interior tile: a thread's 16 loads are in flight together
            T v[TR_TILE / TR_ROWS];
#pragma unroll
            for (int k = 0; k < TR_TILE / TR_ROWS; ++k) v[k] = in[(r0 + ty + k * TR_ROWS) * (long)cols + c0 + tx];
#pragma unroll
            for (int k = 0; k < TR_TILE / TR_ROWS; ++k) tile[(ty + k * TR_ROWS) * TR_LD + tx] = v[k];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < TR_TILE / TR_ROWS; ++k) v[k] = tile[tx * TR_LD + ty + k * TR_ROWS];
#pragma unroll
            for (int k = 0; k < TR_TILE / TR_ROWS; ++k) out[(c0 + ty + k * TR_ROWS) * (long)rows + r0 + tx] = v[k];
        } else {                                                  // edge tile: every access guarded
            if (c0 + tx < cols)
                for (int j = ty; j < TR_TILE; j += TR_ROWS)
                    if (r0 + j < rows) tile[j * TR_LD + tx] = in[(r0 + j) * (long)cols + c0 + tx];
            __syncthreads();
            if (r0 + tx < rows)
                for (int j = ty; j < TR_TILE; j += TR_ROWS)
                    if (c0 + j < cols) out[(c0 + j) * (long)rows + r0 + tx] = tile[tx * TR_LD + j];
        }
        __syncthreads();      // (the next tile of this workgroup overwrites the LDS tile)
    }
}

template <typename T> static int transpose2d_dev(const void *in, void *out, int rows, int cols, const char *name)
{
    const long tiles_x = cdiv(cols, TR_TILE), tiles = tiles_x * cdiv(rows, TR_TILE);
    const int grid = (int)(tiles < (1L << 20) ? tiles : (1L << 20));
    TIP_LAUNCH(name, transpose2d_kernel<T>, dim3(grid), dim3(TR_TILE, TR_ROWS), 0, (const T *)in, (T *)out, rows, cols, tiles_x,
               tiles);
    return TIP_OK;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_transpose2d_dev(const void *in, void *out, int rows, int cols, int elem_bytes)
{
    Ctx &c = ctx();
    if (!c.stream) return TIP_ERR_HIP;
    if (!in || !out) return fail(TIP_ERR_ARG, "tip_transpose2d_dev: null pointer");
    if (in == out) return fail(TIP_ERR_ARG, "tip_transpose2d_dev: in and out are the same buffer (the transpose is not in place)");
    if (rows < 1 || cols < 1) return fail(TIP_ERR_ARG, "tip_transpose2d_dev: extents %d x %d (each must be >= 1)", rows, cols);
    if (elem_bytes == 4) return transpose2d_dev<uint32_t>(in, out, rows, cols, "transpose2d_b4");
    if (elem_bytes == 8) return transpose2d_dev<uint64_t>(in, out, rows, cols, "transpose2d_b8");
    return fail(TIP_ERR_ARG, "tip_transpose2d_dev: elem_bytes %d (4 or 8)", elem_bytes);
}

}  // extern "C"
