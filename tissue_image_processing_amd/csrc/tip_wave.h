// tip_wave.h -- the wave and workgroup primitives of the device code (included by tip_internal.h): one reduction, one scan,
// one lane combine.  Stateless templates for the 64-lane wave of gfx950, called by whole wavefronts of a 1-D workgroup
// (lane = threadIdx.x & 63, wave = threadIdx.x >> 6); the block forms need every thread of the workgroup at the call.
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <type_traits>

namespace tip {

// Called by whole wavefronts of a 1-D workgroup: f(key, count) runs once for every distinct key among the active lanes, on the
// first lane that holds it, with the number of lanes that do -- so a wave pays one atomic or one store per key, not per lane.
template <typename Key, typename F>
__device__ __forceinline__ void wave_combine(bool active, Key key, F f)
{
    unsigned long long todo = __ballot(active);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const Key lk = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(active && key == lk) & todo;
        if (lane == leader) f(lk, __popcll(same));
        todo &= ~same;
    }
}

// the value of lane (own lane ^ d); a small struct (a key pair under one comparison) travels dword by dword
template <typename T>
__device__ __forceinline__ T lane_xor(T v, int d)
{
    if constexpr (std::is_arithmetic<T>::value) {
        return __shfl_xor(v, d, 64);
    } else {
        static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "lane_xor: dwords only");
        int w[sizeof(T) / 4];
        memcpy(w, &v, sizeof(T));
#pragma unroll
        for (unsigned k = 0; k < sizeof(T) / 4; ++k) w[k] = __shfl_xor(w[k], d, 64);
        memcpy(&v, w, sizeof(T));
        return v;
    }
}

// Butterfly reduction over the 64 lanes: v = op(v, value of lane ^ d) for d = 32, 16, 8, 4, 2, 1; every lane ends with the
// result.  The order is part of the contract: a lane's own partial result is op's first argument, and after step d it holds
// the op over the 64 / d lanes that are multiples of d away, so the result is ((v0 + v32) + (v16 + v48)) + ... on lane 0.
// With a commutative op (floating-point + is one: a + b and b + a are the same bits) every lane ends with the bits of lane 0,
// and those are the bits a shuffle-down tree with the same steps leaves on lane 0.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
    for (int d = 32; d >= 1; d >>= 1) v = op(v, lane_xor(v, d));
    return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, [](T a, T b) { return b < a ? b : a; }); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T a, T b) { return b > a ? b : a; }); }

// inclusive prefix sum over the 64 lanes of a wave: lane l returns v(0) + ... + v(l)
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// Exclusive prefix sum over a workgroup of WAVES waves: returns v(0) + ... + v(threadIdx.x - 1) and leaves the workgroup's sum
// in total (on every thread).  wave_sums is LDS, T[WAVES]; there is ONE barrier inside, between the write of the wave totals and
// their reads -- so wave_sums must not be written again (a second call, a loop's next trip) before another barrier, which is
// the caller's.  Up to four wave totals every thread adds up itself (broadcast reads); more of them every wave scans once more
// with its lanes, which keeps sixteen totals out of the registers.
template <int WAVES, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *wave_sums, T &total)
{
    static_assert(WAVES >= 1 && WAVES <= 64, "block_exclusive_scan: one lane per wave total");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive_scan(v);
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    T before = incl - v;
    if constexpr (WAVES <= 4) {
        total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) before += wave_sums[w];
            total += wave_sums[w];
        }
    } else {
        const T s = lane < WAVES ? wave_sums[lane] : (T)0;
        const T upto = wave_inclusive_scan(s);
        before += __shfl(upto - s, wave, 64);
        total = __shfl(upto, WAVES - 1, 64);
    }
    return before;
}

// Reduction over a workgroup of WAVES waves: a wave_reduce, lane 0 of every wave to wave_vals (LDS, T[WAVES]), one barrier, and
// every thread folds the wave results in wave order, ((w0 op w1) op w2) op ...  The same rule as above: wave_vals must not be
// written again before another barrier.
template <int WAVES, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T *wave_vals, Op op)
{
    v = wave_reduce(v, op);
    if ((threadIdx.x & 63) == 0) wave_vals[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = wave_vals[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = op(r, wave_vals[w]);
    return r;
}
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T *wave_vals) { return block_reduce<WAVES>(v, wave_vals, [](T a, T b) { return a + b; }); }

// The tile scan of the device-wide int32 scans (256 threads, 8 consecutive items each): out[base + i] = the sum of the tile's
// items in front of base + i for base + i < n, where base is this thread's first item; returns the tile's sum (on every thread).
constexpr int SCAN_ITEMS = 8, SCAN_THREADS = 256, SCAN_BLOCK = SCAN_ITEMS * SCAN_THREADS;
__device__ __forceinline__ int scan_tile_i32(const int *__restrict__ in, int *__restrict__ out, long base, long n, int *wave_sums)
{
    int v[SCAN_ITEMS], s = 0, total;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        v[i] = base + i < n ? in[base + i] : 0;
        s += v[i];
    }
    int run = block_exclusive_scan<SCAN_THREADS / 64>(s, wave_sums, total);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    return total;
}

}  // namespace tip
