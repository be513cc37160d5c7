// Shared device/host helpers for libngp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ngp_hip.h"

#define NGP_WAVE 64
#define NGP_HALF 32

static inline int ngp_check_launch()
{
    return hipGetLastError() == hipSuccess ? NGP_OK : NGP_ELAUNCH;
}

static inline unsigned ngp_blocks(int64_t work, int per_block)
{
    int64_t b = (work + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b);
}

// workgroups of a grid-stride launch over n items: one per tile of `tile` items, at most max_blocks
static inline int64_t ngp_capped_tiles(int64_t n, int tile, int max_blocks)
{
    const int64_t n_tiles = (n + tile - 1) / tile;
    return n_tiles < max_blocks ? n_tiles : max_blocks;
}

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// ---- host state that belongs to a device, not to the process ------------------------------
// Slot of the CURRENT device in a small per-device cache, or -1 (runtime error, or an ordinal beyond the cache: the
// callers then look the fact up again on every call, which is slower and still right).
constexpr int NGP_MAX_DEVICES = 64;

static inline int ngp_device_slot()
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    return dev >= 0 && dev < NGP_MAX_DEVICES ? dev : -1;
}

// compute units of the current device (the streaming kernels launch one workgroup per CU); 0: the runtime cannot say
inline int cu_count()
{
    static int cached[NGP_MAX_DEVICES] = {};
    const int slot = ngp_device_slot();
    if (slot >= 0 && cached[slot]) return cached[slot];
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    if (n <= 0) n = 256;
    if (slot >= 0) cached[slot] = n;
    return n;
}

// Launch of a kernel that needs more dynamic LDS than the 64 KiB a kernel gets by default.  hipFuncSetAttribute lifts
// the limit to max_lds bytes; the runtime resolves the host function to the current device's code object, so the
// "already set" flag is kept per kernel instantiation AND device.
template <auto Kernel, typename... Args>
int launch_big_lds(dim3 grid, dim3 block, size_t lds, int max_lds, hipStream_t stream, Args... args)
{
    static bool attr_set[NGP_MAX_DEVICES] = {};
    const int slot = ngp_device_slot();
    if (slot < 0 || !attr_set[slot]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                max_lds) != hipSuccess)
            return NGP_ELAUNCH;
        if (slot >= 0) attr_set[slot] = true;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    return ngp_check_launch();
}

// ---- cross-lane helpers over a 32-lane half-wave (one ray segment per half) ----------
// __shfl_* with width=32 never crosses the half-wave boundary.
template <typename T>   // float or double
__device__ __forceinline__ T half_sum(T v)
{
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
    return v;
}

__device__ __forceinline__ float half_incl_scan_add(float v, int lane32)
{
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        float u = __shfl_up(v, o, 32);
        if (lane32 >= o) v += u;
    }
    return v;
}

__device__ __forceinline__ float half_incl_scan_mul(float v, int lane32)
{
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        float u = __shfl_up(v, o, 32);
        if (lane32 >= o) v *= u;
    }
    return v;
}

// first set bit (0-based) of this half-wave's 32-bit slice of a 64-bit ballot, or -1
__device__ __forceinline__ int half_first(unsigned long long ballot, int lane64)
{
    unsigned m = (unsigned)(ballot >> (lane64 & 32));
    return m ? (__ffs((int)m) - 1) : -1;
}

// ---- cross-lane helpers over the whole 64-lane wave -------------------------------------------
// Sum of the wave on every lane (int, float or double).  The xor butterfly runs 32 -> 1: that order is part of every
// float and double result built on it.
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < NGP_WAVE; o <<= 1) {
        const int u = __shfl_up(v, o, NGP_WAVE);
        if (lane >= o) v += u;
    }
    return v;
}

// ---- scans over a workgroup -------------------------------------------------------------------
// Exclusive scan of v over a workgroup of THREADS lanes (every lane calls it); *total, if asked for, is the workgroup's
// sum on every lane.  The wave totals pass through LDS that the function owns, behind ONE barrier: lanes may still be
// reading it when the function returns, so a second call in the same kernel needs a __syncthreads() between the two
// (block_carry_scan ends every tile with one).
template <int THREADS>
__device__ __forceinline__ int block_excl_scan(int v, int* total = nullptr)
{
    static_assert(THREADS % NGP_WAVE == 0, "whole waves");
    __shared__ int wsum[THREADS / NGP_WAVE];
    const int lane = threadIdx.x & (NGP_WAVE - 1), wave = threadIdx.x / NGP_WAVE;
    const int inc = wave_incl_scan(v, lane);
    if (lane == NGP_WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    int off = inc - v;
    for (int w = 0; w < wave; w++) off += wsum[w];
    if (total) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < THREADS / NGP_WAVE; w++) tot += wsum[w];
        *total = tot;
    }
    return off;
}

// ONE workgroup of THREADS lanes scans n values tile by tile: store(i, sum of load(0) .. load(i - 1)) for every i < n,
// and the sum of all n comes back on every lane.  A tile's values and their sum are int32; the running carry is a
// Carry, int64_t where the total may pass 2^31.
template <int THREADS, typename Carry, typename Load, typename Store>
__device__ __forceinline__ Carry block_carry_scan(int n, Load load, Store store)
{
    Carry carry = 0;
    for (int base = 0; base < n; base += THREADS) {
        const int i = base + threadIdx.x;
        int tot;
        const int off = block_excl_scan<THREADS>(i < n ? load(i) : 0, &tot);
        if (i < n) store(i, carry + off);
        carry += tot;
        __syncthreads();   // the next tile reuses block_excl_scan's LDS
    }
    return carry;
}

// Sum of element e of n_blocks rows of `stride` doubles (the per-workgroup partial sums of a backward), in row order:
// two accumulators over the even and the odd rows, rounded ONCE, where the sum meets its float32 sink.  No atomics: the
// same bits on every run.
__device__ __forceinline__ float ordered_partial_sum(const double* __restrict__ partials, int n_blocks, int stride, int e)
{
    double s0 = 0.0, s1 = 0.0;
    int b = 0;
    for (; b + 1 < n_blocks; b += 2) {
        s0 += partials[(size_t)b * stride + e];
        s1 += partials[(size_t)(b + 1) * stride + e];
    }
    if (b < n_blocks) s0 += partials[(size_t)b * stride + e];
    return (float)(s0 + s1);
}
