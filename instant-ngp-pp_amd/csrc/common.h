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
__device__ __forceinline__ float half_sum(float v)
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
