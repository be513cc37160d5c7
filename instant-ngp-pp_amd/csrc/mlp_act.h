// Activation functions of the MLP kernels, shared with the fused density-field kernel (grid_kernels.hip), which
// has to round exactly as the standalone MLP kernels do.
#pragma once
#include "common.h"

namespace {

// softplus(v) = log(1+e^v) with the hardware exp/log (v_exp_f32 / v_log_f32, ~1e-6 relative):
// v > 20 -> v (torch's threshold); v < -15 -> e^v (1+e^v would round to 1); else log(1+e^v).
__device__ __forceinline__ float softplus_fast(float v)
{
    // raw v_exp_f32 / v_log_f32 (base 2): __expf / __logf wrap them in denormal-range scaling (compare, select, ldexp: ~8 more
    // vector instructions per element) that a softplus never needs — below v = -87 the result is < 1e-38 either way
    const float e = __builtin_amdgcn_exp2f(v * 1.4426950408889634f);
    float l = 0.6931471805599453f * __builtin_amdgcn_logf(1.0f + e);
    // the logarithm is computed unconditionally and SELECTED: left inside the conditional, hipcc wraps every element of an
    // epilogue tile in its own exec-mask branch (64 s_and_saveexec / s_cbranch / s_or per tile and wave, with their s_nop padding)
    asm volatile("" : "+v"(l));
    const float r = v < -15.0f ? e : l;
    return v > 20.0f ? v : r;
}

__device__ __forceinline__ float act_fwd(float v, int act)
{
    switch (act) {
        case NGP_ACT_RELU: return v > 0.0f ? v : 0.0f;
        case NGP_ACT_SIGMOID: return 1.0f / (1.0f + __expf(-v));
        case NGP_ACT_SOFTPLUS: return softplus_fast(v);
        case NGP_ACT_EXP: return __expf(v);
        default: return v;
    }
}

// derivative of an activation expressed through its OUTPUT y, for a unit upstream gradient (bitwise what act_bwd_kernel writes)
__device__ __forceinline__ float act_dout(float y, int act)
{
    switch (act) {
        case NGP_ACT_RELU: return y > 0.0f ? 1.0f : 0.0f;
        case NGP_ACT_SIGMOID: return y * (1.0f - y);
        case NGP_ACT_SOFTPLUS: return -expm1f(-y);
        case NGP_ACT_EXP: return y;
        default: return 1.0f;
    }
}

__device__ __forceinline__ float act_grad_from_output(float y, int act)
{
    switch (act) {
        case NGP_ACT_RELU: return y > 0.0f ? 1.0f : 0.0f;
        case NGP_ACT_SIGMOID: return y * (1.0f - y);
        case NGP_ACT_SOFTPLUS: return -expm1f(-y);
        case NGP_ACT_EXP: return y;
        default: return 1.0f;
    }
}

// derivative through the OUTPUT for the two hidden activations of the model, cheap enough for the
// staging path of a GEMM (softplus' = 1 - exp(-y), v_exp_f32)
__device__ __forceinline__ float act_grad_fast(float y, int act)
{
    if (act == NGP_ACT_SOFTPLUS) { // 1 - exp(-y) cancels for tiny y: two Taylor terms there (relative error < 2e-7)
        // raw v_exp_f32 (base 2): y >= 0, so exp(-y) never needs __expf's denormal-range scaling (~5 more instructions)
        const float e = __builtin_amdgcn_exp2f(y * -1.4426950408889634f), t = y * (1.0f - 0.5f * y);   // both sides evaluated: a select, not a branch
        return y < 1e-3f ? t : 1.0f - e;
    }
    return act == NGP_ACT_RELU ? (y > 0.0f ? 1.0f : 0.0f) : act_grad_from_output(y, act);
}

}  // namespace
