// The optimizer's kernels: fused Adam on the flat parameter buffer, sums of squares and the gradient-clipping
// coefficient, exact (ngp_sumsq*, ngp_clip_coef*) or settled from an upper bound of the gradient norm
// (ngp_row_norm_sum, ngp_clip_decide*).  Elementwise sweeps and reductions only: nothing here knows a GEMM tile.
#include "common.h"

namespace {

// One element's Adam update.  The three multiply-adds are fused by name and nothing else may be: left to the compiler, the
// quad loops and the tail of adam_kernel fused v * beta2 + (1 - beta2) g g each its own way, and the last bit of exp_avg_sq
// depended on which loop an element fell into, that is on n and on the launch width.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float gs, float step_size, float beta1,
                                            float beta2, float eps, float bc2_sqrt, float weight_decay)
{
#pragma clang fp contract(off)
    float gr = g * gs;
    if (weight_decay != 0.0f) gr = fmaf(weight_decay, p, gr);
    m = fmaf(gr - m, 1.0f - beta1, m);
    v = fmaf(v, beta2, (1.0f - beta2) * gr * gr);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = fmaf(-step_size, m / denom, p);
}

__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float step_size, float beta1, float beta2,
                                                   float eps, float bc2_sqrt, float weight_decay,
                                                   const float* __restrict__ grad_scale, int zero_grad, bool sparse_zero)
{
    constexpr int U = 2;   // 16-byte quads per lane and trip
    const float gs = grad_scale ? *grad_scale : 1.0f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p); float4* g4 = reinterpret_cast<float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m); float4* v4 = reinterpret_cast<float4*>(v);
    auto update = [&](float4& pp, const float4& gg, float4& mm, float4& vv) {
        float* pa = &pp.x; const float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x;
#pragma unroll
        for (int j = 0; j < 4; j++)
            adam_update(pa[j], ga[j], ma[j], va[j], gs, step_size, beta1, beta2, eps, bc2_sqrt, weight_decay);
    };
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    auto nz = [](const float4& q) { return q.x != 0.0f || q.y != 0.0f || q.z != 0.0f || q.w != 0.0f; };
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // U independent 16-B quads per lane and trip: the launch is capped well below full occupancy
    // (other streams' kernels must be able to get wave slots and registers), so the bytes in flight come from
    // the unroll instead of from more waves
    for (; i + (U - 1) * stride < n4; i += U * stride) {
        float4 pa[U], ga[U], ma[U], va[U];
#pragma unroll
        for (int u = 0; u < U; u++) { pa[u] = p4[i + u * stride]; ga[u] = g4[i + u * stride]; ma[u] = m4[i + u * stride]; va[u] = v4[i + u * stride]; }
#pragma unroll
        for (int u = 0; u < U; u++) {
            update(pa[u], ga[u], ma[u], va[u]);
            p4[i + u * stride] = pa[u]; m4[i + u * stride] = ma[u]; v4[i + u * stride] = va[u];
            // untouched table rows (no sample near them this step) already hold zeros: do not write them again
            if (zero_grad && (sparse_zero ? nz(ga[u]) : true)) g4[i + u * stride] = zero4;
        }
    }
    for (; i < n4; i += stride) {
        float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
        update(pp, gg, mm, vv);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if (zero_grad && (sparse_zero ? nz(gg) : true)) g4[i] = zero4;
    }
    // tail
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_update(pp, g[i], mm, vv, gs, step_size, beta1, beta2, eps, bc2_sqrt, weight_decay);
        m[i] = mm; v[i] = vv; p[i] = pp;
        if (zero_grad) g[i] = 0.0f;
    }
}

__global__ void __launch_bounds__(256) sumsq_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out,
                                                    const int32_t* __restrict__ flag)
{
    if (flag && *flag == 0) return;   // the clip decision did not need the exact norm

    __shared__ float part[4];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float a = 0.0f, b = 0.0f;
    // 16-byte loads, two independent quads per trip (x is 16-byte aligned: checked by the caller)
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const int64_t n4 = n >> 2;
    int64_t i = tid;
    for (; i + stride < n4; i += 2 * stride) {
        const float4 p = x4[i], q = x4[i + stride];
        a = fmaf(p.x, p.x, a); a = fmaf(p.y, p.y, a); a = fmaf(p.z, p.z, a); a = fmaf(p.w, p.w, a);
        b = fmaf(q.x, q.x, b); b = fmaf(q.y, q.y, b); b = fmaf(q.z, q.z, b); b = fmaf(q.w, q.w, b);
    }
    for (; i < n4; i += stride) {
        const float4 p = x4[i];
        a = fmaf(p.x, p.x, a); a = fmaf(p.y, p.y, a); a = fmaf(p.z, p.z, a); a = fmaf(p.w, p.w, a);
    }
    for (int64_t j = (n4 << 2) + tid; j < n; j += stride) a = fmaf(x[j], x[j], a);
    a += b;
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}

__global__ void __launch_bounds__(256) sumsq_scalar_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out,
                                                           const int32_t* __restrict__ flag)
{
    if (flag && *flag == 0) return;

    __shared__ float part[4];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float a = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) a = fmaf(x[i], x[i], a);
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}

// coef = extra_scale * min(1, max_norm / (sqrt(sumsq) + 1e-6))   (torch.nn.utils.clip_grad_norm_)
__global__ void clip_coef_kernel(const float* __restrict__ sumsq, float max_norm, float extra_scale,
                                 float* __restrict__ coef)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float norm = sqrtf(*sumsq) * extra_scale;
        float c = max_norm / (norm + 1e-6f);
        if (c > 1.0f) c = 1.0f;
        *coef = c * extra_scale;
    }
}

// sum over rows of the Euclidean norm of the first `cols` entries (cols <= 16): one lane per row
__global__ void __launch_bounds__(256) row_norm_sum_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int cols,
                                                           float* __restrict__ out)
{
    __shared__ float part[4];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float a = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float q = 0.0f;
        for (int c = 0; c < cols; c++) { const float v = x[i * ldx + c]; q = fmaf(v, v, q); }
        a += sqrtf(q);
    }
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}

// clipping settled from an upper bound of the gradient norm (see ngp_clip_decide in the header)
// (sumsq_rest and sumsq_out are not __restrict__: ngp_clip_decide_rest passes one running sum as both)
__global__ void __launch_bounds__(1024) clip_decide_kernel(const float* __restrict__ sums,
                                                           const float* __restrict__ w1a, int64_t n1a,
                                                           const float* __restrict__ w2a, int64_t n2a,
                                                           const float* __restrict__ w1b, int64_t n1b,
                                                           const float* __restrict__ w2b, int64_t n2b,
                                                           const float* sumsq_rest, float max_norm,
                                                           float extra_scale, float* __restrict__ coef,
                                                           int32_t* __restrict__ need_exact,
                                                           const float* __restrict__ rest, int64_t n_rest,
                                                           float* sumsq_out)
{
    __shared__ float ws[5][16];
    const float* ptr[5] = {w1a, w2a, w1b, w2b, rest};
    const int64_t cnt[5] = {n1a, n2a, n1b, n2b, rest ? n_rest : 0};
    for (int k = 0; k < 5; k++) {
        float q = 0.0f;
        // 16-byte pieces, several in flight per thread (one block reads ~80 k floats: the loads' latency is the launch's length)
        const bool vec = (((uintptr_t)ptr[k]) & 15) == 0;
        const int64_t n4 = vec ? cnt[k] / 4 : 0;
        const float4* p4 = reinterpret_cast<const float4*>(ptr[k]);
        float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
#pragma unroll 4
        for (int64_t i = threadIdx.x; i < n4; i += 1024) {
            const float4 v = p4[i];
            q0 = fmaf(v.x, v.x, q0); q1 = fmaf(v.y, v.y, q1); q2 = fmaf(v.z, v.z, q2); q3 = fmaf(v.w, v.w, q3);
        }
        q = (q0 + q1) + (q2 + q3);
        for (int64_t i = 4 * n4 + threadIdx.x; i < cnt[k]; i += 1024) q = fmaf(ptr[k][i], ptr[k][i], q);
#pragma unroll   // wave_sum(q): the text the kernel's compiled shape was measured with
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        if ((threadIdx.x & 63) == 0) ws[k][threadIdx.x >> 6] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float f[4];
        for (int k = 0; k < 4; k++) {
            float t = 0.0f;
            for (int w = 0; w < 16; w++) t += ws[k][w];
            f[k] = sqrtf(t);
        }
        float rest_sq = sumsq_rest ? *sumsq_rest : 0.0f;
        if (rest) {                       // the exact part summed here (ngp_clip_decide_rest): no launch of its own
            for (int w = 0; w < 16; w++) rest_sq += ws[4][w];
            *sumsq_out = rest_sq;         // the conditional exact route (ngp_sumsq_if) continues from it
        }
        const float ba = f[0] * f[1] * sums[0], bb = f[2] * f[3] * sums[1];
        const float bound = sqrtf(ba * ba + bb * bb + rest_sq) * extra_scale;
        const bool safe = bound * 1.001f + 1e-6f < max_norm;     // false for NaN / inf
        *need_exact = safe ? 0 : 1;
        if (safe) *coef = extra_scale;
    }
}

__global__ void clip_coef_if_kernel(const float* __restrict__ sumsq, float max_norm, float extra_scale,
                                    float* __restrict__ coef, const int32_t* __restrict__ flag)
{
    if (threadIdx.x == 0 && blockIdx.x == 0 && *flag != 0) {
        const float norm = sqrtf(*sumsq) * extra_scale;
        float c = max_norm / (norm + 1e-6f);
        if (c > 1.0f) c = 1.0f;
        *coef = c * extra_scale;
    }
}

} // namespace


extern "C" {

int ngp_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int64_t step, const float* grad_scale, int zero_grad,
                  void* stream)
{
    return ngp_adam_step_width(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                               zero_grad, 0, stream);
}

int ngp_adam_step_width(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int64_t step, const float* grad_scale, int zero_grad,
                        int workgroups, void* stream)
{
    if (n < 0 || step < 1 || workgroups < 0) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq) return NGP_EINVAL;
    if (!aligned16(param) || !aligned16(grad) || !aligned16(exp_avg) || !aligned16(exp_avg_sq)) return NGP_EINVAL;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    // Default 2 workgroups per CU (a wave per SIMD each, 64 registers): 5.2 TB/s alone (2048 workgroups: 4.5) and the sweep ends
    // soonest.  ONE workgroup per CU lets the 8-wave MLP workgroups of the next step's density path in beside it (the sweep then
    // takes 1.5-1.7 instead of 1.1-1.4 ms, the colour chain follows alone).  Which is faster per step depends on the loop and
    // the box (+-3 %: profiles/r03_occupancy_shaping.txt (1), (9)), so the caller may name the width:
    // NGPTrainer times both in its own loop and keeps the faster one.
    const int64_t cap = workgroups > 0 ? workgroups : 512;
    int64_t blocks = ((n >> 2) + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, n, step_size, beta1, beta2, eps, bc2_sqrt, weight_decay, grad_scale, zero_grad, true);
    return ngp_check_launch();
}

int ngp_sumsq(const float* x, int64_t n, float* out, void* stream)
{
    return ngp_sumsq_if(x, n, out, nullptr, stream);
}

int ngp_sumsq_if(const float* x, int64_t n, float* out, const int32_t* flag, void* stream)
{
    if (n < 0 || !out) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!x) return NGP_EINVAL;
    if (aligned16(x)) {
        int64_t blocks = ((n >> 2) + 255) / 256;
        if (blocks < 1) blocks = 1;
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, out, flag);
    } else {
        int64_t blocks = (n + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(sumsq_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, out, flag);
    }
    return ngp_check_launch();
}

int ngp_clip_coef(const float* sumsq, float max_norm, float extra_scale, float* coef, void* stream)
{
    if (!sumsq || !coef) return NGP_EINVAL;
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sumsq, max_norm, extra_scale, coef);
    return ngp_check_launch();
}

int ngp_row_norm_sum(const float* x, int64_t ldx, int64_t n, int cols, float* out, void* stream)
{
    if (n < 0 || cols < 1 || cols > 16 || ldx < cols || !out) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!x) return NGP_EINVAL;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 512) blocks = 512;
    hipLaunchKernelGGL(row_norm_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, n, cols, out);
    return ngp_check_launch();
}

int ngp_clip_decide(const float* row_norm_sums, const float* w1_a, int64_t n1_a, const float* w2_a, int64_t n2_a,
                    const float* w1_b, int64_t n1_b, const float* w2_b, int64_t n2_b, const float* sumsq_rest,
                    float max_norm, float extra_scale, float* coef, int32_t* need_exact, void* stream)
{
    if (!row_norm_sums || !w1_a || !w2_a || !w1_b || !w2_b || n1_a < 1 || n2_a < 1 || n1_b < 1 || n2_b < 1 || !coef ||
        !need_exact)
        return NGP_EINVAL;
    hipLaunchKernelGGL(clip_decide_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_norm_sums, w1_a, n1_a, w2_a,
                       n2_a, w1_b, n1_b, w2_b, n2_b, sumsq_rest, max_norm, extra_scale, coef, need_exact,
                       (const float*)nullptr, (int64_t)0, (float*)nullptr);
    return ngp_check_launch();
}

int ngp_clip_decide_rest(const float* row_norm_sums, const float* w1_a, int64_t n1_a, const float* w2_a, int64_t n2_a,
                         const float* w1_b, int64_t n1_b, const float* w2_b, int64_t n2_b, const float* rest,
                         int64_t n_rest, float* sumsq, float max_norm, float extra_scale, float* coef,
                         int32_t* need_exact, void* stream)
{
    if (!row_norm_sums || !w1_a || !w2_a || !w1_b || !w2_b || n1_a < 1 || n2_a < 1 || n1_b < 1 || n2_b < 1 || !coef ||
        !need_exact || !rest || n_rest < 0 || !sumsq)
        return NGP_EINVAL;
    hipLaunchKernelGGL(clip_decide_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_norm_sums, w1_a, n1_a, w2_a,
                       n2_a, w1_b, n1_b, w2_b, n2_b, (const float*)sumsq, max_norm, extra_scale, coef, need_exact, rest,
                       n_rest, sumsq);
    return ngp_check_launch();
}

int ngp_clip_coef_if(const float* sumsq, float max_norm, float extra_scale, float* coef, const int32_t* flag,
                     void* stream)
{
    if (!sumsq || !coef || !flag) return NGP_EINVAL;
    hipLaunchKernelGGL(clip_coef_if_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sumsq, max_norm, extra_scale,
                       coef, flag);
    return ngp_check_launch();
}

} // extern "C"
