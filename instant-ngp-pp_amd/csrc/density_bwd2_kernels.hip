// Second-order backward of the density head (128 -> 128 softplus -> 1 softplus), the element-wise pass between the
// products: what a gradient v on d(sigma)/dx leaves for the head once ngp_grid_bwd_bwd_input has turned v into
// u = dL/d(dfeat) and ngp_linear_fwd has formed r = u W1^T (include/ngp_hip.h, D2, has the algebra).
//
// Work decomposition: a workgroup of 256 lanes takes tiles of DH_ROWS = 8 rows with a grid stride; a 32-lane half-wave is
// one row, a lane holds four neighbouring hidden units of it (one 16-byte load of a1 and of r, one 16-byte store of m and
// of e1: the pass moves 2 KB a row and is bound by that).  The row's q = sum_h r_h w2_h s1_h is a butterfly over the
// half-wave in double: every lane ends with the same bits.  A lane owns the same four columns in every tile, so its four
// dW2 sums (and lane 0's db2 sum) stay in registers, as doubles, ACROSS the workgroup's tiles; at the end the eight
// half-waves are added through LDS in slot order and the workgroup stores its 129 sums (plain vector stores) to the
// caller's workspace, where a second launch adds them over the workgroups in launch-index order into the float32 sinks:
// no float atomics, the same bits on every run (ngp_tonemap_bwd's and ngp_skybox_bwd's scheme).
//
// Near saturation: s = 1 - exp(-y) is -expm1f(-y) (y = 1e-6 keeps its digits, where 1 - expf(-y) has one), and 1 - s is
// expf(-y) itself, never 1 - s of a rounded s (at y = 30 that difference is 0 while exp(-y) = 9.4e-14): s (1 - s), which
// is all of q's share of e2 on a saturated row, comes out with float32's full relative precision at both ends.  The
// tone-mapper's y (1 - y) lost exactly that (tonemap_kernels.hip).  Products of two rounded float32 factors and every
// sum are formed in double and rounded once where they meet their float32 outputs.
#include "common.h"
#include "mlp_act.h"

namespace {

constexpr int DH_H = 128;                          // hidden width
constexpr int DH_ROWS = NGP_DENSITY_BWD2_ROWS;     // rows per tile: one per half-wave
constexpr int DH_THREADS = 32 * DH_ROWS;
constexpr int DH_SUMS = DH_H + 1;                  // dW2 (128) | db2

// e1 may be r itself: a lane reads its four values of r before it writes its four of e1, and no other lane touches them
__global__ void __launch_bounds__(DH_THREADS) density_head_bwd2_kernel(const float* __restrict__ a1, const float* __restrict__ sig,
                                                                       const float* r, const float* __restrict__ W2,
                                                                       const float* __restrict__ d_sig, int64_t n, int64_t n_tiles,
                                                                       float* __restrict__ m, float* e1,
                                                                       double* __restrict__ partials)
{
    __shared__ double red[DH_ROWS][DH_SUMS + 3];
    const int lane = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const int h0 = 4 * lane;
    const float w[4] = {W2[h0], W2[h0 + 1], W2[h0 + 2], W2[h0 + 3]};
    double acc_w[4] = {0.0, 0.0, 0.0, 0.0}, acc_b = 0.0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row = tile * DH_ROWS + slot;
        const bool live = row < n;      // (the same for the 32 lanes of a row; the butterfly below runs on every lane)
        float4 av = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rv = av;
        float sg = 0.0f, gs = 0.0f;
        if (live) {
            av = *reinterpret_cast<const float4*>(a1 + row * DH_H + h0);
            rv = *reinterpret_cast<const float4*>(r + row * DH_H + h0);
            sg = sig[row];
            if (d_sig) gs = d_sig[row];
        }
        const float a[4] = {av.x, av.y, av.z, av.w}, rr[4] = {rv.x, rv.y, rv.z, rv.w};
        double s1[4], o1[4], ws1[4], qp = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            s1[k] = (double)-expm1f(-a[k]);      // sigmoid(z1) = 1 - exp(-a1)
            o1[k] = (double)expf(-a[k]);         // 1 - sigmoid(z1)
            ws1[k] = (double)w[k] * s1[k];
            qp = fma((double)rr[k], ws1[k], qp);
        }
        const double q = half_sum(qp);
        const double s2 = (double)-expm1f(-sg), o2 = (double)expf(-sg);
        const double e2 = q * (s2 * o2) + (double)gs * s2;
        if (live) {
            float mo[4], eo[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double rs2 = (double)rr[k] * s2;
                mo[k] = (float)(s2 * ws1[k]);
                eo[k] = (float)(ws1[k] * (e2 + rs2 * o1[k]));
                acc_w[k] += e2 * (double)a[k] + rs2 * s1[k];
            }
            *reinterpret_cast<float4*>(m + row * DH_H + h0) = make_float4(mo[0], mo[1], mo[2], mo[3]);
            *reinterpret_cast<float4*>(e1 + row * DH_H + h0) = make_float4(eo[0], eo[1], eo[2], eo[3]);
            if (lane == 0) acc_b += e2;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) red[slot][h0 + k] = acc_w[k];
    if (lane == 0) red[slot][DH_H] = acc_b;
    __syncthreads();
    if (threadIdx.x < DH_SUMS) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < DH_ROWS; k++) s += red[k][threadIdx.x];
        partials[(size_t)blockIdx.x * DH_SUMS + threadIdx.x] = s;
    }
}

// lane e = one of a workgroup's 129 sums: adds it over the workgroups in launch-index order, rounds once, adds to the sink
__global__ void __launch_bounds__(DH_THREADS) density_head_bwd2_sum_kernel(const double* __restrict__ partials, int n_blocks,
                                                                           float* __restrict__ dW2, float* __restrict__ db2)
{
    const int e = threadIdx.x;
    if (e >= DH_SUMS) return;
    const float s = ordered_partial_sum(partials, n_blocks, DH_SUMS, e);
    if (e < DH_H) dW2[e] += s;
    else db2[0] += s;
}

} // namespace

extern "C" {

int64_t ngp_density_head_bwd2_workspace(int64_t n)
{
    if (n < 0) return NGP_EINVAL;
    return ngp_capped_tiles(n, DH_ROWS, NGP_DENSITY_BWD2_MAX_BLOCKS) * DH_SUMS * 2;   // doubles, counted in floats
}

int ngp_density_head_bwd2(const float* a1, const float* sig, const float* r, const float* W2, const float* d_sig, int64_t n,
                          float* m, float* e1, float* dW2, float* db2, float* workspace, void* stream)
{
    if (n < 0) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!a1 || !sig || !r || !W2 || !m || !e1 || !dW2 || !db2 || !workspace) return NGP_EINVAL;
    if ((((uintptr_t)a1 | (uintptr_t)r | (uintptr_t)m | (uintptr_t)e1) & 15) || ((uintptr_t)workspace & 7) ||
        (((uintptr_t)sig | (uintptr_t)W2 | (uintptr_t)d_sig | (uintptr_t)dW2 | (uintptr_t)db2) & 3))
        return NGP_EINVAL;
    const int64_t n_tiles = (n + DH_ROWS - 1) / DH_ROWS;
    const int blocks = (int)ngp_capped_tiles(n, DH_ROWS, NGP_DENSITY_BWD2_MAX_BLOCKS);
    hipLaunchKernelGGL(density_head_bwd2_kernel, dim3((unsigned)blocks), dim3(DH_THREADS), 0, (hipStream_t)stream, a1, sig, r, W2,
                       d_sig, n, n_tiles, m, e1, reinterpret_cast<double*>(workspace));
    if (ngp_check_launch() != NGP_OK) return NGP_ELAUNCH;
    hipLaunchKernelGGL(density_head_bwd2_sum_kernel, dim3(1), dim3(DH_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const double*>(workspace), blocks, dW2, db2);
    return ngp_check_launch();
}

} // extern "C"
