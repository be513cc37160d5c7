// HDR-NeRF tone-mappers (NGP(rgb_act='None'): three tcnn networks 1 -> 64 (ReLU) -> 1 (Sigmoid), one per colour channel,
// bias-free with tcnn's ones-padding of the input to 16 columns), ONE launch forward and ONE launch (+ a 9-block sum)
// backward, for all three channels.
//
// With the padding a channel is
//     z_j = a_j u + b_j,   a_j = W1[j][0],  b_j = sum_{k=1..15} W1[j][k],   u = log_radiance + ln(exposure)
//     y   = sigmoid(sum_j w_j relu(z_j)),   w_j = W2[0][j]
// so the layered route's (n,16) / (n,64) / (n,16) intermediates per channel (1.1 KB a sample through HBM, ~50 launches a
// step) shrink to the 28 useful bytes a sample.  Work decomposition:
//   weights  (a_j, b_j, w_j, a_j w_j) of the 3 x 64 hidden units are folded once per workgroup into LDS (6 KB) and read
//            from there with wave-uniform (broadcast) reads, two 16-byte reads a unit;
//   double   everything between the float32 inputs and the float32 outputs of the backward, and the hidden layer of the
//            forward, is formed in DOUBLE (~6 v_*_f64 a unit and sample; its cost against a float32 build was not
//            measured).  Three things float32 got wrong against the float64 restatement: a z_j within rounding of 0 takes
//            the wrong side of the ReLU's kink (seen: z = -1.3e-8 in one of 300 001 random samples, 192 units each) and
//            that sample's input gradient is off by a whole term dt a_j w_j; the rounding of a 64-term sum of both signs
//            goes through sigmoid' into every gradient; and y (1 - y) of a float32 y next to 1 has no correct digit, which
//            is all of a parameter sum that only saturated samples feed.  The forward's colour is mlp_act.h's sigmoid of the
//            float32-rounded sum; the parameter sums are rounded once, where they meet their float32 sinks;
//   forward  a lane per sample, tiles of 256 samples walked with a grid stride;
//   backward nothing is saved but the inputs: phase A (a lane per sample) recomputes the hidden layer, writes
//            d_log_radiance and stages u and dt = dy y (1 - y) per channel in LDS; phase B (a lane per (channel, hidden
//            unit): waves 0..2, a wave is one channel) walks the tile's 256 samples with broadcast reads and keeps its
//            three sums (dW2[0][j], dW1[j][0], the sum all 15 padding columns of dW1[j] share) in registers ACROSS the
//            workgroup's tiles.  At the end a workgroup stores its 576 sums (doubles, plain vector stores) to the caller's
//            workspace, and ngp_tonemap_bwd's second launch adds them over the workgroups in a fixed order into the sinks:
//            no float atomics (a step has ~10^6 samples on 576 addresses: one row for every adder is the slowest shape
//            there is) and a result that does not depend on scheduling.
// The forward's sigmoid is mlp_act.h's (act_fwd on the float32 sum); the ReLU is max(z, 0), its derivative z > 0 (act_bwd's
// y > 0 on y = relu(z)), the sigmoid's e^-|s| / (1 + e^-|s|)^2.
#include "common.h"
#include "mlp_act.h"

namespace {

constexpr int TM_H = 64;              // hidden width
constexpr int TM_IN = 16;             // padded input width
constexpr int TM_UNITS = 3 * TM_H;    // (channel, hidden unit) pairs
constexpr int TM_TILE = 256;          // samples per tile = lanes per workgroup
constexpr int TM_W2_AT = TM_H * TM_IN;   // first element of W2 inside a channel's parameters
constexpr int TM_FWD_MAX_BLOCKS = 2048;

struct TmParams {
    const float* p[3];
};
struct TmSinks {
    float* p[3];
};

struct __attribute__((aligned(16))) TmUnit {
    double a, b, w, aw;
};
struct TmFold {
    TmUnit unit[TM_UNITS];   // unit j of channel c at [c * 64 + j]
};

__device__ __forceinline__ void fold_weights(TmFold& fold, const TmParams& prm)
{
    if (threadIdx.x < TM_UNITS) {
        const int c = threadIdx.x / TM_H, j = threadIdx.x % TM_H;
        const float4* row = reinterpret_cast<const float4*>(prm.p[c] + j * TM_IN);   // 64-byte rows of a 16-byte aligned array
        const float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
        const double b = (((double)r0.y + r0.z) + ((double)r0.w + r1.x)) + (((double)r1.y + r1.z) + ((double)r1.w + r2.x)) +
                         ((((double)r2.y + r2.z) + ((double)r2.w + r3.x)) + (((double)r3.y + r3.z) + r3.w));
        const float w = prm.p[c][TM_W2_AT + j];
        fold.unit[threadIdx.x] = TmUnit{(double)r0.x, b, (double)w, (double)r0.x * (double)w};
    }
}

__device__ __forceinline__ double log_exposure(const float* __restrict__ exposure, int stride, int64_t i)
{
    return exposure ? log((double)exposure[stride ? i : 0]) : 0.0;
}

// sum_j w_j relu(a_j u + b_j) of one channel; also sum_j [z_j > 0] a_j w_j (the derivative of the first sum w.r.t. u)
template <bool WITH_DU>
__device__ __forceinline__ double hidden_dot(const TmFold& fold, int c, double u, double& dsum)
{
    double s = 0.0, d = 0.0;
#pragma unroll 16
    for (int j = 0; j < TM_H; j++) {
        const TmUnit f = fold.unit[c * TM_H + j];
        const double z = fma(f.a, u, f.b);
        s = fma(f.w, fmax(z, 0.0), s);
        if (WITH_DU) d += z > 0.0 ? f.aw : 0.0;
    }
    dsum = d;
    return s;
}

__global__ void __launch_bounds__(TM_TILE) tonemap_fwd_kernel(TmParams prm, const float* __restrict__ log_radiance,
                                                              const float* __restrict__ exposure, int stride, int64_t n,
                                                              int64_t n_tiles, float* __restrict__ rgb)
{
    __shared__ TmFold fold;
    fold_weights(fold, prm);
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t i = tile * TM_TILE + threadIdx.x;
        if (i >= n) continue;
        const double le = log_exposure(exposure, stride, i);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double unused;
            const double s = hidden_dot<false>(fold, c, (double)log_radiance[3 * i + c] + le, unused);
            rgb[3 * i + c] = act_fwd((float)s, NGP_ACT_SIGMOID);
        }
    }
}

__global__ void __launch_bounds__(TM_TILE) tonemap_bwd_kernel(TmParams prm, const float* __restrict__ log_radiance,
                                                              const float* __restrict__ exposure, int stride,
                                                              const float* __restrict__ dL_drgb, int64_t n, int64_t n_tiles,
                                                              float* __restrict__ d_log_radiance,
                                                              double* __restrict__ partials)
{
    __shared__ TmFold fold;
    __shared__ __attribute__((aligned(16))) double su[3][TM_TILE];    // u of the tile's samples, per channel
    __shared__ __attribute__((aligned(16))) double sdt[3][TM_TILE];   // dL/d(second-layer pre-activation)
    fold_weights(fold, prm);
    __syncthreads();
    const int tid = threadIdx.x;
    const int uc = tid / TM_H;   // phase B: this lane's channel (3: the fourth wave has no unit)
    const double mine_a = uc < 3 ? fold.unit[tid].a : 0.0, mine_b = uc < 3 ? fold.unit[tid].b : 0.0;
    const double mine_w = uc < 3 ? fold.unit[tid].w : 0.0;
    double acc_w2 = 0.0, acc_w10 = 0.0, acc_pad = 0.0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();   // the previous tile's phase B is done with su / sdt
        // ---- phase A: a lane per sample
        const int64_t i = tile * TM_TILE + tid;
        const bool live = i < n;
        const double le = live ? log_exposure(exposure, stride, i) : 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double u = 0.0, dt = 0.0;
            if (live) {
                u = (double)log_radiance[3 * i + c] + le;
                double dsum;
                const double s = hidden_dot<true>(fold, c, u, dsum);
                // sigmoid' from the double sum, through e = exp(-|s|): e / (1 + e)^2 keeps its digits where a float32 y next
                // to 1 leaves y (1 - y) with none
                const double e = exp(-fabs(s));
                dt = (double)dL_drgb[3 * i + c] * (e / ((1.0 + e) * (1.0 + e)));
                if (d_log_radiance) d_log_radiance[3 * i + c] = (float)(dt * dsum);
            }
            su[c][tid] = u;
            sdt[c][tid] = dt;
        }
        __syncthreads();
        // ---- phase B: a lane per (channel, hidden unit); samples behind n carry dt = 0.  The pre-activation is phase A's
        // expression on phase A's operands: both phases see the same side of the kink
        if (uc < 3) {
            const double2* u2 = reinterpret_cast<const double2*>(su[uc]);
            const double2* t2 = reinterpret_cast<const double2*>(sdt[uc]);
#pragma unroll 4
            for (int r = 0; r < TM_TILE / 2; r++) {
                const double2 u = u2[r], t = t2[r];
                const double us[2] = {u.x, u.y}, ts[2] = {t.x, t.y};
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const double z = fma(mine_a, us[k], mine_b);
                    const double g = z > 0.0 ? ts[k] * mine_w : 0.0;   // dL/dz_j
                    acc_w2 = fma(ts[k], fmax(z, 0.0), acc_w2);
                    acc_w10 = fma(g, us[k], acc_w10);
                    acc_pad += g;
                }
            }
        }
    }
    if (uc < 3) {
        double* out = partials + (size_t)blockIdx.x * (3 * TM_UNITS);
        out[tid] = acc_w2;
        out[TM_UNITS + tid] = acc_w10;
        out[2 * TM_UNITS + tid] = acc_pad;
    }
}

// lane (quantity q, channel c, unit j) = one of a workgroup's 576 sums: adds it over the workgroups in launch-index order
__global__ void __launch_bounds__(TM_H) tonemap_bwd_sum_kernel(const double* __restrict__ partials, int n_blocks, TmSinks dprm)
{
    const int e = blockIdx.x * TM_H + threadIdx.x;   // 0 .. 575
    const int q = e / TM_UNITS, c = (e % TM_UNITS) / TM_H, j = e % TM_H;
    const float s = ordered_partial_sum(partials, n_blocks, 3 * TM_UNITS, e);
    float* d = dprm.p[c];
    if (q == 0) {
        d[TM_W2_AT + j] += s;
    } else if (q == 1) {
        d[j * TM_IN] += s;
    } else {
#pragma unroll
        for (int k = 1; k < TM_IN; k++) d[j * TM_IN + k] += s;
    }
}

inline bool aligned16(const void* a, const void* b, const void* c)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

} // namespace

extern "C" {

int ngp_tonemap_fwd(const float* params0, const float* params1, const float* params2, const float* log_radiance,
                    const float* exposure, int exposure_stride, int64_t n, float* rgb, void* stream)
{
    if (n < 0 || (exposure_stride != 0 && exposure_stride != 1)) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!params0 || !params1 || !params2 || !log_radiance || !rgb || !aligned16(params0, params1, params2)) return NGP_EINVAL;
    const int64_t n_tiles = (n + TM_TILE - 1) / TM_TILE;
    const unsigned blocks = (unsigned)ngp_capped_tiles(n, TM_TILE, TM_FWD_MAX_BLOCKS);
    const TmParams prm = {{params0, params1, params2}};
    hipLaunchKernelGGL(tonemap_fwd_kernel, dim3(blocks), dim3(TM_TILE), 0, (hipStream_t)stream, prm, log_radiance, exposure,
                       exposure_stride, n, n_tiles, rgb);
    return ngp_check_launch();
}

int64_t ngp_tonemap_bwd_workspace(int64_t n)
{
    if (n < 0) return NGP_EINVAL;
    return ngp_capped_tiles(n, TM_TILE, NGP_TONEMAP_BWD_MAX_BLOCKS) * (3 * TM_UNITS) * 2;   // doubles, counted in floats
}

int ngp_tonemap_bwd(const float* params0, const float* params1, const float* params2, const float* log_radiance,
                    const float* exposure, int exposure_stride, const float* dL_drgb, int64_t n, float* d_log_radiance,
                    float* dparams0, float* dparams1, float* dparams2, float* workspace, void* stream)
{
    if (n < 0 || (exposure_stride != 0 && exposure_stride != 1)) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!params0 || !params1 || !params2 || !log_radiance || !dL_drgb || !dparams0 || !dparams1 || !dparams2 || !workspace ||
        !aligned16(params0, params1, params2) || ((uintptr_t)workspace & 7))
        return NGP_EINVAL;
    const int64_t n_tiles = (n + TM_TILE - 1) / TM_TILE;
    const int blocks = (int)ngp_capped_tiles(n, TM_TILE, NGP_TONEMAP_BWD_MAX_BLOCKS);
    const TmParams prm = {{params0, params1, params2}};
    const TmSinks dprm = {{dparams0, dparams1, dparams2}};
    hipLaunchKernelGGL(tonemap_bwd_kernel, dim3((unsigned)blocks), dim3(TM_TILE), 0, (hipStream_t)stream, prm, log_radiance,
                       exposure, exposure_stride, dL_drgb, n, n_tiles, d_log_radiance, reinterpret_cast<double*>(workspace));
    if (ngp_check_launch() != NGP_OK) return NGP_ELAUNCH;
    hipLaunchKernelGGL(tonemap_bwd_sum_kernel, dim3(3 * TM_UNITS / TM_H), dim3(TM_H), 0, (hipStream_t)stream,
                       reinterpret_cast<const double*>(workspace), blocks, dprm);
    return ngp_check_launch();
}

} // extern "C"
