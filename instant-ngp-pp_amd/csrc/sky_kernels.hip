// The skybox (NGP(use_skybox=True), models/networks.py:128-148, 284-291): the colour of a ray's background from its
// direction alone, SH degree 3 -> tcnn network 9 -> 32 (ReLU) -> 3 (Sigmoid), bias-free with tcnn's ones-padding of the
// 9 inputs to 16 columns.  ONE launch forward and ONE launch (+ a 416-lane sum) backward, where the module route takes
// the normalisation, the remap, the SH encode and two MLP layers each way.
//
// Per ray, with params the network's 1024 floats, W1 (32,16) row-major then W2 (16,32) row-major:
//     u   = d / |d|                       (forward_skybox normalises the direction, no epsilon: a zero direction is NaN)
//     x   = (u + 1) / 2,  v = 2 x - 1     (the remap the encoder undoes)
//     y_0..8 = the degree-3 real SH basis of v, ngp_sh_fwd's polynomial forms:
//              0.2820948, -0.4886025 v_y, 0.4886025 v_z, -0.4886025 v_x, 1.0925484 v_x v_y, -1.0925484 v_y v_z,
//              0.9461747 v_z^2 - 0.3153916, -1.0925484 v_x v_z, 0.5462742 v_x^2 - 0.5462742 v_y^2
//     z_j = sum_{k<9} W1[j][k] y_k + sum_{k=9..15} W1[j][k]            (the padding columns multiply ones)
//     rgb_c = sigmoid(sum_j W2[c][j] relu(z_j)),  c < 3                 (rows 3..15 of W2 are never read)
// Work decomposition:
//   weights  folded once per workgroup into LDS as doubles: W1[j][0..8], b_j = the seven padding columns' sum, W2[c][j]
//            (416 doubles), read from there with wave-uniform (broadcast) reads;
//   double   everything between the float32 inputs and the float32 outputs, as the tone-mapper kernels do and for their
//            reasons: a z_j within float32 rounding of 0 takes the wrong side of the ReLU's kink and the ray's gradient is
//            off by a whole term, and y (1 - y) of a float32 y next to saturation has no digit.  A step has 8192 rays of
//            ~400 FMAs: the cost against a float32 build was not measured;
//   forward  a lane per ray, tiles of 256 rays walked with a grid stride;
//   backward nothing is saved but the inputs: phase A (a lane per ray) recomputes the basis and the hidden layer and
//            stages y_0..8 and dt_c = dL/drgb_c rgb_c (1 - rgb_c) in LDS; phase B (lane = (hidden unit j, slice q of 8):
//            the unit's rays q, q + 8, ... of the tile) recomputes z_j by phase A's expression on phase A's operands (the
//            same side of the kink) and keeps its 13 sums (dW2[0..2][j], dW1[j][0..8], the sum the seven padding columns
//            share) in registers ACROSS the workgroup's tiles.  At the end the eight slices are added in slice order
//            through LDS and the workgroup stores its 416 sums (doubles, plain vector stores) to the caller's workspace;
//            ngp_skybox_bwd's second launch adds them over the workgroups in launch-index order into dparams: no atomics,
//            the same bits on every run.  The ReLU derivative is z_j > 0, the sigmoid's e^-|s| / (1 + e^-|s|)^2.
// There is no gradient for the direction.
#include "common.h"

namespace {

constexpr int SKY_H = 32;                 // hidden width
constexpr int SKY_IN = 16;                // padded input width
constexpr int SKY_Y = 9;                  // SH degree 3
constexpr int SKY_W2_AT = SKY_H * SKY_IN; // first element of W2 inside the parameters
constexpr int SKY_TILE = 256;             // rays per tile = lanes per workgroup
constexpr int SKY_SLICES = SKY_TILE / SKY_H;      // phase B: lanes per hidden unit
constexpr int SKY_PER_UNIT = 3 + SKY_Y + 1;       // sums a phase-B lane keeps
constexpr int SKY_SUMS = SKY_H * SKY_PER_UNIT;    // 416: [0,96) dW2[c][j], [96,384) dW1[j][k<9], [384,416) padding of row j
constexpr int SKY_FWD_MAX_BLOCKS = 1024;

struct SkyFold {
    double w1[SKY_H][SKY_Y + 1];   // [j][0..8] = W1[j][k], [j][9] = b_j
    double w2[3][SKY_H];
};

__device__ __forceinline__ void fold_weights(SkyFold& fold, const float* __restrict__ prm)
{
    const int tid = threadIdx.x;
    if (tid < SKY_H) {
        const float* row = prm + tid * SKY_IN;
#pragma unroll
        for (int k = 0; k < SKY_Y; k++) fold.w1[tid][k] = (double)row[k];
        double b = 0.0;
#pragma unroll
        for (int k = SKY_Y; k < SKY_IN; k++) b += (double)row[k];
        fold.w1[tid][SKY_Y] = b;
    } else if (tid < SKY_H + 3 * SKY_H) {
        const int e = tid - SKY_H;   // c * 32 + j: rows 0..2 of W2 are contiguous
        fold.w2[e / SKY_H][e % SKY_H] = (double)prm[SKY_W2_AT + e];
    }
}

// the nine basis values of a raw direction
__device__ __forceinline__ void sky_basis(const float* __restrict__ rays_d, int64_t i, double* y)
{
    const double dx = (double)rays_d[3 * i], dy = (double)rays_d[3 * i + 1], dz = (double)rays_d[3 * i + 2];
    const double len = sqrt(dx * dx + dy * dy + dz * dz);
    const double x0 = (dx / len + 1.0) / 2.0, x1 = (dy / len + 1.0) / 2.0, x2 = (dz / len + 1.0) / 2.0;
    const double x = x0 * 2.0 - 1.0, yy = x1 * 2.0 - 1.0, z = x2 * 2.0 - 1.0;
    y[0] = 0.28209479177387814;
    y[1] = -0.48860251190291987 * yy; y[2] = 0.48860251190291987 * z; y[3] = -0.48860251190291987 * x;
    y[4] = 1.0925484305920792 * (x * yy); y[5] = -1.0925484305920792 * (yy * z);
    y[6] = 0.94617469575755997 * (z * z) - 0.31539156525251999;
    y[7] = -1.0925484305920792 * (x * z); y[8] = 0.54627421529603959 * (x * x) - 0.54627421529603959 * (yy * yy);
}

// z_j: one expression for the forward, phase A and phase B
__device__ __forceinline__ double sky_preact(const double* w /* [10] */, const double* y)
{
    double z = w[SKY_Y];
#pragma unroll
    for (int k = 0; k < SKY_Y; k++) z = fma(w[k], y[k], z);
    return z;
}

// s_c = sum_j W2[c][j] relu(z_j)
__device__ __forceinline__ void sky_hidden(const SkyFold& fold, const double* y, double* s)
{
    s[0] = s[1] = s[2] = 0.0;
#pragma unroll 8
    for (int j = 0; j < SKY_H; j++) {
        const double h = fmax(sky_preact(fold.w1[j], y), 0.0);
        s[0] = fma(fold.w2[0][j], h, s[0]);
        s[1] = fma(fold.w2[1][j], h, s[1]);
        s[2] = fma(fold.w2[2][j], h, s[2]);
    }
}

__global__ void __launch_bounds__(SKY_TILE) skybox_fwd_kernel(const float* __restrict__ prm, const float* __restrict__ rays_d,
                                                              int64_t n, int64_t n_tiles, float* __restrict__ rgb_bg)
{
    __shared__ SkyFold fold;
    fold_weights(fold, prm);
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t i = tile * SKY_TILE + threadIdx.x;
        if (i >= n) continue;
        double y[SKY_Y], s[3];
        sky_basis(rays_d, i, y);
        sky_hidden(fold, y, s);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double e = exp(-fabs(s[c]));
            rgb_bg[3 * i + c] = (float)(s[c] >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e));
        }
    }
}

__global__ void __launch_bounds__(SKY_TILE) skybox_bwd_kernel(const float* __restrict__ prm, const float* __restrict__ rays_d,
                                                              const float* __restrict__ dL_drgb, int64_t n, int64_t n_tiles,
                                                              double* __restrict__ partials)
{
    __shared__ SkyFold fold;
    // per tile rows 0..8: y_k, rows 9..11: dt_c of the tile's rays; at the end the 13 sums of every lane
    __shared__ __attribute__((aligned(16))) double stage[SKY_PER_UNIT][SKY_TILE];
    fold_weights(fold, prm);
    __syncthreads();
    const int tid = threadIdx.x;
    const int uj = tid % SKY_H, uq = tid / SKY_H;   // phase B: this lane's hidden unit and slice
    double mine[SKY_Y + 1], mine_w2[3];
#pragma unroll
    for (int k = 0; k <= SKY_Y; k++) mine[k] = fold.w1[uj][k];
#pragma unroll
    for (int c = 0; c < 3; c++) mine_w2[c] = fold.w2[c][uj];
    double acc_w2[3] = {0.0, 0.0, 0.0}, acc_w1[SKY_Y], acc_pad = 0.0;
#pragma unroll
    for (int k = 0; k < SKY_Y; k++) acc_w1[k] = 0.0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();   // the previous tile's phase B is done with the stage
        // ---- phase A: a lane per ray; rays behind n carry y = 0 and dt = 0
        const int64_t i = tile * SKY_TILE + tid;
        double y[SKY_Y], dt[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SKY_Y; k++) y[k] = 0.0;
        if (i < n) {
            double s[3];
            sky_basis(rays_d, i, y);
            sky_hidden(fold, y, s);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double e = exp(-fabs(s[c]));
                dt[c] = (double)dL_drgb[3 * i + c] * (e / ((1.0 + e) * (1.0 + e)));
            }
        }
#pragma unroll
        for (int k = 0; k < SKY_Y; k++) stage[k][tid] = y[k];
#pragma unroll
        for (int c = 0; c < 3; c++) stage[SKY_Y + c][tid] = dt[c];
        __syncthreads();
        // ---- phase B: hidden unit uj over the rays uq, uq + 8, ... of the tile
        for (int r = uq; r < SKY_TILE; r += SKY_SLICES) {
            double yr[SKY_Y];
#pragma unroll
            for (int k = 0; k < SKY_Y; k++) yr[k] = stage[k][r];
            const double t0 = stage[SKY_Y][r], t1 = stage[SKY_Y + 1][r], t2 = stage[SKY_Y + 2][r];
            const double z = sky_preact(mine, yr);
            const double h = fmax(z, 0.0);
            acc_w2[0] = fma(t0, h, acc_w2[0]); acc_w2[1] = fma(t1, h, acc_w2[1]); acc_w2[2] = fma(t2, h, acc_w2[2]);
            const double g = z > 0.0 ? fma(t2, mine_w2[2], fma(t1, mine_w2[1], t0 * mine_w2[0])) : 0.0;   // dL/dz_j
#pragma unroll
            for (int k = 0; k < SKY_Y; k++) acc_w1[k] = fma(g, yr[k], acc_w1[k]);
            acc_pad += g;
        }
    }
    // ---- the eight slices of a unit, added in slice order
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; c++) stage[c][tid] = acc_w2[c];
#pragma unroll
    for (int k = 0; k < SKY_Y; k++) stage[3 + k][tid] = acc_w1[k];
    stage[3 + SKY_Y][tid] = acc_pad;
    __syncthreads();
    double* out = partials + (size_t)blockIdx.x * SKY_SUMS;
    for (int e = tid; e < SKY_SUMS; e += SKY_TILE) {
        // e -> (row of the stage, hidden unit)
        int row, j;
        if (e < 3 * SKY_H) { row = e / SKY_H; j = e % SKY_H; }                                             // dW2[c][j]
        else if (e < 3 * SKY_H + SKY_H * SKY_Y) { const int f = e - 3 * SKY_H; j = f / SKY_Y; row = 3 + f % SKY_Y; }   // dW1[j][k]
        else { j = e - (3 * SKY_H + SKY_H * SKY_Y); row = 3 + SKY_Y; }                                       // padding of row j
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < SKY_SLICES; q++) s += stage[row][q * SKY_H + j];
        out[e] = s;
    }
}

// lane e = one of a workgroup's 416 sums: adds it over the workgroups in launch-index order
__global__ void __launch_bounds__(SKY_H) skybox_bwd_sum_kernel(const double* __restrict__ partials, int n_blocks,
                                                               float* __restrict__ dprm)
{
    const int e = blockIdx.x * SKY_H + threadIdx.x;   // 0 .. 415
    const float s = ordered_partial_sum(partials, n_blocks, SKY_SUMS, e);
    if (e < 3 * SKY_H) {
        dprm[SKY_W2_AT + e] += s;
    } else if (e < 3 * SKY_H + SKY_H * SKY_Y) {
        const int f = e - 3 * SKY_H;
        dprm[(f / SKY_Y) * SKY_IN + f % SKY_Y] += s;
    } else {
        const int j = e - (3 * SKY_H + SKY_H * SKY_Y);
#pragma unroll
        for (int k = SKY_Y; k < SKY_IN; k++) dprm[j * SKY_IN + k] += s;
    }
}

} // namespace

extern "C" {

int ngp_skybox_fwd(const float* params, const float* rays_d, int64_t n_rays, float* rgb_bg, void* stream)
{
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!params || !rays_d || !rgb_bg) return NGP_EINVAL;
    const int64_t n_tiles = (n_rays + SKY_TILE - 1) / SKY_TILE;
    const unsigned blocks = (unsigned)ngp_capped_tiles(n_rays, SKY_TILE, SKY_FWD_MAX_BLOCKS);
    hipLaunchKernelGGL(skybox_fwd_kernel, dim3(blocks), dim3(SKY_TILE), 0, (hipStream_t)stream, params, rays_d, n_rays, n_tiles,
                       rgb_bg);
    return ngp_check_launch();
}

int64_t ngp_skybox_bwd_workspace(int64_t n)
{
    if (n < 0) return NGP_EINVAL;
    return ngp_capped_tiles(n, SKY_TILE, NGP_SKYBOX_BWD_MAX_BLOCKS) * SKY_SUMS * 2;   // doubles, counted in floats
}

int ngp_skybox_bwd(const float* params, const float* rays_d, const float* dL_drgb_bg, int64_t n_rays, float* dparams,
                   float* workspace, void* stream)
{
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!params || !rays_d || !dL_drgb_bg || !dparams || !workspace || ((uintptr_t)workspace & 7)) return NGP_EINVAL;
    const int64_t n_tiles = (n_rays + SKY_TILE - 1) / SKY_TILE;
    const int blocks = (int)ngp_capped_tiles(n_rays, SKY_TILE, NGP_SKYBOX_BWD_MAX_BLOCKS);
    hipLaunchKernelGGL(skybox_bwd_kernel, dim3((unsigned)blocks), dim3(SKY_TILE), 0, (hipStream_t)stream, params, rays_d,
                       dL_drgb_bg, n_rays, n_tiles, reinterpret_cast<double*>(workspace));
    if (ngp_check_launch() != NGP_OK) return NGP_ELAUNCH;
    hipLaunchKernelGGL(skybox_bwd_sum_kernel, dim3(SKY_SUMS / SKY_H), dim3(SKY_H), 0, (hipStream_t)stream,
                       reinterpret_cast<const double*>(workspace), blocks, dparams);
    return ngp_check_launch();
}

} // extern "C"
