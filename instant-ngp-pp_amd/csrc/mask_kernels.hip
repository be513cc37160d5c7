// Transient mask field (the reference's models/implicit_mask.py: an 8-level F = 2 hash grid over (u, v, image) and a
// 16 -> 64 (ReLU) -> 1 (Sigmoid) MLP with biases), ONE launch forward and ONE launch backward.
//
// The field is evaluated per RAY (2 048 - 16 384 rows a step), so it is launch-bound: the layered route costs a grid
// launch, two linear launches, two activation launches forward and eight more backward.  Work decomposition:
//   a TILE is 32 rows, a workgroup (256 lanes) owns a tile, lane = (row, j) with j in 0..7;
//   gather   lane (row, j) interpolates level j (8 corners x float2) -> feat[row][2j, 2j+1] in LDS;
//   layer 1  lane (row, j) forms the 8 hidden pre-activations k = 8q + j (W1, b1, W2 staged in LDS; the +1 padding of
//            the W1 rows makes the 8 distinct addresses of a wave instruction fall into 8 banks);
//   forward  partial <W2, relu(z1)> over the lane's 8 units, summed over the 8 lanes of the row, sigmoid;
//   backward the table is gathered AGAIN (3.4 MB, L2 resident) instead of saving feat / z1 (80 floats a row written and
//            read back through HBM by two launches); z1 goes through LDS once, then
//              - lane (row, j) forms d feat[2j, 2j+1] = sum_k W1[k][.] dz1[k] and scatters it into the level-j corners
//                it still holds in registers (float atomics, like ngp_grid_bwd_param);
//              - lane (k, quarter) adds the tile's 32 rows into its 4 dW1 elements (registers), db1 / dW2 / db2 likewise;
//            a workgroup walks its tiles with a grid stride and adds its weight sums ONCE at the end: 1 089 atomics per
//            workgroup, at most 256 workgroups.
// Negative coordinates (uvi lies in [-0.5, 0.5)) take tiny-cuda-nn's route (grid_index.h): (uint32_t)(int)floorf(p) and
// unsigned wrap in the dense index and in the hash.
#include "common.h"
#include "grid_index.h"

namespace {

constexpr int MK_L = 8;          // levels
constexpr int MK_IN = 16;        // L * F
constexpr int MK_H = 64;         // hidden width
constexpr int MK_ROWS = 32;      // rows per tile
constexpr int MK_LDW = MK_IN + 1;
constexpr int MK_LDZ = MK_H + 1;
constexpr int MK_MAX_BLOCKS = 256;

// the layout the kernels are written for (levels and features as compile-time constants)
bool mask_meta(const ngp_grid_desc* d, GridMeta& m)
{
    return make_meta(d, m) && m.n_levels == MK_L && m.n_features == 2;
}

struct Corners {
    uint32_t row[8];   // table row (level offset included)
    float w[8];
};

// the level rule is grid_index.h's
__device__ __forceinline__ Corners corners_of(const GridMeta& m, int level, float px, float py, float pz)
{
    const LevelInfo li = level_info(m, level);
    const Cell cell = cell_of(li.scale, px, py, pz);
    Corners c;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        c.row[k] = corner_row(li, cell, k);
        c.w[k] = corner_weight(cell.w[0], cell.w[1], cell.w[2], k);
    }
    return c;
}

struct MaskLds {
    float W1[MK_H * MK_LDW];
    float b1[MK_H], W2[MK_H];
    float feat[MK_ROWS * MK_IN];
};

__device__ __forceinline__ void stage_weights(MaskLds& s, const float* __restrict__ W1, const float* __restrict__ b1,
                                              const float* __restrict__ W2)
{
    for (int e = threadIdx.x; e < MK_H * MK_IN; e += 256) s.W1[(e / MK_IN) * MK_LDW + (e % MK_IN)] = W1[e];
    if (threadIdx.x < MK_H) { s.b1[threadIdx.x] = b1[threadIdx.x]; s.W2[threadIdx.x] = W2[threadIdx.x]; }
}

// lane (row, j): level j of the row -> feat[row][2j, 2j+1] in LDS (zeros for rows behind n); keeps the corners
__device__ __forceinline__ Corners gather_level(const GridMeta& m, const float* __restrict__ table,
                                                const float* __restrict__ uvi, int64_t row, bool live, int lrow, int j,
                                                MaskLds& s)
{
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) { px = uvi[3 * row]; py = uvi[3 * row + 1]; pz = uvi[3 * row + 2]; }
    const Corners c = corners_of(m, j, px, py, pz);
    float f0 = 0.0f, f1 = 0.0f;
    if (live) {
        float2 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = *reinterpret_cast<const float2*>(table + (size_t)c.row[k] * 2);
#pragma unroll
        for (int k = 0; k < 8; k++) { f0 = fmaf(c.w[k], v[k].x, f0); f1 = fmaf(c.w[k], v[k].y, f1); }
    }
    s.feat[lrow * MK_IN + 2 * j] = f0;
    s.feat[lrow * MK_IN + 2 * j + 1] = f1;
    return c;
}

// lane (row, j): pre-activations of the hidden units k = 8q + j, q = 0..7
__device__ __forceinline__ void layer1(const MaskLds& s, int lrow, int j, float (&z)[8])
{
    float x[MK_IN];
#pragma unroll
    for (int i = 0; i < MK_IN; i++) x[i] = s.feat[lrow * MK_IN + i];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int k = 8 * q + j;
        float a = s.b1[k];
#pragma unroll
        for (int i = 0; i < MK_IN; i++) a = fmaf(s.W1[k * MK_LDW + i], x[i], a);
        z[q] = a;
    }
}

__global__ void __launch_bounds__(256) mask_field_fwd_kernel(GridMeta m, const float* __restrict__ table,
                                                             const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ W2, const float* __restrict__ b2,
                                                             const float* __restrict__ uvi, int64_t n,
                                                             float* __restrict__ mask)
{
    __shared__ MaskLds s;
    stage_weights(s, W1, b1, W2);
    const int lrow = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int64_t row = (int64_t)blockIdx.x * MK_ROWS + lrow;
    const bool live = row < n;
    gather_level(m, table, uvi, row, live, lrow, j, s);
    __syncthreads();
    float z[8];
    layer1(s, lrow, j, z);
    float a2 = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; q++) a2 = fmaf(s.W2[8 * q + j], fmaxf(z[q], 0.0f), a2);
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) a2 += __shfl_xor(a2, o, 8);
    if (live && j == 0) mask[row] = 1.0f / (1.0f + expf(-(a2 + b2[0])));
}

// (waves_per_eu: with the shared level rule's plain modulo hipcc otherwise settles at 106 registers, 4 waves; held to the
// 5 waves it had, it allocates 88 without scratch)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) mask_field_bwd_kernel(GridMeta m, const float* __restrict__ table,
                                                             const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ W2, const float* __restrict__ uvi,
                                                             const float* __restrict__ mask,
                                                             const float* __restrict__ dL_dmask, int64_t n, int64_t n_tiles,
                                                             float* __restrict__ dtable, float* __restrict__ dW1,
                                                             float* __restrict__ db1, float* __restrict__ dW2,
                                                             float* __restrict__ db2)
{
    __shared__ MaskLds s;
    __shared__ float zs[MK_ROWS * MK_LDZ];   // layer-1 pre-activations of the tile
    __shared__ float dz2[MK_ROWS];           // dL/d(layer-2 pre-activation) of the tile's rows
    stage_weights(s, W1, b1, W2);
    const int lrow = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int wk = threadIdx.x >> 2, wi = (threadIdx.x & 3) * 4;   // this lane's weight-gradient elements: dW1[wk][wi..wi+3]
    float aW[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ab1 = 0.0f, aW2 = 0.0f, ab2 = 0.0f;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row = tile * MK_ROWS + lrow;
        const bool live = row < n;
        __syncthreads();   // the previous tile's readers are done with feat / zs / dz2 (and the weights are staged)
        const Corners c = gather_level(m, table, uvi, row, live, lrow, j, s);
        if (j == 0) {
            float d = 0.0f;
            if (live) { const float mk = mask[row]; d = dL_dmask[row] * mk * (1.0f - mk); }
            dz2[lrow] = d;
        }
        __syncthreads();
        {
            float z[8];
            layer1(s, lrow, j, z);
#pragma unroll
            for (int q = 0; q < 8; q++) zs[lrow * MK_LDZ + 8 * q + j] = z[q];
        }
        __syncthreads();
        // ---- lane (row, j): d feat[2j], d feat[2j+1], scattered into the corners of level j
        if (live) {
            const float d = dz2[lrow];
            float g0 = 0.0f, g1 = 0.0f;
#pragma unroll 8
            for (int k = 0; k < MK_H; k++) {
                const float dz1 = zs[lrow * MK_LDZ + k] > 0.0f ? d * s.W2[k] : 0.0f;
                g0 = fmaf(s.W1[k * MK_LDW + 2 * j], dz1, g0);
                g1 = fmaf(s.W1[k * MK_LDW + 2 * j + 1], dz1, g1);
            }
            if (g0 != 0.0f || g1 != 0.0f) {
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    atomicAdd(dtable + (size_t)c.row[k] * 2, c.w[k] * g0);
                    atomicAdd(dtable + (size_t)c.row[k] * 2 + 1, c.w[k] * g1);
                }
            }
        }
        // ---- lane (k, quarter): the tile's 32 rows into the lane's weight sums (rows behind n carry dz2 = 0)
        {
            const float w2 = s.W2[wk];
#pragma unroll 4
            for (int r = 0; r < MK_ROWS; r++) {
                const float z = zs[r * MK_LDZ + wk], d = dz2[r];
                const float dz1 = z > 0.0f ? d * w2 : 0.0f;
#pragma unroll
                for (int i = 0; i < 4; i++) aW[i] = fmaf(dz1, s.feat[r * MK_IN + wi + i], aW[i]);
                ab1 += dz1;
                aW2 = fmaf(d, fmaxf(z, 0.0f), aW2);
                ab2 += d;
            }
        }
    }
    // one add per workgroup per element
#pragma unroll
    for (int i = 0; i < 4; i++) atomicAdd(dW1 + wk * MK_IN + wi + i, aW[i]);
    if ((threadIdx.x & 3) == 0) { atomicAdd(db1 + wk, ab1); atomicAdd(dW2 + wk, aW2); }
    if (threadIdx.x == 0) atomicAdd(db2, ab2);
}

} // namespace

extern "C" {

int ngp_mask_field_fwd(const ngp_grid_desc* desc, const float* table, const float* W1, const float* b1, const float* W2,
                       const float* b2, const float* uvi, int64_t n, float* mask, void* stream)
{
    if (n < 0) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    GridMeta m;
    if (!mask_meta(desc, m) || !table || !W1 || !b1 || !W2 || !b2 || !uvi || !mask) return NGP_EINVAL;
    const int64_t n_tiles = (n + MK_ROWS - 1) / MK_ROWS;
    if (n_tiles > 0x7fffffff) return NGP_EINVAL;
    hipLaunchKernelGGL(mask_field_fwd_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, m, table, W1, b1,
                       W2, b2, uvi, n, mask);
    return ngp_check_launch();
}

int ngp_mask_field_bwd(const ngp_grid_desc* desc, const float* table, const float* W1, const float* b1, const float* W2,
                       const float* uvi, const float* mask, const float* dL_dmask, int64_t n, float* dtable, float* dW1,
                       float* db1, float* dW2, float* db2, void* stream)
{
    if (n < 0) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    GridMeta m;
    if (!mask_meta(desc, m) || !table || !W1 || !b1 || !W2 || !uvi || !mask || !dL_dmask || !dtable || !dW1 || !db1 ||
        !dW2 || !db2) return NGP_EINVAL;
    const int64_t n_tiles = (n + MK_ROWS - 1) / MK_ROWS;
    const unsigned blocks = (unsigned)ngp_capped_tiles(n, MK_ROWS, MK_MAX_BLOCKS);
    hipLaunchKernelGGL(mask_field_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, m, table, W1, b1, W2, uvi,
                       mask, dL_dmask, n, n_tiles, dtable, dW1, db1, dW2, db2);
    return ngp_check_launch();
}

} // extern "C"
