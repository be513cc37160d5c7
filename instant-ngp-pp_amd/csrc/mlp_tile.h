// Tile pieces of the kernels built on v_mfma_f32_32x32x2_f32 with a 32-row tile per wave: the streaming MLP kernels
// (mlp_kernels.hip) and the fused density-field kernel (grid_kernels.hip), which has to take the same steps in the
// same order to write the same bits.  Arithmetic and data movement only: where a kernel places its loads and
// scheduling barriers stays with the kernel.
//   lane (li = lane & 31, lh = lane >> 5) holds A[row li][k = lh] and B[k = lh][column li] of one MFMA step;
//   accumulator register r of the lane is C[row acc_row(r, lh)][column li].
#pragma once
#include "common.h"
#include "mlp_act.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ constexpr int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// Four K steps for TN column blocks: the lane's 4 consecutive reduction indices of A against the same 4 of each B
// piece (the reduction index may be permuted freely as long as A and B agree).  A4: f32x4 or float[4].
template <int TN, typename A4>
__device__ __forceinline__ void mfma_k4(f32x16 (&acc)[TN], const A4& a, const float4 (&b)[TN])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int tn = 0; tn < TN; tn++) {
            const float bf[4] = {b[tn].x, b[tn].y, b[tn].z, b[tn].w};
            acc[tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bf[j], acc[tn], 0, 0, 0);
        }
    }
}

// dz1 = act1'(h) * sum_o dz2[o] W2[o][.] for 4 hidden units: the operand of a first layer's data and weight gradient,
// formed from the saved activations h so that dz1 never exists in memory
template <int OM, typename H4>
__device__ __forceinline__ void dz1_of(float (&out)[4], const float* d, const float (&w2)[OM][4], const H4& h, int act)
{
    float sv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int o = 0; o < OM; o++)
#pragma unroll
        for (int j = 0; j < 4; j++) sv[j] = fmaf(d[o], w2[o][j], sv[j]);
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = sv[j] * act_grad_fast(h[j], act);
}

// Accumulator block -> the wave's LDS tile [32][LD].  64 dword stores per lane and block would overrun the 64
// vector-memory operations a wave may have in flight; through LDS the 32x32 block leaves as 4 x 16 bytes per lane
// (tile_rows_out).  LDS operations of one wave execute in order, so a kernel that keeps to its wave's tile needs no
// barrier between the two on an unpadded tile (LD = 32: both access patterns are conflict-free).
template <int LD>
__device__ __forceinline__ void acc_to_tile(float* __restrict__ stg, const f32x16& acc, int li, int lh)
{
#pragma unroll
    for (int r = 0; r < 16; r++) stg[acc_row(r, lh) * LD + li] = acc[r];
}

// the wave's [32][LD] LDS tile -> rows m0 .. m0 + 31 (those below M) of dst, columns col0 .. col0 + 31: every store
// instruction writes whole 128-byte row segments
template <int LD>
__device__ __forceinline__ void tile_rows_out(const float* __restrict__ stg, float* __restrict__ dst, int64_t ld,
                                              int64_t m0, int64_t M, int col0, int lane)
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int f = lane + 64 * i, row = f >> 3, c4 = (f & 7) * 4;
        const float4 v = *reinterpret_cast<const float4*>(stg + row * LD + c4);
        if (m0 + row < M) *reinterpret_cast<float4*>(dst + (m0 + row) * ld + col0 + c4) = v;
    }
}

// Transposing butterfly: every lane holds 16 partial sums (one per accumulator register, i.e. per row) of its column;
// 16 shuffles instead of 16 x 5 leave the total over the 32 columns of ONE row per lane pair: both lanes of the pair
// hold the total of row butterfly_row(li, lh).
// PLAIN: an empty asm barrier on the two inputs of each select.  Without it hipcc turns `up ? v[j + half] : v[j]`
// into an extract with a lane-dependent index, i.e. a 15-compare select chain per read (930 vector instructions per
// tile).  For one output per lane only: with four the compiler emits the plain selects by itself and the barrier
// costs 5 %.
template <bool PLAIN>
__device__ __forceinline__ float butterfly16(float (&v)[16], int li)
{
#pragma unroll
    for (int half = 8; half >= 1; half >>= 1) {
        const int mask = half * 2;   // 16, 8, 4, 2
        const bool up = (li & mask) != 0;
#pragma unroll
        for (int j = 0; j < half; j++) {
            float lo = v[j], hi = v[j + half];
            if constexpr (PLAIN) asm volatile("" : "+v"(lo), "+v"(hi));
            const float keep = up ? hi : lo;
            const float send = up ? lo : hi;
            v[j] = keep + __shfl_xor(send, mask, 64);
        }
    }
    return v[0] + __shfl_xor(v[0], 1, 64);
}

__device__ __forceinline__ int butterfly_row(int li, int lh)
{
    const int rr = ((li >> 4) & 1) * 8 + ((li >> 3) & 1) * 4 + ((li >> 2) & 1) * 2 + ((li >> 1) & 1);
    return acc_row(rr, lh);
}

}  // namespace
