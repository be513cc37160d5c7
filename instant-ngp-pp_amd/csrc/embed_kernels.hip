// Per-image appearance codes (the reference's embed_a: an nn.Embedding(n_imgs, E) row per training image, read by
// rgb_net in the columns behind the 144 encoded ones): the per-sample broadcast of a ray's code into rgb_net's input
// matrix, and the segmented sum of that block's gradient back into the table.  ONE launch each way, in place of
// weight[img][ray] -> repeat_interleave -> strided copy -> ones fill and of their autograd chain.
//
// Both kernels are RAY-parallel: a wave owns a row of rays_a (ray index, first sample, sample count) and walks the
// ray's samples; there is no sample -> ray map, and none is needed.
//   forward   the wave reads the ray's code once (E 4-byte loads: a table row is 4 E bytes and 16-byte aligned only when
//             E is a multiple of 4) and writes it, followed by tcnn's ones-padding, into `n_cols` columns of every sample
//             row.  Where the destination allows it (16-byte aligned base, ld and n_cols multiples of 4, n_cols / 4 a
//             divisor of 64: rgb_in's column 144 always does) a lane owns one float4 of a row and the wave covers
//             256 / n_cols rows per store instruction; otherwise a lane owns one float.
//   backward  lane = (sample slot, column) with CP = E rounded up to a power of two columns and 64 / CP slots; each lane
//             sums its column over the samples slot, slot + 64/CP, ... (4-byte loads: the rows of dfeat_rgb are 4 (128 + E)
//             bytes apart), xor-shuffles over the slots leave the ray's sum in every slot.  A wave walks EB_CHUNK
//             CONSECUTIVE rows of rays_a and keeps one running sum per column, tagged with the image index: it goes to
//             memory (one float atomic per column, from slot 0) when the image changes and once at the end.  With all
//             rays of a batch from one image (the datasets' `same_image` strategy) that is one flush per wave instead of
//             one per ray on the same 4 E bytes.
// Guards: a ray with count <= 0 contributes nothing; a ray whose image index lies outside [0, n_imgs), or whose ray index
// lies outside [0, n_rays), gets ZEROS forward (and the ones-padding) and contributes nothing backward: such an index is
// never used as an address.  Sample rows that belong to no segment, and columns outside [0, n_cols), are not touched.
#include "common.h"

namespace {

constexpr int EB_WAVES = 4;          // waves per workgroup (256 lanes)
constexpr int EB_MAX_BLOCKS = 2048;
constexpr int EB_MAX_E = 32;
constexpr int EB_CHUNK = 8;          // rays_a rows per wave in the backward (not tuned)

// image of row r of rays_a, or -1 when the ray or its image is out of range
__device__ __forceinline__ int64_t image_of(const int64_t* __restrict__ img_idxs, int64_t ray, int64_t n_rays,
                                            int64_t n_imgs)
{
    if (ray < 0 || ray >= n_rays) return -1;
    const int64_t img = img_idxs[ray];
    return (img < 0 || img >= n_imgs) ? -1 : img;
}

template <bool VEC>
__global__ void __launch_bounds__(64 * EB_WAVES) embed_a_fwd_kernel(const float* __restrict__ weight, int64_t n_imgs, int E,
                                                                    const int64_t* __restrict__ img_idxs,
                                                                    const int64_t* __restrict__ rays_a, int64_t n_rays,
                                                                    float* __restrict__ out, int64_t ld, int n_cols)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * EB_WAVES + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * EB_WAVES;
    // this lane's place in a sample row: VEC one float4 (columns c0 .. c0+3), else one float (column c0)
    const int per_row = VEC ? n_cols / 4 : n_cols;       // lanes that cover one row
    const int rows_per_pass = VEC ? 64 / per_row : 0;    // VEC only: per_row divides 64
    const int c0 = VEC ? (lane % per_row) * 4 : 0;
    for (int64_t r = wave; r < n_rays; r += n_waves) {
        const int64_t start = rays_a[3 * r + 1], count = rays_a[3 * r + 2];
        if (count <= 0) continue;
        const int64_t img = image_of(img_idxs, rays_a[3 * r], n_rays, n_imgs);
        const float* __restrict__ w = weight + (img < 0 ? 0 : img) * (int64_t)E;
        if (VEC) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int c = c0 + i;
                v[i] = c >= E ? 1.0f : (img < 0 ? 0.0f : w[c]);
            }
            const float4 q = make_float4(v[0], v[1], v[2], v[3]);
            for (int64_t s = lane / per_row; s < count; s += rows_per_pass)
                *reinterpret_cast<float4*>(out + (start + s) * ld + c0) = q;
        } else {
            const int64_t total = count * n_cols;
            for (int64_t e = lane; e < total; e += 64) {
                const int64_t s = e / n_cols;
                const int c = (int)(e - s * n_cols);
                out[(start + s) * ld + c] = c >= E ? 1.0f : (img < 0 ? 0.0f : w[c]);
            }
        }
    }
}

template <int CP>   // columns per slot group: E rounded up to a power of two
__global__ void __launch_bounds__(64 * EB_WAVES) embed_a_bwd_kernel(const float* __restrict__ dL_dcols, int64_t ld, int E,
                                                                    const int64_t* __restrict__ img_idxs,
                                                                    const int64_t* __restrict__ rays_a, int64_t n_rays,
                                                                    int64_t n_imgs, float* __restrict__ d_weight)
{
    constexpr int SLOTS = 64 / CP;
    const int lane = threadIdx.x & 63;
    const int col = lane % CP, slot = lane / CP;
    const bool live = col < E;
    const int64_t wave = (int64_t)blockIdx.x * EB_WAVES + (threadIdx.x >> 6);
    const int64_t r0 = wave * EB_CHUNK;
    const int64_t r1 = r0 + EB_CHUNK < n_rays ? r0 + EB_CHUNK : n_rays;
    int64_t run_img = -1;    // wave-uniform
    float run = 0.0f;        // this lane's column of the run (every slot holds the same value)
    for (int64_t r = r0; r < r1; r++) {
        const int64_t start = rays_a[3 * r + 1], count = rays_a[3 * r + 2];
        if (count <= 0) continue;
        const int64_t img = image_of(img_idxs, rays_a[3 * r], n_rays, n_imgs);
        if (img < 0) continue;
        float a = 0.0f;
        if (live) {
            const float* __restrict__ p = dL_dcols + start * ld + col;
#pragma unroll 4
            for (int64_t s = slot; s < count; s += SLOTS) a += p[s * ld];
        }
#pragma unroll
        for (int o = CP; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
        if (img != run_img) {
            if (run_img >= 0 && live && slot == 0) atomicAdd(d_weight + run_img * E + col, run);
            run_img = img;
            run = 0.0f;
        }
        run += a;
    }
    if (run_img >= 0 && live && slot == 0) atomicAdd(d_weight + run_img * E + col, run);
}

} // namespace

extern "C" {

int ngp_embed_a_fwd(const float* weight, int64_t n_imgs, int E, const int64_t* img_idxs, const int64_t* rays_a,
                    int64_t n_rays, float* out, int64_t ld, int n_cols, void* stream)
{
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!weight || !img_idxs || !rays_a || !out || n_imgs <= 0 || E < 1 || E > EB_MAX_E || n_cols < E || n_cols > 64 ||
        ld < n_cols) return NGP_EINVAL;
    const dim3 grid((unsigned)ngp_capped_tiles(n_rays, EB_WAVES, EB_MAX_BLOCKS));
    const bool vec = ((uintptr_t)out % 16 == 0) && ld % 4 == 0 && n_cols % 4 == 0 && 64 % (n_cols / 4) == 0;
    if (vec)
        hipLaunchKernelGGL(embed_a_fwd_kernel<true>, grid, dim3(64 * EB_WAVES), 0, (hipStream_t)stream, weight, n_imgs, E,
                           img_idxs, rays_a, n_rays, out, ld, n_cols);
    else
        hipLaunchKernelGGL(embed_a_fwd_kernel<false>, grid, dim3(64 * EB_WAVES), 0, (hipStream_t)stream, weight, n_imgs, E,
                           img_idxs, rays_a, n_rays, out, ld, n_cols);
    return ngp_check_launch();
}

int ngp_embed_a_bwd(const float* dL_dcols, int64_t ld, int E, const int64_t* img_idxs, const int64_t* rays_a,
                    int64_t n_rays, int64_t n_imgs, float* d_weight, void* stream)
{
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!dL_dcols || !img_idxs || !rays_a || !d_weight || n_imgs <= 0 || E < 1 || E > EB_MAX_E || ld < E) return NGP_EINVAL;
    const int64_t waves = (n_rays + EB_CHUNK - 1) / EB_CHUNK;
    const int64_t blocks = (waves + EB_WAVES - 1) / EB_WAVES;
    if (blocks > 0x7fffffff) return NGP_EINVAL;
    const dim3 grid((unsigned)blocks), block(64 * EB_WAVES);
#define EB_LAUNCH(CP) hipLaunchKernelGGL(embed_a_bwd_kernel<CP>, grid, block, 0, (hipStream_t)stream, dL_dcols, ld, E, \
                                         img_idxs, rays_a, n_rays, n_imgs, d_weight)
    if (E <= 1) EB_LAUNCH(1);
    else if (E <= 2) EB_LAUNCH(2);
    else if (E <= 4) EB_LAUNCH(4);
    else if (E <= 8) EB_LAUNCH(8);
    else if (E <= 16) EB_LAUNCH(16);
    else EB_LAUNCH(32);
#undef EB_LAUNCH
    return ngp_check_launch();
}

} // extern "C"
