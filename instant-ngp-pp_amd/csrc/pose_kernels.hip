// Camera pose refinement (the reference's --optimize_ext: a per-image axis-angle rotation dR and translation dT trained
// beside the field, train.py:143-149, 225-230): the rays of a batch from (poses, dR, dT, directions, image, pixel) on the
// device, the adjoint of that map reduced per image, and the adjoint of the view-direction encoding.  ONE launch each.
//
//   forward   a lane per ray.  v = dR[img], theta = |v| + 1e-7, K = skew(v) (datasets/ray_utils.py axisangle_to_R):
//             Rd = (I + sin(theta)/theta K) + (1 - cos(theta))/theta^2 K^2,  R' = Rd Rp,  rays_d_i = (R'_i0 dir_0 +
//             R'_i1 dir_1) + R'_i2 dir_2,  rays_o = t + dT[img].  1 - cos(theta) is formed as 2 sin^2(theta/2): the literal
//             form is 0 in float32 below theta ~ 3e-4.  Compiled without FMA contraction: at dR = dT = 0 Rd is exactly I
//             and the rays are bit for bit get_rays' fixed-order float32 products.
//   backward  a wave per PB_CHUNK consecutive rows of rays_a (the shape of embed_a_bwd_kernel).  The lanes stride a ray's
//             samples and sum the six numbers of RayMarcher.backward (custom_functions.py): g_o = sum g_x, g_d = sum (g_x t
//             + g_dir); xor-shuffles leave the sums in every lane.  With w = Rp dir_cam, dL/dRd = g_d (x) w and dL/dT = g_o;
//             both are linear in the ray's sums, so the wave keeps ONE running (3x3 | 3) per run of rays of one image and
//             applies the closed-form derivative of Rd(v) once per run: lanes 0..5 send the six results as float atomics.
//             With the `same_image` sampling strategy that is one flush per wave.
//             d Rd / d v: with A(X) = (X21 - X12, X02 - X20, X10 - X01) (the adjoint of skew) and N = M K^T + K^T M,
//               g_v = a A(M) + b A(N) + (a' <M, K> + b' <M, K^2>) v / |v|,   a = sin(theta)/theta, b = (1 - cos)/theta^2;
//             the last term is exactly 0 at v = 0 (torch's norm backward).  Below theta = 0.25 a' and b' come from their
//             series (the closed forms cancel: theta cos(theta) - sin(theta) ~ -theta^3 / 3).
//   SH        dL/dd of y = SH4((normalize(d, eps = 1e-6) + 1) / 2) (ngp_sh_fwd_dirs), a lane per row: the basis'
//             derivative at the unit direction, then F.normalize's backward (under the clamp: g / eps, as torch's
//             clamp_min passes no gradient to the norm there).
// Guards: an image, pixel, ray or sample index outside its range is never used as an address.  Forward: zero rays.
// Backward: such a ray (or sample) contributes nothing; rows of images that no ray names are not touched.
#include "common.h"

namespace {

constexpr int PB_WAVES = 4;    // waves per workgroup (256 lanes)
constexpr int PB_CHUNK = 8;    // rays_a rows per wave in the backward (embed_a_bwd_kernel's; DESIGN section 7: not tuned)
constexpr float PB_SERIES_BELOW = 0.25f;

struct Rodrigues {
    float a, b;        // sin(theta)/theta, (1 - cos(theta))/theta^2
    float nv, th;      // |v|, |v| + 1e-7
};

__device__ __forceinline__ Rodrigues rodrigues_coef(float x, float y, float z)
{
    Rodrigues r;
    r.nv = sqrtf(x * x + y * y + z * z);
    r.th = r.nv + 1e-7f;
    r.a = sinf(r.th) / r.th;
    const float sh = sinf(0.5f * r.th);
    r.b = 2.0f * sh * sh / (r.th * r.th);
    return r;
}

__device__ __forceinline__ void skew_and_square(float x, float y, float z, float* K, float* K2)
{
    K[0] = 0.0f; K[1] = -z;   K[2] = y;
    K[3] = z;    K[4] = 0.0f; K[5] = -x;
    K[6] = -y;   K[7] = x;    K[8] = 0.0f;
    K2[0] = -(z * z) - y * y; K2[1] = x * y;            K2[2] = x * z;
    K2[3] = x * y;            K2[4] = -(z * z) - x * x; K2[5] = y * z;
    K2[6] = x * z;            K2[7] = y * z;            K2[8] = -(y * y) - x * x;
}

__global__ void __launch_bounds__(256) pose_rays_fwd_kernel(const float* __restrict__ poses, const float* __restrict__ dR,
                                                            const float* __restrict__ dT, const float* __restrict__ directions,
                                                            const int64_t* __restrict__ img_idxs,
                                                            const int64_t* __restrict__ pix_idxs, int64_t n_imgs, int64_t n_pix,
                                                            int64_t n_rays, float* __restrict__ rays_o, float* __restrict__ rays_d)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    const int64_t img = img_idxs[r], pix = pix_idxs[r];
    if (img < 0 || img >= n_imgs || pix < 0 || pix >= n_pix) {
#pragma unroll
        for (int i = 0; i < 3; i++) rays_o[3 * r + i] = rays_d[3 * r + i] = 0.0f;
        return;
    }
    const float* __restrict__ P = poses + img * 12;
    const float x = dR[3 * img], y = dR[3 * img + 1], z = dR[3 * img + 2];
    const Rodrigues c = rodrigues_coef(x, y, z);
    float K[9], K2[9], Rd[9];
    skew_and_square(x, y, z, K, K2);
#pragma unroll
    for (int i = 0; i < 9; i++) Rd[i] = ((i % 4 == 0 ? 1.0f : 0.0f) + c.a * K[i]) + c.b * K2[i];
    const float d0 = directions[3 * pix], d1 = directions[3 * pix + 1], d2 = directions[3 * pix + 2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float Rn[3];
#pragma unroll
        for (int j = 0; j < 3; j++) Rn[j] = (Rd[3 * i] * P[j] + Rd[3 * i + 1] * P[4 + j]) + Rd[3 * i + 2] * P[8 + j];
        rays_d[3 * r + i] = (Rn[0] * d0 + Rn[1] * d1) + Rn[2] * d2;
        rays_o[3 * r + i] = P[4 * i + 3] + dT[3 * img + i];
    }
}

// the six gradient entries of image `img` from the run's sums: M (3x3) = dL/dRd, gT (3) = dL/dT
__device__ __forceinline__ void pose_flush(const float* __restrict__ dR, int64_t img, const float* M, const float* gT,
                                           int lane, float* __restrict__ g_dR, float* __restrict__ g_dT)
{
    const float x = dR[3 * img], y = dR[3 * img + 1], z = dR[3 * img + 2];
    const Rodrigues c = rodrigues_coef(x, y, z);
    float K[9], K2[9], N[9];
    skew_and_square(x, y, z, K, K2);
    // N = M K^T + K^T M = -(M K + K M)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) s += M[3 * i + k] * K[3 * k + j] + K[3 * i + k] * M[3 * k + j];
            N[3 * i + j] = -s;
        }
    float mk = 0.0f, mk2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        mk += M[i] * K[i];
        mk2 += M[i] * K2[i];
    }
    const float th = c.th;
    float da, db;
    if (th < PB_SERIES_BELOW) {
        const float t2 = th * th;
        da = th * (-1.0f / 3.0f + t2 * (1.0f / 30.0f - t2 * (1.0f / 840.0f)));
        db = th * (-1.0f / 12.0f + t2 * (1.0f / 180.0f - t2 * (1.0f / 6720.0f)));
    } else {
        const float s = sinf(th), co = cosf(th), sh = sinf(0.5f * th);
        da = (th * co - s) / (th * th);
        db = (th * s - 4.0f * sh * sh) / (th * th * th);
    }
    const float radial = c.nv > 0.0f ? (da * mk + db * mk2) / c.nv : 0.0f;
    float g[6];
    g[0] = c.a * (M[7] - M[5]) + c.b * (N[7] - N[5]) + radial * x;
    g[1] = c.a * (M[2] - M[6]) + c.b * (N[2] - N[6]) + radial * y;
    g[2] = c.a * (M[3] - M[1]) + c.b * (N[3] - N[1]) + radial * z;
    g[3] = gT[0]; g[4] = gT[1]; g[5] = gT[2];
    if (lane < 3) atomicAdd(g_dR + 3 * img + lane, lane == 0 ? g[0] : (lane == 1 ? g[1] : g[2]));
    else if (lane < 6) atomicAdd(g_dT + 3 * img + (lane - 3), lane == 3 ? g[3] : (lane == 4 ? g[4] : g[5]));
}

__global__ void __launch_bounds__(64 * PB_WAVES) pose_rays_bwd_kernel(
    const float* __restrict__ g_x, const float* __restrict__ g_dir, const float* __restrict__ ts,
    const int64_t* __restrict__ rays_a, const float* __restrict__ poses, const float* __restrict__ dR,
    const float* __restrict__ directions, const int64_t* __restrict__ img_idxs, const int64_t* __restrict__ pix_idxs,
    int64_t n_imgs, int64_t n_pix, int64_t n_rays, int64_t n, float* __restrict__ g_dR, float* __restrict__ g_dT)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * PB_WAVES + (threadIdx.x >> 6);
    const int64_t r0 = wave * PB_CHUNK;
    const int64_t r1 = r0 + PB_CHUNK < n_rays ? r0 + PB_CHUNK : n_rays;
    int64_t run_img = -1;            // wave-uniform
    float M[9], gT[3];               // the run's sums (the same bits in every lane)
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = 0.0f;
    gT[0] = gT[1] = gT[2] = 0.0f;
    for (int64_t r = r0; r < r1; r++) {
        const int64_t ray = rays_a[3 * r], start = rays_a[3 * r + 1], count = rays_a[3 * r + 2];
        if (count <= 0 || ray < 0 || ray >= n_rays) continue;
        const int64_t img = img_idxs[ray], pix = pix_idxs[ray];
        if (img < 0 || img >= n_imgs || pix < 0 || pix >= n_pix) continue;
        // samples outside [0, n) are skipped, not read
        const int64_t lo = start < 0 ? 0 : start;
        const int64_t hi = start + count < n ? start + count : n;
        float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t s = lo + lane; s < hi; s += 64) {
            const float t = ts[s];
            const float gx0 = g_x[3 * s], gx1 = g_x[3 * s + 1], gx2 = g_x[3 * s + 2];
            a[0] += gx0; a[1] += gx1; a[2] += gx2;
            float e0 = gx0 * t, e1 = gx1 * t, e2 = gx2 * t;
            if (g_dir) {
                e0 += g_dir[3 * s]; e1 += g_dir[3 * s + 1]; e2 += g_dir[3 * s + 2];
            }
            a[3] += e0; a[4] += e1; a[5] += e2;
        }
#pragma unroll
        for (int k = 0; k < 6; k++) a[k] = wave_sum(a[k]);
        if (img != run_img) {
            if (run_img >= 0) pose_flush(dR, run_img, M, gT, lane, g_dR, g_dT);
            run_img = img;
#pragma unroll
            for (int i = 0; i < 9; i++) M[i] = 0.0f;
            gT[0] = gT[1] = gT[2] = 0.0f;
        }
        const float* __restrict__ P = poses + img * 12;
        const float d0 = directions[3 * pix], d1 = directions[3 * pix + 1], d2 = directions[3 * pix + 2];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float w = (P[4 * k] * d0 + P[4 * k + 1] * d1) + P[4 * k + 2] * d2;    // (Rp dir_cam)_k
#pragma unroll
            for (int i = 0; i < 3; i++) M[3 * i + k] += a[3 + i] * w;
        }
        gT[0] += a[0]; gT[1] += a[1]; gT[2] += a[2];
    }
    if (run_img >= 0) pose_flush(dR, run_img, M, gT, lane, g_dR, g_dT);
}

__global__ void __launch_bounds__(256) sh_bwd_dirs_kernel(const float* __restrict__ d, const float* __restrict__ dL_dy,
                                                          int64_t lddy, int64_t n, float* __restrict__ dL_dd)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float d0 = d[3 * i], d1 = d[3 * i + 1], d2 = d[3 * i + 2];
    const float nrm = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    const float inv = 1.0f / fmaxf(nrm, 1e-6f);
    const float x = d0 * inv, y = d1 * inv, z = d2 * inv;
    float g[16];
#pragma unroll
    for (int k = 0; k < 16; k++) g[k] = dL_dy[i * lddy + k];
    // d SH4 / d (x, y, z) at the unit direction (the basis of grid_kernels.hip's sh_eval; the (.+1)/2 remap and the
    // encoder's 2x-1 cancel)
    const float x2 = x * x, y2 = y * y, z2 = z * z;
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    gy += -0.48860251190291987f * g[1]; gz += 0.48860251190291987f * g[2]; gx += -0.48860251190291987f * g[3];
    gx += 1.0925484305920792f * y * g[4];  gy += 1.0925484305920792f * x * g[4];
    gy += -1.0925484305920792f * z * g[5]; gz += -1.0925484305920792f * y * g[5];
    gz += 2.0f * 0.94617469575755997f * z * g[6];
    gx += -1.0925484305920792f * z * g[7]; gz += -1.0925484305920792f * x * g[7];
    gx += 2.0f * 0.54627421529603959f * x * g[8]; gy += -2.0f * 0.54627421529603959f * y * g[8];
    gx += 0.59004358992664352f * (-6.0f * x * y) * g[9];  gy += 0.59004358992664352f * (-3.0f * x2 + 3.0f * y2) * g[9];
    gx += 2.8906114426405538f * y * z * g[10]; gy += 2.8906114426405538f * x * z * g[10];
    gz += 2.8906114426405538f * x * y * g[10];
    gy += 0.45704579946446572f * (1.0f - 5.0f * z2) * g[11]; gz += 0.45704579946446572f * y * (-10.0f * z) * g[11];
    gz += 0.3731763325901154f * (15.0f * z2 - 3.0f) * g[12];
    gx += 0.45704579946446572f * (1.0f - 5.0f * z2) * g[13]; gz += 0.45704579946446572f * x * (-10.0f * z) * g[13];
    gx += 1.4453057213202769f * z * 2.0f * x * g[14]; gy += -1.4453057213202769f * z * 2.0f * y * g[14];
    gz += 1.4453057213202769f * (x2 - y2) * g[14];
    gx += 0.59004358992664352f * (-3.0f * x2 + 3.0f * y2) * g[15]; gy += 0.59004358992664352f * 6.0f * x * y * g[15];
    // F.normalize(eps = 1e-6) backward: u = d / max(|d|, eps)
    float o0, o1, o2;
    if (nrm >= 1e-6f) {
        const float dot = (gx * x + gy * y) + gz * z;
        o0 = (gx - x * dot) * inv; o1 = (gy - y * dot) * inv; o2 = (gz - z * dot) * inv;
    } else {
        o0 = gx * inv; o1 = gy * inv; o2 = gz * inv;
    }
    dL_dd[3 * i] = o0; dL_dd[3 * i + 1] = o1; dL_dd[3 * i + 2] = o2;
}

} // namespace

extern "C" {

int ngp_pose_rays_fwd(const float* poses, const float* dR, const float* dT, const float* directions,
                      const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_imgs, int64_t n_pix, int64_t n_rays,
                      float* rays_o, float* rays_d, void* stream)
{
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!poses || !dR || !dT || !directions || !img_idxs || !pix_idxs || !rays_o || !rays_d || n_imgs <= 0 || n_pix <= 0)
        return NGP_EINVAL;
    const int64_t blocks = (n_rays + 255) / 256;
    if (blocks > 0x7fffffff) return NGP_EINVAL;
    hipLaunchKernelGGL(pose_rays_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, poses, dR, dT,
                       directions, img_idxs, pix_idxs, n_imgs, n_pix, n_rays, rays_o, rays_d);
    return ngp_check_launch();
}

int ngp_pose_rays_bwd(const float* g_x, const float* g_dir, const float* ts, const int64_t* rays_a, const float* poses,
                      const float* dR, const float* directions, const int64_t* img_idxs, const int64_t* pix_idxs,
                      int64_t n_imgs, int64_t n_pix, int64_t n_rays, int64_t n, float* g_dR, float* g_dT, void* stream)
{
    if (n_rays < 0 || n < 0) return NGP_EINVAL;
    if (n_rays == 0 || n == 0) return NGP_OK;
    if (!g_x || !ts || !rays_a || !poses || !dR || !directions || !img_idxs || !pix_idxs || !g_dR || !g_dT || n_imgs <= 0 ||
        n_pix <= 0) return NGP_EINVAL;
    const int64_t waves = (n_rays + PB_CHUNK - 1) / PB_CHUNK;
    const int64_t blocks = (waves + PB_WAVES - 1) / PB_WAVES;
    if (blocks > 0x7fffffff) return NGP_EINVAL;
    hipLaunchKernelGGL(pose_rays_bwd_kernel, dim3((unsigned)blocks), dim3(64 * PB_WAVES), 0, (hipStream_t)stream, g_x, g_dir,
                       ts, rays_a, poses, dR, directions, img_idxs, pix_idxs, n_imgs, n_pix, n_rays, n, g_dR, g_dT);
    return ngp_check_launch();
}

int ngp_sh_bwd_dirs(const float* d, const float* dL_dy, int64_t lddy, int64_t n, float* dL_dd, void* stream)
{
    if (n < 0) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!d || !dL_dy || !dL_dd || lddy < 16) return NGP_EINVAL;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffff) return NGP_EINVAL;
    hipLaunchKernelGGL(sh_bwd_dirs_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d, dL_dy, lddy, n, dL_dd);
    return ngp_check_launch();
}

} // extern "C"
