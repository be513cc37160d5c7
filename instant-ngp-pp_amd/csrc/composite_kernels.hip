// Ray-segment kernels: alpha compositing (train fw/bw, alpha-only, test), Ref-NeRF normal
// regularisers, distortion loss, segment_csr.
//
// Layout: one 32-lane half-wave per rays_a row.  The lanes of a half-wave take 32
// consecutive samples of the ray (coalesced loads), the transmittance T_k = prod(1-a_j) is a
// multiplicative scan across the lanes, early termination is a ballot on T <= T_threshold,
// and per-ray outputs are one cross-lane reduction at the end.  The reference walks each ray
// serially in one thread (volumerendering.cu:84-114 etc.).
//
// Differences from the serial walk are confined to fp32 summation/product association.
#include "common.h"

namespace {

struct Seg {
    int64_t ray, start;
    int n;
};

__device__ __forceinline__ bool seg_load(const int64_t* __restrict__ rays_a, int n_rays, Seg& s, int& lane32)
{
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = gtid >> 5;
    lane32 = threadIdx.x & 31;
    if (row >= n_rays) return false;
    s.ray = rays_a[3 * (size_t)row];
    s.start = rays_a[3 * (size_t)row + 1];
    s.n = (int)rays_a[3 * (size_t)row + 2];
    return true;
}

// Per-chunk transmittance bookkeeping shared by all compositing kernels.
struct Chunk {
    float a, T_before, T_after;
    bool valid, active;
    int first; // lane of the stopping sample inside this chunk, or -1
};

__device__ __forceinline__ Chunk chunk_alpha(const float* __restrict__ sigmas, const float* __restrict__ deltas,
                                             int64_t s, bool valid, float T_run, float T_thr, int lane32)
{
    Chunk c;
    c.valid = valid;
    const float sig = valid ? sigmas[s] : 0.0f;
    const float dl = valid ? deltas[s] : 0.0f;
    c.a = valid ? 1.0f - __expf(-sig * dl) : 0.0f;
    const float om = 1.0f - c.a;
    const float pin = half_incl_scan_mul(om, lane32);
    float pex = __shfl_up(pin, 1, 32);
    if (lane32 == 0) pex = 1.0f;
    c.T_before = T_run * pex;
    c.T_after = T_run * pin;
    const bool stopped = valid && (c.T_after <= T_thr);
    c.first = half_first(__ballot(stopped), threadIdx.x & 63);
    c.active = valid && (c.first < 0 || lane32 <= c.first);
    return c;
}

// ------------------------------------------------------------------ composite_alpha_fw
__global__ void composite_alpha_fw_kernel(const float* __restrict__ sigmas, const float* __restrict__ deltas,
                                          const int64_t* __restrict__ rays_a, float T_thr, int n_rays,
                                          float* __restrict__ alphas, float* __restrict__ ws)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    float T_run = 1.0f;
    int k0 = 0;
    for (; k0 < sg.n; k0 += 32) {
        const int k = k0 + lane;
        const int64_t s = sg.start + k;
        const Chunk c = chunk_alpha(sigmas, deltas, s, k < sg.n, T_run, T_thr, lane);
        if (c.valid) { alphas[s] = c.active ? c.a : 0.0f; ws[s] = c.active ? c.a * c.T_before : 0.0f; }
        if (c.first >= 0) { k0 += 32; break; }
        T_run = __shfl(c.T_after, 31, 32);
    }
    for (; k0 < sg.n; k0 += 32) {
        const int k = k0 + lane;
        if (k < sg.n) { alphas[sg.start + k] = 0.0f; ws[sg.start + k] = 0.0f; }
    }
}

// ------------------------------------------------------------------ composite_train_fw (V1)
template <int CMAX>
__global__ void composite_train_fw_kernel(const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                          const float* __restrict__ normals, const float* __restrict__ sems,
                                          const float* __restrict__ deltas, const float* __restrict__ ts,
                                          const int64_t* __restrict__ rays_a, float T_thr, int classes, int n_rays,
                                          int64_t* __restrict__ total_samples, float* __restrict__ opacity,
                                          float* __restrict__ depth, float* __restrict__ rgb,
                                          float* __restrict__ normal, float* __restrict__ sem, float* __restrict__ ws)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    float T_run = 1.0f;
    float aO = 0, aD = 0, aR = 0, aG = 0, aB = 0, aNx = 0, aNy = 0, aNz = 0;
    float aS[CMAX > 0 ? CMAX : 1];
#pragma unroll
    for (int c = 0; c < CMAX; c++) aS[c] = 0;
    int stop = -1;
    int k0 = 0;
    for (; k0 < sg.n; k0 += 32) {
        const int k = k0 + lane;
        const int64_t s = sg.start + k;
        const Chunk c = chunk_alpha(sigmas, deltas, s, k < sg.n, T_run, T_thr, lane);
        const float w = c.active ? c.a * c.T_before : 0.0f;
        if (c.valid) {
            ws[s] = w;
            aO += w;
            aD += w * ts[s];
            aR += w * rgbs[3 * s]; aG += w * rgbs[3 * s + 1]; aB += w * rgbs[3 * s + 2];
            aNx += w * normals[3 * s]; aNy += w * normals[3 * s + 1]; aNz += w * normals[3 * s + 2];
#pragma unroll
            for (int cc = 0; cc < CMAX; cc++)
                if (cc < classes) aS[cc] += w * sems[s * classes + cc];
        }
        if (c.first >= 0) { stop = k0 + c.first; k0 += 32; break; }
        T_run = __shfl(c.T_after, 31, 32);
    }
    for (; k0 < sg.n; k0 += 32) { // samples behind the stop: zero weight
        const int k = k0 + lane;
        if (k < sg.n) ws[sg.start + k] = 0.0f;
    }
    aO = half_sum(aO); aD = half_sum(aD);
    aR = half_sum(aR); aG = half_sum(aG); aB = half_sum(aB);
    aNx = half_sum(aNx); aNy = half_sum(aNy); aNz = half_sum(aNz);
#pragma unroll
    for (int cc = 0; cc < CMAX; cc++)
        if (cc < classes) aS[cc] = half_sum(aS[cc]);
    if (lane == 0) {
        const size_t r = (size_t)sg.ray;
        total_samples[r] = stop >= 0 ? stop : sg.n;
        opacity[r] = aO; depth[r] = aD;
        rgb[3 * r] = aR; rgb[3 * r + 1] = aG; rgb[3 * r + 2] = aB;
        normal[3 * r] = aNx; normal[3 * r + 1] = aNy; normal[3 * r + 2] = aNz;
#pragma unroll
        for (int cc = 0; cc < CMAX; cc++)
            if (cc < classes) sem[r * classes + cc] = aS[cc];
    }
}

// ------------------------------------------------------------------ composite_train_bw (V2)
template <int CMAX>
__global__ void composite_train_bw_kernel(const float* __restrict__ dL_dopacity, const float* __restrict__ dL_ddepth,
                                          const float* __restrict__ dL_drgb, const float* __restrict__ dL_dnormal,
                                          const float* __restrict__ dL_dsem, const float* __restrict__ dL_dws,
                                          const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                          const float* __restrict__ ws, const float* __restrict__ deltas,
                                          const float* __restrict__ ts, const int64_t* __restrict__ rays_a,
                                          const float* __restrict__ opacity, const float* __restrict__ depth,
                                          const float* __restrict__ rgb, float T_thr, int classes, int n_rays,
                                          float* __restrict__ dL_dsigmas, float* __restrict__ dL_drgbs,
                                          float* __restrict__ dL_dnormals, float* __restrict__ dL_dsems)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    if (sg.n <= 0) return;
    const size_t r = (size_t)sg.ray;
    const float R = rgb[3 * r], G = rgb[3 * r + 1], B = rgb[3 * r + 2];
    const float O = opacity[r], D = depth[r];
    // a NULL upstream gradient is an all-zero one (outputs the loss never touched)
    float gR = 0.0f, gG = 0.0f, gB = 0.0f;
    if (dL_drgb) { gR = dL_drgb[3 * r]; gG = dL_drgb[3 * r + 1]; gB = dL_drgb[3 * r + 2]; }
    const float gO = dL_dopacity ? dL_dopacity[r] : 0.0f, gD = dL_ddepth ? dL_ddepth[r] : 0.0f;
    float gNx = 0.0f, gNy = 0.0f, gNz = 0.0f;
    if (dL_dnormals) { gNx = dL_dnormal[3 * r]; gNy = dL_dnormal[3 * r + 1]; gNz = dL_dnormal[3 * r + 2]; }
    float gS[CMAX > 0 ? CMAX : 1];
#pragma unroll
    for (int cc = 0; cc < CMAX; cc++) gS[cc] = (dL_dsems && cc < classes) ? dL_dsem[r * classes + cc] : 0.0f;

    // total of dL_dws*ws over the whole segment (volumerendering.cu:206-210)
    float tot = 0.0f;
    if (dL_dws) {
        for (int k = lane; k < sg.n; k += 32) tot += dL_dws[sg.start + k] * ws[sg.start + k];
        tot = half_sum(tot);
    }

    float T_run = 1.0f, r_run = 0, g_run = 0, b_run = 0, d_run = 0, p_run = 0;
    int k0 = 0;
    for (; k0 < sg.n; k0 += 32) {
        const int k = k0 + lane;
        const int64_t s = sg.start + k;
        const Chunk c = chunk_alpha(sigmas, deltas, s, k < sg.n, T_run, T_thr, lane);
        const float w = c.valid ? c.a * c.T_before : 0.0f;
        float cr = 0, cg = 0, cb = 0, tt = 0, dws = 0, dl = 0, wsv = 0;
        if (c.valid) {
            cr = rgbs[3 * s]; cg = rgbs[3 * s + 1]; cb = rgbs[3 * s + 2];
            tt = ts[s]; dws = dL_dws ? dL_dws[s] : 0.0f; dl = deltas[s]; wsv = ws[s];
        }
        const float ri = r_run + half_incl_scan_add(w * cr, lane);
        const float gi = g_run + half_incl_scan_add(w * cg, lane);
        const float bi = b_run + half_incl_scan_add(w * cb, lane);
        const float di = d_run + half_incl_scan_add(w * tt, lane);
        const float pi = p_run + half_incl_scan_add(dws * wsv, lane);
        if (c.valid) {
            const float wa = c.active ? w : 0.0f;
            dL_drgbs[3 * s] = gR * wa; dL_drgbs[3 * s + 1] = gG * wa; dL_drgbs[3 * s + 2] = gB * wa;
            if (dL_dnormals) {
                dL_dnormals[3 * s] = gNx * wa; dL_dnormals[3 * s + 1] = gNy * wa; dL_dnormals[3 * s + 2] = gNz * wa;
            }
            if (dL_dsems) {
#pragma unroll
                for (int cc = 0; cc < CMAX; cc++)
                    if (cc < classes) dL_dsems[s * classes + cc] = gS[cc] * wa;
            }
            const float T = c.T_after;
            const float v = dl * (gR * (cr * T - (R - ri)) +
                                  gG * (cg * T - (G - gi)) +
                                  gB * (cb * T - (B - bi)) +
                                  gO * (1 - O) +
                                  gD * (tt * T - (D - di)) +
                                  T * dws - (tot - pi));
            dL_dsigmas[s] = c.active ? v : 0.0f;
        }
        if (c.first >= 0) { k0 += 32; break; }
        T_run = __shfl(c.T_after, 31, 32);
        r_run = __shfl(ri, 31, 32); g_run = __shfl(gi, 31, 32); b_run = __shfl(bi, 31, 32);
        d_run = __shfl(di, 31, 32); p_run = __shfl(pi, 31, 32);
    }
    for (; k0 < sg.n; k0 += 32) {
        const int k = k0 + lane;
        if (k < sg.n) {
            const int64_t s = sg.start + k;
            dL_dsigmas[s] = 0.0f;
            dL_drgbs[3 * s] = 0.0f; dL_drgbs[3 * s + 1] = 0.0f; dL_drgbs[3 * s + 2] = 0.0f;
            if (dL_dnormals) { dL_dnormals[3 * s] = 0.0f; dL_dnormals[3 * s + 1] = 0.0f; dL_dnormals[3 * s + 2] = 0.0f; }
            if (dL_dsems) for (int cc = 0; cc < classes; cc++) dL_dsems[s * classes + cc] = 0.0f;
        }
    }
}

// Generic-classes fallbacks (classes > 32): semantic channels handled by a second sweep that
// re-derives w from the ws written by the first sweep.
__global__ void composite_sem_fw_kernel(const float* __restrict__ ws, const float* __restrict__ sems,
                                        const int64_t* __restrict__ rays_a, int classes, int n_rays,
                                        float* __restrict__ sem)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    for (int cc = 0; cc < classes; cc++) {
        float a = 0.0f;
        for (int k = lane; k < sg.n; k += 32) a += ws[sg.start + k] * sems[(sg.start + k) * classes + cc];
        a = half_sum(a);
        if (lane == 0) sem[(size_t)sg.ray * classes + cc] = a;
    }
}

__global__ void composite_sem_bw_kernel(const float* __restrict__ dL_dsem, const float* __restrict__ w_eff,
                                        const int64_t* __restrict__ rays_a, int classes, int n_rays,
                                        float* __restrict__ dL_dsems)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    for (int k = lane; k < sg.n; k += 32) {
        const int64_t s = sg.start + k;
        const float w = w_eff[s];
        for (int cc = 0; cc < classes; cc++) dL_dsems[s * classes + cc] = dL_dsem[(size_t)sg.ray * classes + cc] * w;
    }
}

// ------------------------------------------------------------------ composite_test_fw (T1)
// One lane per alive ray (<= 64 samples per call, volumerendering.cu:335-373).
__global__ void composite_test_fw_kernel(const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                         const float* __restrict__ normals, const float* __restrict__ normals_raw,
                                         const float* __restrict__ sems, const float* __restrict__ deltas,
                                         const float* __restrict__ ts, int64_t* __restrict__ alive, float T_thr,
                                         int classes, const int32_t* __restrict__ n_eff, int n_alive, int n_samples,
                                         float* __restrict__ opacity, float* __restrict__ depth,
                                         float* __restrict__ rgb, float* __restrict__ normal,
                                         float* __restrict__ normal_raw, float* __restrict__ sem)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_alive) return;
    const int ne = n_eff[n];
    if (ne == 0) { alive[n] = -1; return; }
    const size_t r = (size_t)alive[n];
    // accumulators start from the running per-ray values so that the additions happen in the
    // reference's order (volumerendering.cu:352-365 adds sample by sample into the outputs)
    float aO = opacity[r], aD = depth[r];
    float T = 1 - aO;
    float aR = rgb[3 * r], aG = rgb[3 * r + 1], aB = rgb[3 * r + 2];
    float nx = normal[3 * r], ny = normal[3 * r + 1], nz = normal[3 * r + 2];
    float rx = normal_raw[3 * r], ry = normal_raw[3 * r + 1], rz = normal_raw[3 * r + 2];
    int s = 0;
    bool dead = false;
    while (s < ne) {
        const size_t o = (size_t)n * n_samples + s;
        const float a = 1.0f - __expf(-sigmas[o] * deltas[o]);
        const float w = a * T;
        aR += w * rgbs[3 * o]; aG += w * rgbs[3 * o + 1]; aB += w * rgbs[3 * o + 2];
        aD += w * ts[o]; aO += w;
        nx += w * normals[3 * o]; ny += w * normals[3 * o + 1]; nz += w * normals[3 * o + 2];
        rx += w * normals_raw[3 * o]; ry += w * normals_raw[3 * o + 1]; rz += w * normals_raw[3 * o + 2];
        for (int c = 0; c < classes; c++) sem[r * classes + c] += w * sems[o * classes + c];
        T *= 1.0f - a;
        if (T <= T_thr) { dead = true; break; }
        s++;
    }
    rgb[3 * r] = aR; rgb[3 * r + 1] = aG; rgb[3 * r + 2] = aB;
    depth[r] = aD; opacity[r] = aO;
    normal[3 * r] = nx; normal[3 * r + 1] = ny; normal[3 * r + 2] = nz;
    normal_raw[3 * r] = rx; normal_raw[3 * r + 1] = ry; normal_raw[3 * r + 2] = rz;
    if (dead) alive[n] = -1;
}

// ------------------------------------------------------------------ RefLoss (V3)
__global__ void refloss_fw_kernel(const float* __restrict__ sigmas, const float* __restrict__ ndiff,
                                  const float* __restrict__ nori, const float* __restrict__ deltas,
                                  const int64_t* __restrict__ rays_a, float T_thr, int n_rays,
                                  float* __restrict__ loss_o, float* __restrict__ loss_p)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    float T_run = 1.0f, ao = 0, ax = 0, ay = 0, az = 0;
    for (int k0 = 0; k0 < sg.n; k0 += 32) {
        const int k = k0 + lane;
        const int64_t s = sg.start + k;
        const Chunk c = chunk_alpha(sigmas, deltas, s, k < sg.n, T_run, T_thr, lane);
        if (c.active) {
            const float w = c.a * c.T_before;
            ax += w * ndiff[3 * s]; ay += w * ndiff[3 * s + 1]; az += w * ndiff[3 * s + 2];
            ao += w * nori[s];
        }
        if (c.first >= 0) break;
        T_run = __shfl(c.T_after, 31, 32);
    }
    ao = half_sum(ao); ax = half_sum(ax); ay = half_sum(ay); az = half_sum(az);
    if (lane == 0) {
        const size_t r = (size_t)sg.ray;
        loss_o[r] = ao; loss_p[3 * r] = ax; loss_p[3 * r + 1] = ay; loss_p[3 * r + 2] = az;
    }
}

__global__ void refloss_bw_kernel(const float* __restrict__ dL_dlo, const float* __restrict__ dL_dlp,
                                  const float* __restrict__ sigmas, const float* __restrict__ ndiff,
                                  const float* __restrict__ nori, const float* __restrict__ deltas,
                                  const int64_t* __restrict__ rays_a, const float* __restrict__ loss_o,
                                  const float* __restrict__ loss_p, float T_thr, int n_rays,
                                  float* __restrict__ dL_dsigmas, float* __restrict__ dL_dndiff,
                                  float* __restrict__ dL_dnori)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    const size_t r = (size_t)sg.ray;
    const float X = loss_p[3 * r], Y = loss_p[3 * r + 1], Z = loss_p[3 * r + 2], O = loss_o[r];
    const float gx = dL_dlp[3 * r], gy = dL_dlp[3 * r + 1], gz = dL_dlp[3 * r + 2], go = dL_dlo[r];
    float T_run = 1.0f, x_run = 0, y_run = 0, z_run = 0, o_run = 0;
    int k0 = 0;
    for (; k0 < sg.n; k0 += 32) {
        const int k = k0 + lane;
        const int64_t s = sg.start + k;
        const Chunk c = chunk_alpha(sigmas, deltas, s, k < sg.n, T_run, T_thr, lane);
        const float w = c.valid ? c.a * c.T_before : 0.0f;
        float dx = 0, dy = 0, dz = 0, no = 0, dl = 0;
        if (c.valid) { dx = ndiff[3 * s]; dy = ndiff[3 * s + 1]; dz = ndiff[3 * s + 2]; no = nori[s]; dl = deltas[s]; }
        const float xi = x_run + half_incl_scan_add(w * dx, lane);
        const float yi = y_run + half_incl_scan_add(w * dy, lane);
        const float zi = z_run + half_incl_scan_add(w * dz, lane);
        const float oi = o_run + half_incl_scan_add(w * no, lane);
        if (c.valid) {
            const float wa = c.active ? w : 0.0f;
            dL_dndiff[3 * s] = gx * wa; dL_dndiff[3 * s + 1] = gy * wa; dL_dndiff[3 * s + 2] = gz * wa;
            dL_dnori[s] = go * wa;
            const float T = c.T_after;
            const float v = dl * (gx * (dx * T - (X - xi)) + gy * (dy * T - (Y - yi)) + gz * (dz * T - (Z - zi)) +
                                  go * (no * T - (O - oi)));
            dL_dsigmas[s] = c.active ? v : 0.0f;
        }
        if (c.first >= 0) { k0 += 32; break; }
        T_run = __shfl(c.T_after, 31, 32);
        x_run = __shfl(xi, 31, 32); y_run = __shfl(yi, 31, 32); z_run = __shfl(zi, 31, 32); o_run = __shfl(oi, 31, 32);
    }
    for (; k0 < sg.n; k0 += 32) {
        const int k = k0 + lane;
        if (k < sg.n) {
            const int64_t s = sg.start + k;
            dL_dsigmas[s] = 0.0f; dL_dnori[s] = 0.0f;
            dL_dndiff[3 * s] = 0.0f; dL_dndiff[3 * s + 1] = 0.0f; dL_dndiff[3 * s + 2] = 0.0f;
        }
    }
}

// ------------------------------------------------------------------ distortion loss (D1)
__global__ void distortion_fw_kernel(const float* __restrict__ ws, const float* __restrict__ deltas,
                                     const float* __restrict__ ts, const int64_t* __restrict__ rays_a, int n_rays,
                                     float* __restrict__ loss, float* __restrict__ ws_inc, float* __restrict__ wts_inc)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    float w_run = 0, wt_run = 0, acc = 0;
    for (int k0 = 0; k0 < sg.n; k0 += 32) {
        const int k = k0 + lane;
        const int64_t s = sg.start + k;
        const bool valid = k < sg.n;
        const float w = valid ? ws[s] : 0.0f;
        const float wt = valid ? w * ts[s] : 0.0f;
        const float wi = w_run + half_incl_scan_add(w, lane);
        const float wti = wt_run + half_incl_scan_add(wt, lane);
        float we = __shfl_up(wi, 1, 32), wte = __shfl_up(wti, 1, 32);
        if (lane == 0) { we = w_run; wte = wt_run; }
        if (valid) {
            ws_inc[s] = wi; wts_inc[s] = wti;
            acc += 2 * (wti * we - wi * wte) + 1.0f / 3 * w * w * deltas[s];
        }
        w_run = __shfl(wi, 31, 32); wt_run = __shfl(wti, 31, 32);
    }
    acc = half_sum(acc);
    if (lane == 0) loss[(size_t)sg.ray] = acc;
}

__global__ void distortion_bw_kernel(const float* __restrict__ dL_dloss, const float* __restrict__ ws_inc,
                                     const float* __restrict__ wts_inc, const float* __restrict__ ws,
                                     const float* __restrict__ deltas, const float* __restrict__ ts,
                                     const int64_t* __restrict__ rays_a, int n_rays, float* __restrict__ dL_dws)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    if (sg.n <= 0) return; // the reference reads start-1 here (losses.cu:125-128)
    const int64_t end = sg.start + sg.n - 1;
    const float w_sum = ws_inc[end], wt_sum = wts_inc[end];
    const float g = dL_dloss[(size_t)sg.ray];
    for (int k = lane; k < sg.n; k += 32) {
        const int64_t s = sg.start + k;
        const float t = ts[s];
        const float left = (k == 0) ? 0.0f : (t * ws_inc[s - 1] - wts_inc[s - 1]);
        float v = g * 2 * (left + (wt_sum - wts_inc[s] - t * (w_sum - ws_inc[s])));
        v += g * 2.0f / 3 * ws[s] * deltas[s];
        dL_dws[s] = v;
    }
}

// ------------------------------------------------------------------ segment_csr sum (R4)
__global__ void segment_csr_kernel(const float* __restrict__ src, const int64_t* __restrict__ indptr, int n_seg,
                                   int width, float* __restrict__ out)
{
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x;
    const int seg = gtid >> 5, lane = threadIdx.x & 31;
    if (seg >= n_seg) return;
    const int64_t b = indptr[seg], e = indptr[seg + 1];
    for (int c = 0; c < width; c++) {
        float a = 0.0f;
        for (int64_t k = b + lane; k < e; k += 32) a += src[k * width + c];
        a = half_sum(a);
        if (lane == 0) out[(size_t)seg * width + c] = a;
    }
}

// ------------------------------------------------------------------ fused loss / glue kernels
// NeRFLoss default terms (losses.py:96-105, reduced as train.py:307 does: sum of term means) with the
// gradients of the rgb / opacity terms, one pass over the rays:
//   terms[1] += mean (rgb-gt)^2                    d_rgb     = 2 (rgb-gt) / (3 n)
//   terms[2] += lambda_o mean(-o log o), o=op+1e-10 d_opacity = lambda_o (-log o - 1) / n
//   terms[3] += lambda_d mean(dist)                (dist = per-ray distortion loss, may be NULL)
//   terms[0] += their sum
__global__ void __launch_bounds__(256) nerf_loss_kernel(const float* __restrict__ rgb, const float* __restrict__ gt,
                                                        const float* __restrict__ opacity,
                                                        const float* __restrict__ dist, int n_rays, float g_rgb,
                                                        float g_op, float g_dist, float* __restrict__ terms,
                                                        float* __restrict__ d_rgb, float* __restrict__ d_opacity)
{
    __shared__ float part[3][4];
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    if (r < n_rays) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float e = rgb[3 * r + c] - gt[3 * r + c];
            s0 += e * e;
            d_rgb[3 * r + c] = g_rgb * 2.0f * e;
        }
        const float o = opacity[r] + 1e-10f;
        const float lg = logf(o);
        s1 = -o * lg;
        d_opacity[r] = g_op * (-lg - 1.0f);
        if (dist) s2 = dist[r];
    }
#pragma unroll   // wave_sum of the three, interleaved: the text the kernel's compiled shape was measured with
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = s0; part[1][threadIdx.x >> 6] = s1; part[2][threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float t_rgb = (part[0][0] + part[0][1] + part[0][2] + part[0][3]) * g_rgb;
        const float t_op = (part[1][0] + part[1][1] + part[1][2] + part[1][3]) * g_op;
        const float t_dist = (part[2][0] + part[2][1] + part[2][2] + part[2][3]) * g_dist;
        atomicAdd(terms, t_rgb + t_op + t_dist);
        atomicAdd(terms + 1, t_rgb);
        atomicAdd(terms + 2, t_op);
        atomicAdd(terms + 3, t_dist);
    }
}

// ------------------------------------------------------------------ fused render + default loss + its gradients
// Everything between the field's raw outputs and the field's backward on the default recipe (rendering.py:221-249,
// losses.py:96-105, train.py:307), per ray, in ONE launch (it replaces -normalize x2, softmax, composite_train_fw,
// the RefLoss inputs + forward, distortion fw/bw, the loss and composite_train_bw: 12 launches on a serial chain):
//   pass A  compositing with early stop: ws, opacity, depth, rgb, normal_pred, semantic, total_samples, Ro, Rp, and the
//           distortion loss of the ray (running inclusive scans of w and w t);
//           per-sample normals (-normalize of d sigma/dx and of the head's output) and softmax live in registers only;
//   seeds   d_rgb = 2 (rgb - gt) / (3 R), d_opacity = lambda_o (-log o - 1) / R, d_dist = lambda_d / R; loss terms;
//   pass B  tot = sum_s dL_dws[s] ws[s] (distortion backward in closed form, losses.cu:130-139);
//   pass C  composite_train_bw's scans: dL_dsigmas, dL_drgbs (volumerendering.cu:193-245; normal / semantic terms do not
//           enter dL_dsigma there, and their own gradients are zero on this recipe).
// Every lane re-reads only what the SAME lane wrote (ws), the scans are recomputed: no cross-lane traffic through memory.
struct RenderLossArgs {
    const float *sigmas, *rgbs, *dsig_dx, *np_raw, *sem_logits, *dirs, *deltas, *ts, *gt, *scale3;
    const float* bg;   // optional (3): background colour, rgb += bg (1 - opacity) (rendering.py:236-241)
    const int64_t* rays_a;
    int64_t ld_np, ld_sem;
    float T_thr, g_rgb, g_op, g_dist;
    int classes, n_rays;
    int64_t *total_samples, *vr_samples;
    float *opacity, *depth, *rgb, *normal, *sem, *ws, *Ro, *Rp, *terms, *d_sigmas, *d_rgbs;
    // MASKED only (NeRFLoss(embed_msk=True), losses.py:85-93): the transient mask of every ray, g_ms = size_delta / R,
    // and the loss's gradient w.r.t. the mask
    const float* mask;
    float g_ms;
    float* d_mask;
    // SEM only (NeRFLoss(semantic=True), losses.py:120-123): the label of every ray, the workspace (SemWs below, filled by
    // count_valid_labels_kernel ahead of this launch), lambda_sem, g_sky = lambda_sky / R, and the loss's gradient w.r.t.
    // the class logits, dense (n, classes)
    const int64_t* labels;
    int* sem_ws;
    float lam_sem, g_sky;
    float* d_sem;
    // NRM only (NeRFLoss's normal_mono term, losses.py:111-118): the target normal of every ray (all three components
    // exactly 0: the pixel has none), the workspace (NRM_WS_* below, cleared by the entry's fill), g_nm = lambda_nm / (3 R),
    // and the loss's gradient w.r.t. the normal head's raw output, dense (n, 3)
    const float* nrm_gt;
    int* nrm_ws;
    float g_nm;
    float* d_np;
    // DEP only (NeRFLoss's depth_mono term, losses.py:125-131): the raw monocular depth of every ray (z = depth / 25, valid
    // iff z > 0), the workspace (DEP_WS_* below: depth_fit_kernel leaves the batch's scale and shift there ahead of this
    // launch), g_dm = lambda_dm / R and the scene scale of the falloff exp(-D / scale)
    const float* dep_gt;
    int* dep_ws;
    float g_dm, dm_scale;
    // SKY only (use_skybox): bg is (n_rays_total, 3), one background colour per ray, and the loss's gradient w.r.t. it
    float* d_bg;
    // where the last workgroup puts the rounded normal_mono and depth_mono terms: terms[4] for the single entries,
    // terms[6] and terms[7] for ngp_render_loss_fused_multi (CELoss and sky_depth are terms[4], terms[5] in both)
    int slot_nm, slot_dm;
};

// The semantic tail's workspace, NGP_SEM_WS_INTS = 8 int32, 8-byte aligned: [0] n_valid, [2:4] and [4:6] two doubles, the
// batch's sums of CE_r and of [y == 4] exp(-D_r), [6] the number of workgroups that have added theirs.  The two new terms
// are means of O(1) values scaled by weights of 1e-1: summed with one float atomic per workgroup (as terms[0:4] are) they
// would carry a few ulps of the result in arrival order, more than a faithful float32 evaluation of the loss has.  The
// workgroups add doubles instead, and the last one to finish rounds the two sums once into terms[4], terms[5] and terms[0].
constexpr int SEM_WS_NVALID = 0, SEM_WS_SUMS = 2, SEM_WS_DONE = 6;

// number of rows whose ray carries a valid label (0 <= y < classes), and the rest of the workspace cleared: one workgroup,
// no atomics, so the workspace needs no fill of its own
__global__ void __launch_bounds__(1024) count_valid_labels_kernel(const int64_t* __restrict__ labels,
                                                                  const int64_t* __restrict__ rays_a, int n_rays, int classes,
                                                                  int* __restrict__ ws)
{
    __shared__ int part[16];
    int c = 0;
    for (int row = threadIdx.x; row < n_rays; row += 1024) {
        const int64_t y = labels[rays_a[3 * (size_t)row]];
        c += (y >= 0 && y < classes) ? 1 : 0;
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int q = 0; q < 16; q++) t += part[q];
#pragma unroll
        for (int q = 0; q < 8; q++) ws[q] = q == SEM_WS_NVALID ? t : 0;   // the sums and the workgroup count start at 0
    }
}

// MASKED: the colour term is mean (1 - m) e^2 (its seed, and through it the background's share of d_opacity, carry the
// factor 1 - m), terms[4] = size_delta mean m^2, d_mask = 2 size_delta m / R - sum_c e_c^2 / (3 R); the rendered outputs
// are those of the unmasked kernel.  With m = 0 and size_delta = 0 every product below is by 1.0 and every sum with 0.0.
// SEM: with y the ray's label (valid iff 0 <= y < classes; 256, 255, negative, ... are ignored and never index anything),
// S = sem (the composited probabilities) and n_valid the batch's count of valid labels,
//   terms[4] = lambda_sem sum_valid (logsumexp(S) - S_y) / n_valid   (nn.CrossEntropyLoss(ignore_index=256) on S; 0 when
//              n_valid == 0, where torch gives NaN), seed g_c = lambda_sem / n_valid (softmax(S)_c - [c == y]),
//   d_sem[s, j] = w_s p_sj (g_j - sum_c g_c p_sc) with p the per-sample softmax, recomputed in pass C; the weights are
//              constants of this term (composite_train_bw drops dL_dsem from dL_dsigma, volumerendering.cu:234-241),
//   terms[5] = lambda_sky / R sum [y == 4] exp(-depth) (the literal 4, losses.py:122), seed g_D = -g_sky [y == 4] exp(-D),
//              which enters d_sigmas as delta_s g_D (t_s T_s - (D - d_s)), d_s the inclusive prefix of w t: the scan pass C
//              forms for the distortion term anyway.
// NRM: with N = normal_pred (the composited head normals, pass A's aN*), g the ray's target normal, N^ = N / max(|N|, 1e-12)
// and g^ = g / max(|g|, 1e-12) (F.normalize's defaults) and a ray whose target is (0, 0, 0) left out of everything below,
//   terms[4] = lambda_nm / (3 R) sum_r sum_c (|N^_c - g^_c| - 0.1 N^_c g^_c)        (NeRFLoss._normal_mono, mean over R x 3)
//   seed q_c = lambda_nm / (3 R) (sign(N^_c - g^_c) - 0.1 g^_c), sign(0) = 0 (torch's abs backward),
//        g_N = (q - N^ <N^, q>) / |N| where |N| > 1e-12, else q / 1e-12 (the clamp is then the divisor: rays without weight),
//   d_np[s] = -(w_s / |h_s|) (g_N - h^ <h^, g_N>) with h the head's raw output of the sample and h^ = h / |h| where
//        |h| > 1e-6, else -w_s g_N / 1e-6; exactly 0 behind the stop, for a sample without weight and on a ray without
//        a target.  The weights are constants of this term (composite_train_bw drops dL_dnormal_pred from dL_dsigma,
//        volumerendering.cu:234-241): d_sigmas and d_rgbs are the default entry's.
// The term is summed in double through the workspace and rounded once by the last workgroup, as the SEM terms are.
constexpr int NRM_WS_SUM = 0, NRM_WS_DONE = 2;   // NGP_NRM_WS_INTS = 4 int32, 8-byte aligned: one double, the workgroup count
// DEP: with z_r = depth_gt_r / 25 (valid iff z_r > 0: zero, negative and NaN targets add nothing anywhere), D = depth and
// (a, b) the least-squares scale and shift of a D + b ~ z over the batch's valid rays (depth_fit_kernel below; D is a
// constant of the fit, a singular system gives (0, 0)),
//   terms[4] = lambda_dm / R sum_valid exp(-D / scale) (a D + b - z)^2     (NeRFLoss._depth_mono, mean over all R rays; the
//              falloff is a constant too),
//   seed g_D = lambda_dm / R [valid] exp(-D / scale) 2 a (a D + b - z), which enters d_sigmas as the sky term's depth seed
//              does: delta_s g_D (t_s T_s - (D - d_s)).  d_rgbs is the default entry's.
// The depth_mono workspace, NGP_DEP_WS_INTS = 18 int32, 8-byte aligned, cleared by the entry's fill:
//   [0:10]  five doubles, the valid rays' sums of D^2, D, 1, D z, z (depth_fit_kernel's workgroups add theirs)
//   [10:12] one double, the batch's sum of exp(-D / scale) (a D + b - z)^2 (the tail's workgroups add theirs)
//   [12] a, [13] b as float32 and [14] n_valid as int32: written by the last workgroup of depth_fit_kernel
//   [15]    workgroups of depth_fit_kernel that have added their sums
//   [16]    workgroups of the tail that have added theirs (a counter of its own: nothing is reset between the two launches)
//   [17]    unused (keeps the size a multiple of 8 bytes)
constexpr int DEP_WS_SUMS = 0, DEP_WS_TERM = 10, DEP_WS_A = 12, DEP_WS_B = 13, DEP_WS_NVALID = 14, DEP_WS_FIT_DONE = 15,
              DEP_WS_TAIL_DONE = 16;

// The fit of the depth_mono term: the composited depth of every ray by the tail's own decomposition (32 lanes per ray, the
// same chunks, stop rule and accumulation order of w t, so D is the tail's `depth` output bit for bit), the five sums of the
// normal equations added as doubles per workgroup, and the 2x2 system solved in double by the last workgroup to finish.
// No per-sample output, no host read: the tail that follows on the stream reads (a, b) from the workspace.
__global__ void __launch_bounds__(256) depth_fit_kernel(const float* __restrict__ sigmas, const float* __restrict__ deltas,
                                                        const float* __restrict__ ts, const int64_t* __restrict__ rays_a,
                                                        const float* __restrict__ depth_gt, int n_rays, float T_thr,
                                                        int* __restrict__ dep_ws)
{
    constexpr int RPB = 256 / 32;
    __shared__ float part_d[RPB], part_z[RPB];
    Seg sg; int lane;
    const bool have = seg_load(rays_a, n_rays, sg, lane);
    float aD = 0.0f, z = 0.0f;
    if (have) {
        float T_run = 1.0f;
        for (int k0 = 0; k0 < sg.n; k0 += 32) {
            const int k = k0 + lane;
            const int64_t s = sg.start + k;
            const Chunk c = chunk_alpha(sigmas, deltas, s, k < sg.n, T_run, T_thr, lane);
            const float w = c.active ? c.a * c.T_before : 0.0f;
            float tt = 0.0f;
            if (c.valid) tt = ts[s];
            {
                // the tail rounds w t before it adds (the product also feeds its distortion scans, so it is never
                // contracted into the sum): the same two roundings here
#pragma clang fp contract(off)
                if (c.active) aD += w * tt;
            }
            if (c.first >= 0) break;
            T_run = __shfl(c.T_after, 31, 32);
        }
        aD = half_sum(aD);
        z = depth_gt[sg.ray] / 25.0f;
    }
    if ((threadIdx.x & 31) == 0) {
        part_d[threadIdx.x / 32] = aD;
        part_z[threadIdx.x / 32] = z > 0.0f ? z : 0.0f;   // (0: the ray takes no part; NaN compares false)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s_dd = 0.0, s_d = 0.0, s_n = 0.0, s_dz = 0.0, s_z = 0.0;
        for (int q = 0; q < RPB; q++) {
            if (part_z[q] > 0.0f) {
                const double d = (double)part_d[q], t = (double)part_z[q];
                s_dd += d * d; s_d += d; s_n += 1.0; s_dz += d * t; s_z += t;
            }
        }
        double* sums = reinterpret_cast<double*>(dep_ws + DEP_WS_SUMS);
        if (s_n > 0.0) {
            atomicAdd(sums, s_dd); atomicAdd(sums + 1, s_d); atomicAdd(sums + 2, s_n);
            atomicAdd(sums + 3, s_dz); atomicAdd(sums + 4, s_z);
        }
        __threadfence();
        const unsigned done = atomicAdd(reinterpret_cast<unsigned*>(dep_ws + DEP_WS_FIT_DONE), 1u);
        if (done == gridDim.x - 1) {   // every workgroup's sums are in: solve by Cramer's rule
            __threadfence();
            const double a00 = atomicAdd(sums, 0.0), a01 = atomicAdd(sums + 1, 0.0), a11 = atomicAdd(sums + 2, 0.0);
            const double b0 = atomicAdd(sums + 3, 0.0), b1 = atomicAdd(sums + 4, 0.0);
            const double det = a00 * a11 - a01 * a01;
            float fa = 0.0f, fb = 0.0f;
            if (det != 0.0) {   // (no valid ray, one valid ray, ...: a singular system gives (0, 0))
                fa = (float)((a11 * b0 - a01 * b1) / det);
                fb = (float)((a00 * b1 - a01 * b0) / det);
            }
            dep_ws[DEP_WS_A] = __float_as_int(fa);
            dep_ws[DEP_WS_B] = __float_as_int(fb);
            dep_ws[DEP_WS_NVALID] = (int)a11;
        }
    }
}

// SKY: the background is a colour per ray, bg[3 r + c] (the skybox's, rendering.py:236-241), and the launch also writes the
// loss's gradient w.r.t. it, d_bg[r] = g_rgb (1 - opacity), for every row (a ray without samples: opacity 0, d_bg = g_rgb).
// Everything else is the default form's arithmetic on bg0..2.
template <int CMAX, bool MASKED, bool SEM, bool NRM, bool DEP, bool SKY = false>
__global__ void __launch_bounds__(256) render_loss_fused_kernel(RenderLossArgs p)
{
    static_assert(!(MASKED && (SEM || NRM || DEP)), "MASKED x SEM, MASKED x NRM and MASKED x DEP are not built");
    static_assert(!(SKY && (MASKED || SEM || NRM || DEP)), "SKY is built with the default terms only");
    // rays per block, a half-wave each (a whole wave per ray was measured: 144 us per launch in the step against 85 -
    // 83 VGPRs leave 5 waves per SIMD, so 8192 wave-sized rays no longer fit the chip at once)
    constexpr int RPB = 256 / 32;
    // one row of partials per active term behind the three of the default recipe: [ms] or [ce, sky][nm][dm]
    constexpr int ROW_SEM = 3, ROW_NRM = 3 + (SEM ? 2 : 0), ROW_DEP = ROW_NRM + (NRM ? 1 : 0);
    __shared__ float part[MASKED ? 4 : ROW_DEP + (DEP ? 1 : 0)][RPB];
    __shared__ unsigned long long part_n[RPB];
    Seg sg; int lane;
    const bool have = seg_load(p.rays_a, p.n_rays, sg, lane);
    float s_rgb = 0.0f, s_op = 0.0f, s_dist = 0.0f, s_ms = 0.0f, s_ce = 0.0f, s_sky = 0.0f, s_nm = 0.0f, s_dm = 0.0f;
    unsigned long long n_used = 0;
    const int n_valid = SEM ? p.sem_ws[SEM_WS_NVALID] : 0;
    const float fit_a = DEP ? __int_as_float(p.dep_ws[DEP_WS_A]) : 0.0f, fit_b = DEP ? __int_as_float(p.dep_ws[DEP_WS_B]) : 0.0f;
    if (have) {
        const size_t r = (size_t)sg.ray;
        const float sc0 = p.scale3 ? p.scale3[0] : 1.0f, sc1 = p.scale3 ? p.scale3[1] : 1.0f, sc2 = p.scale3 ? p.scale3[2] : 1.0f;
        // ---------------- pass A
        float T_run = 1.0f;
        float aO = 0, aD = 0, aR = 0, aG = 0, aB = 0, aNx = 0, aNy = 0, aNz = 0, aRo = 0, aPx = 0, aPy = 0, aPz = 0;
        float aS[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; c++) aS[c] = 0;
        float w_run = 0, wt_run = 0, dacc = 0;
        int stop = -1;
        int k0 = 0;
        for (; k0 < sg.n; k0 += 32) {
            const int k = k0 + lane;
            const int64_t s = sg.start + k;
            const Chunk c = chunk_alpha(p.sigmas, p.deltas, s, k < sg.n, T_run, p.T_thr, lane);
            const float w = c.active ? c.a * c.T_before : 0.0f;
            float tt = 0.0f, dl = 0.0f;
            if (c.valid) {
                p.ws[s] = w;
                tt = p.ts[s]; dl = p.deltas[s];
            }
            if (c.active) {   // samples behind the stop carry no weight: their normals / classes are not needed
                aO += w;
                {
                    // a rounded product, then the add, in every form: depth_fit_kernel composites the same depth and its
                    // (a, b) are only the tail's own if the two agree bit for bit
#pragma clang fp contract(off)
                    aD += w * tt;
                }
                aR += w * p.rgbs[3 * s]; aG += w * p.rgbs[3 * s + 1]; aB += w * p.rgbs[3 * s + 2];
                // normals_raw = -normalize(d sigma/dx * scale3), normals_pred = -normalize(head), eps 1e-6 (F.normalize)
                float gx = p.dsig_dx[3 * s] * sc0, gy = p.dsig_dx[3 * s + 1] * sc1, gz = p.dsig_dx[3 * s + 2] * sc2;
                float inv = -1.0f / fmaxf(sqrtf(gx * gx + gy * gy + gz * gz), 1e-6f);
                gx *= inv; gy *= inv; gz *= inv;
                float hx = p.np_raw[s * p.ld_np], hy = p.np_raw[s * p.ld_np + 1], hz = p.np_raw[s * p.ld_np + 2];
                inv = -1.0f / fmaxf(sqrtf(hx * hx + hy * hy + hz * hz), 1e-6f);
                hx *= inv; hy *= inv; hz *= inv;
                aNx += w * hx; aNy += w * hy; aNz += w * hz;
                // Ref-NeRF regularisers (rendering.py:243-245)
                const float ex = gx - hx, ey = gy - hy, ez = gz - hz;
                aPx += w * (ex * ex); aPy += w * (ey * ey); aPz += w * (ez * ez);
                const float dx = p.dirs[3 * s], dy = p.dirs[3 * s + 1], dz = p.dirs[3 * s + 2];
                const float dinv = 1.0f / fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-6f);
                const float dot = fmaxf((gx * dx + gy * dy + gz * dz) * dinv, 0.0f);
                aRo += w * (dot * dot);
                // softmax over the class logits
                float lg[CMAX], mx = -INFINITY;
#pragma unroll
                for (int cc = 0; cc < CMAX; cc++) {
                    lg[cc] = cc < p.classes ? p.sem_logits[s * p.ld_sem + cc] : -INFINITY;
                    mx = fmaxf(mx, lg[cc]);
                }
                float den = 0.0f;
#pragma unroll
                for (int cc = 0; cc < CMAX; cc++) { lg[cc] = cc < p.classes ? __expf(lg[cc] - mx) : 0.0f; den += lg[cc]; }
                const float winv = w / den;
#pragma unroll
                for (int cc = 0; cc < CMAX; cc++) aS[cc] += winv * lg[cc];
            }
            // distortion loss (losses.cu:8-59): inclusive scans of w and w t over the ray
            const float wt = w * tt;
            const float wi = w_run + half_incl_scan_add(w, lane);
            const float wti = wt_run + half_incl_scan_add(wt, lane);
            float we = __shfl_up(wi, 1, 32), wte = __shfl_up(wti, 1, 32);
            if (lane == 0) { we = w_run; wte = wt_run; }
            if (c.valid) dacc += 2 * (wti * we - wi * wte) + 1.0f / 3 * w * w * dl;
            w_run = __shfl(wi, 31, 32); wt_run = __shfl(wti, 31, 32);
            if (c.first >= 0) { stop = k0 + c.first; k0 += 32; break; }
            T_run = __shfl(c.T_after, 31, 32);
        }
        for (; k0 < sg.n; k0 += 32) {   // behind the stop: zero weight, zero gradients
            const int k = k0 + lane;
            if (k < sg.n) {
                const int64_t s = sg.start + k;
                p.ws[s] = 0.0f; p.d_sigmas[s] = 0.0f;
                p.d_rgbs[3 * s] = 0.0f; p.d_rgbs[3 * s + 1] = 0.0f; p.d_rgbs[3 * s + 2] = 0.0f;
                if (SEM) {
#pragma unroll
                    for (int cc = 0; cc < CMAX; cc++)
                        if (cc < p.classes) p.d_sem[s * p.classes + cc] = 0.0f;
                }
                if (NRM) { p.d_np[3 * s] = 0.0f; p.d_np[3 * s + 1] = 0.0f; p.d_np[3 * s + 2] = 0.0f; }
            }
        }
        const int n_live = stop >= 0 ? (stop / 32 + 1) * 32 : sg.n;   // passes B and C stop behind the stop sample's chunk
        aO = half_sum(aO); aD = half_sum(aD); aR = half_sum(aR); aG = half_sum(aG); aB = half_sum(aB);
        aNx = half_sum(aNx); aNy = half_sum(aNy); aNz = half_sum(aNz);
        aRo = half_sum(aRo); aPx = half_sum(aPx); aPy = half_sum(aPy); aPz = half_sum(aPz);
        dacc = half_sum(dacc);
#pragma unroll
        for (int cc = 0; cc < CMAX; cc++) aS[cc] = half_sum(aS[cc]);
        // ---------------- loss terms and gradient seeds of the ray
        // the image colour: composited colour over the background (black when bg == NULL)
        float fR = aR, fG = aG, fB = aB, bg0 = 0.0f, bg1 = 0.0f, bg2 = 0.0f;
        // (SKY: the ray's own colour; the entry has checked rgb_bg, and the test of the pointer stays so that this form's
        // arithmetic is laid out, and contracted, exactly as the constant background's)
        const float* bg = SKY ? p.bg + 3 * r : p.bg;
        if (bg) {
            bg0 = bg[0]; bg1 = bg[1]; bg2 = bg[2];
            const float rest = 1.0f - aO;
            fR = aR + bg0 * rest; fG = aG + bg1 * rest; fB = aB + bg2 * rest;
        }
        const float e0 = fR - p.gt[3 * r], e1 = fG - p.gt[3 * r + 1], e2 = fB - p.gt[3 * r + 2];
        float gR = p.g_rgb * 2.0f * e0, gG = p.g_rgb * 2.0f * e1, gB = p.g_rgb * 2.0f * e2;
        float mk = 0.0f, keep = 1.0f;
        if (MASKED) {
            mk = p.mask[r]; keep = 1.0f - mk;
            gR *= keep; gG *= keep; gB *= keep;
        }
        const float oo = aO + 1e-10f;
        const float lgo = logf(oo);
        // d loss / d opacity: the entropy term, and through the background's weight (1 - opacity)
        const float gO = p.g_op * (-lgo - 1.0f) - (gR * bg0 + gG * bg1 + gB * bg2);
        const float gd = p.g_dist;
        // SEM: the seeds of the class probabilities and of the depth (every lane holds the ray's sums)
        float gS[CMAX], gD = 0.0f, ce = 0.0f, sky = 0.0f;
        if (SEM) {
            const int64_t y = p.labels[r];
            const bool y_ok = y >= 0 && y < p.classes;
            const float gs = (y_ok && n_valid > 0) ? p.lam_sem / (float)n_valid : 0.0f;
            float mx = -INFINITY, den = 0.0f, Sy = 0.0f;
#pragma unroll
            for (int cc = 0; cc < CMAX; cc++)
                if (cc < p.classes) mx = fmaxf(mx, aS[cc]);
#pragma unroll
            for (int cc = 0; cc < CMAX; cc++) {
                gS[cc] = cc < p.classes ? expf(aS[cc] - mx) : 0.0f;
                den += gS[cc];
                if ((int64_t)cc == y) Sy = aS[cc];      // (a select per class: the label never indexes)
            }
            if (y_ok) ce = mx + logf(den) - Sy;
            const float ginv = gs / den;
#pragma unroll
            for (int cc = 0; cc < CMAX; cc++) gS[cc] = gS[cc] * ginv - ((int64_t)cc == y && y_ok ? gs : 0.0f);
            if (y == 4) sky = expf(-aD);
            gD = -p.g_sky * sky;
        }
        // NRM: the term of the ray and the seed of its composited normal (every lane holds the ray's sums)
        float gNx = 0.0f, gNy = 0.0f, gNz = 0.0f, nm = 0.0f;
        bool nm_live = false;
        if (NRM) {
            const float tx = p.nrm_gt[3 * r], ty = p.nrm_gt[3 * r + 1], tz = p.nrm_gt[3 * r + 2];
            nm_live = tx != 0.0f || ty != 0.0f || tz != 0.0f;   // (0, 0, 0): a pixel without a normal
            if (nm_live) {
                const float nl = sqrtf(aNx * aNx + aNy * aNy + aNz * aNz), nd = fmaxf(nl, 1e-12f);
                const float ux = aNx / nd, uy = aNy / nd, uz = aNz / nd;
                const float td = fmaxf(sqrtf(tx * tx + ty * ty + tz * tz), 1e-12f);
                const float vx = tx / td, vy = ty / td, vz = tz / td;
                const float ex = ux - vx, ey = uy - vy, ez = uz - vz;
                nm = (fabsf(ex) - 0.1f * ux * vx) + (fabsf(ey) - 0.1f * uy * vy) + (fabsf(ez) - 0.1f * uz * vz);
                const float qx = p.g_nm * ((ex > 0.0f ? 1.0f : ex < 0.0f ? -1.0f : 0.0f) - 0.1f * vx);
                const float qy = p.g_nm * ((ey > 0.0f ? 1.0f : ey < 0.0f ? -1.0f : 0.0f) - 0.1f * vy);
                const float qz = p.g_nm * ((ez > 0.0f ? 1.0f : ez < 0.0f ? -1.0f : 0.0f) - 0.1f * vz);
                if (nl > 1e-12f) {
                    const float uq = ux * qx + uy * qy + uz * qz;
                    gNx = (qx - ux * uq) / nl; gNy = (qy - uy * uq) / nl; gNz = (qz - uz * uq) / nl;
                } else {
                    gNx = qx / 1e-12f; gNy = qy / 1e-12f; gNz = qz / 1e-12f;
                }
            }
        }
        // DEP: the term of the ray and the seed of its depth (every lane holds the ray's sums).  With SEM the sky term's
        // seed is already in gD and the two add: pass C's one depth line then serves both terms.
        float dm = 0.0f;
        if (DEP) {
            const float z = p.dep_gt[r] / 25.0f;
            if (z > 0.0f) {   // (zero, negative, NaN: the ray has no depth)
                const float fall = expf(-aD / p.dm_scale), res = fit_a * aD + fit_b - z;
                dm = fall * (res * res);
                const float gdm = p.g_dm * fall * (2.0f * fit_a * res);
                gD = SEM ? gD + gdm : gdm;
            }
        }
        if (lane == 0) {
            p.total_samples[r] = stop >= 0 ? stop : sg.n;
            p.opacity[r] = aO; p.depth[r] = aD;
            p.rgb[3 * r] = fR; p.rgb[3 * r + 1] = fG; p.rgb[3 * r + 2] = fB;
            p.normal[3 * r] = aNx; p.normal[3 * r + 1] = aNy; p.normal[3 * r + 2] = aNz;
            p.Ro[r] = aRo; p.Rp[3 * r] = aPx; p.Rp[3 * r + 1] = aPy; p.Rp[3 * r + 2] = aPz;
#pragma unroll
            for (int cc = 0; cc < CMAX; cc++)
                if (cc < p.classes) p.sem[r * p.classes + cc] = aS[cc];
            s_rgb = e0 * e0 + e1 * e1 + e2 * e2; s_op = -oo * lgo; s_dist = dacc;
            if (MASKED) {
                p.d_mask[r] = 2.0f * p.g_ms * mk - p.g_rgb * s_rgb;
                s_rgb *= keep;
                s_ms = mk * mk;
            }
            if (SKY) {
                const float rest = 1.0f - aO;
                p.d_bg[3 * r] = gR * rest; p.d_bg[3 * r + 1] = gG * rest; p.d_bg[3 * r + 2] = gB * rest;
            }
            if (SEM) { s_ce = ce; s_sky = sky; }
            if (NRM) s_nm = nm;
            if (DEP) s_dm = dm;
            n_used = (unsigned long long)(stop >= 0 ? stop : sg.n);
        }
        const float w_sum = w_run, wt_sum = wt_run;
        // ---------------- pass B: tot = sum dL_dws ws  (dL_dws of the distortion term, closed form)
        float tot = 0.0f;
        if (gd != 0.0f) {
            float wr = 0, wtr = 0;
            for (int q0 = 0; q0 < n_live; q0 += 32) {
                const int k = q0 + lane;
                const int64_t s = sg.start + k;
                const bool valid = k < sg.n;
                const float w = valid ? p.ws[s] : 0.0f, tt = valid ? p.ts[s] : 0.0f, dl = valid ? p.deltas[s] : 0.0f;
                const float wi = wr + half_incl_scan_add(w, lane);
                const float wti = wtr + half_incl_scan_add(w * tt, lane);
                float we = __shfl_up(wi, 1, 32), wte = __shfl_up(wti, 1, 32);
                if (lane == 0) { we = wr; wte = wtr; }
                const float dws = gd * 2 * ((tt * we - wte) + (wt_sum - wti - tt * (w_sum - wi))) + gd * 2.0f / 3 * w * dl;
                tot += dws * w;
                wr = __shfl(wi, 31, 32); wtr = __shfl(wti, 31, 32);
            }
            tot = half_sum(tot);
        }
        // ---------------- pass C: composite_train_bw
        {
            float T2 = 1.0f, r_run = 0, g_run = 0, b_run = 0, p_run = 0, wr = 0, wtr = 0;
            for (int q0 = 0; q0 < n_live; q0 += 32) {
                const int k = q0 + lane;
                const int64_t s = sg.start + k;
                const Chunk c = chunk_alpha(p.sigmas, p.deltas, s, k < sg.n, T2, p.T_thr, lane);
                const float w = c.valid ? c.a * c.T_before : 0.0f;
                float cr = 0, cg = 0, cb = 0, tt = 0, dl = 0, wsv = 0;
                if (c.valid) {
                    cr = p.rgbs[3 * s]; cg = p.rgbs[3 * s + 1]; cb = p.rgbs[3 * s + 2];
                    tt = p.ts[s]; dl = p.deltas[s]; wsv = p.ws[s];
                }
                const float wi = wr + half_incl_scan_add(wsv, lane);
                const float wti = wtr + half_incl_scan_add(wsv * tt, lane);
                float we = __shfl_up(wi, 1, 32), wte = __shfl_up(wti, 1, 32);
                if (lane == 0) { we = wr; wte = wtr; }
                const float dws = gd != 0.0f ? gd * 2 * ((tt * we - wte) + (wt_sum - wti - tt * (w_sum - wi))) + gd * 2.0f / 3 * wsv * dl
                                             : 0.0f;
                const float ri = r_run + half_incl_scan_add(w * cr, lane);
                const float gi = g_run + half_incl_scan_add(w * cg, lane);
                const float bi = b_run + half_incl_scan_add(w * cb, lane);
                const float pi = p_run + half_incl_scan_add(dws * wsv, lane);
                if (c.valid) {
                    const float wa = c.active ? w : 0.0f;
                    p.d_rgbs[3 * s] = gR * wa; p.d_rgbs[3 * s + 1] = gG * wa; p.d_rgbs[3 * s + 2] = gB * wa;
                    const float T = c.T_after;
                    float v = dl * (gR * (cr * T - (aR - ri)) + gG * (cg * T - (aG - gi)) + gB * (cb * T - (aB - bi)) +
                                    gO * (1 - aO) + T * dws - (tot - pi));
                    if (SEM || DEP) v += dl * gD * (tt * T - (wt_sum - wti));
                    p.d_sigmas[s] = c.active ? v : 0.0f;
                    if (SEM) {
                        // the sample's softmax again (pass A kept none), then the softmax backward of the seeds
                        float pr[CMAX], mx = -INFINITY;
#pragma unroll
                        for (int cc = 0; cc < CMAX; cc++) {
                            pr[cc] = (c.active && cc < p.classes) ? p.sem_logits[s * p.ld_sem + cc] : -INFINITY;
                            mx = fmaxf(mx, pr[cc]);
                        }
                        float den = 0.0f, dot = 0.0f;
#pragma unroll
                        for (int cc = 0; cc < CMAX; cc++) {
                            pr[cc] = (c.active && cc < p.classes) ? __expf(pr[cc] - mx) : 0.0f;
                            den += pr[cc];
                            dot += gS[cc] * pr[cc];
                        }
                        const float winv = c.active ? wa / den : 0.0f;
                        dot = c.active ? dot / den : 0.0f;
#pragma unroll
                        for (int cc = 0; cc < CMAX; cc++)
                            if (cc < p.classes) p.d_sem[s * p.classes + cc] = winv * pr[cc] * (gS[cc] - dot);
                    }
                    if (NRM) {
                        // the head's raw output again (pass A kept none), then -normalize's backward of w g_N
                        float ox = 0.0f, oy = 0.0f, oz = 0.0f;
                        if (nm_live && wa != 0.0f) {
                            const float hx = p.np_raw[s * p.ld_np], hy = p.np_raw[s * p.ld_np + 1], hz = p.np_raw[s * p.ld_np + 2];
                            const float hl = sqrtf(hx * hx + hy * hy + hz * hz);
                            if (hl > 1e-6f) {
                                const float ux = hx / hl, uy = hy / hl, uz = hz / hl;
                                const float ug = ux * gNx + uy * gNy + uz * gNz, kk = -wa / hl;
                                ox = kk * (gNx - ux * ug); oy = kk * (gNy - uy * ug); oz = kk * (gNz - uz * ug);
                            } else {
                                const float kk = -wa / 1e-6f;
                                ox = kk * gNx; oy = kk * gNy; oz = kk * gNz;
                            }
                        }
                        p.d_np[3 * s] = ox; p.d_np[3 * s + 1] = oy; p.d_np[3 * s + 2] = oz;
                    }
                }
                if (c.first >= 0) break;
                T2 = __shfl(c.T_after, 31, 32);
                r_run = __shfl(ri, 31, 32); g_run = __shfl(gi, 31, 32); b_run = __shfl(bi, 31, 32); p_run = __shfl(pi, 31, 32);
                wr = __shfl(wi, 31, 32); wtr = __shfl(wti, 31, 32);
            }
        }
    }
    // ---------------- loss terms of the block's rays: one set of atomics per block
    const int hw = threadIdx.x / 32;
    if ((threadIdx.x & 31) == 0) {
        part[0][hw] = s_rgb; part[1][hw] = s_op; part[2][hw] = s_dist; part_n[hw] = n_used;
        if (MASKED) part[3][hw] = s_ms;
        if (SEM) { part[ROW_SEM][hw] = s_ce; part[ROW_SEM + 1][hw] = s_sky; }
        if (NRM) part[ROW_NRM][hw] = s_nm;
        if (DEP) part[ROW_DEP][hw] = s_dm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t0 = 0, t1 = 0, t2 = 0, t3 = 0;
        unsigned long long tn = 0;
        for (int q = 0; q < RPB; q++) { t0 += part[0][q]; t1 += part[1][q]; t2 += part[2][q]; tn += part_n[q]; }
        t0 *= p.g_rgb; t1 *= p.g_op; t2 *= p.g_dist;
        if (MASKED) {
            for (int q = 0; q < RPB; q++) t3 += part[3][q];
            t3 *= p.g_ms;
            atomicAdd(p.terms, (t0 + t1 + t2) + t3);
            atomicAdd(p.terms + 4, t3);
        } else if (SEM || NRM || DEP) {
            // the optional terms, one or several: each is summed in double into its own term's workspace slot, behind
            // ONE count of finished workgroups (that of the first term built: the SEM block's, else the NRM block's, else
            // the DEP block's tail counter); the last workgroup rounds every term once and adds their float sum to terms[0]
            atomicAdd(p.terms, t0 + t1 + t2);
            double* sem_sums = SEM ? reinterpret_cast<double*>(p.sem_ws + SEM_WS_SUMS) : nullptr;
            double* nrm_sum = NRM ? reinterpret_cast<double*>(p.nrm_ws + NRM_WS_SUM) : nullptr;
            double* dep_sum = DEP ? reinterpret_cast<double*>(p.dep_ws + DEP_WS_TERM) : nullptr;
            if (SEM) {
                double c_sum = 0.0, s_sum = 0.0;
                for (int q = 0; q < RPB; q++) { c_sum += (double)part[ROW_SEM][q]; s_sum += (double)part[ROW_SEM + 1][q]; }
                atomicAdd(sem_sums, c_sum);
                atomicAdd(sem_sums + 1, s_sum);
            }
            if (NRM) {
                double n_sum = 0.0;
                for (int q = 0; q < RPB; q++) n_sum += (double)part[ROW_NRM][q];
                atomicAdd(nrm_sum, n_sum);
            }
            if (DEP) {
                double d_sum = 0.0;
                for (int q = 0; q < RPB; q++) d_sum += (double)part[ROW_DEP][q];
                atomicAdd(dep_sum, d_sum);
            }
            __threadfence();
            int* cnt = SEM ? p.sem_ws + SEM_WS_DONE : NRM ? p.nrm_ws + NRM_WS_DONE : p.dep_ws + DEP_WS_TAIL_DONE;
            const unsigned done = atomicAdd(reinterpret_cast<unsigned*>(cnt), 1u);
            if (done == gridDim.x - 1) {   // every workgroup's sums are in: round them once
                __threadfence();
                float opt = 0.0f;
                if (SEM) {
                    const double ce_all = atomicAdd(sem_sums, 0.0), sky_all = atomicAdd(sem_sums + 1, 0.0);
                    const float t_ce = n_valid > 0 ? (float)(ce_all * ((double)p.lam_sem / (double)n_valid)) : 0.0f;
                    const float t_sky = (float)(sky_all * (double)p.g_sky);
                    p.terms[4] = t_ce;
                    p.terms[5] = t_sky;
                    opt = t_ce + t_sky;
                }
                if (NRM) {
                    const float t_nm = (float)(atomicAdd(nrm_sum, 0.0) * (double)p.g_nm);
                    p.terms[p.slot_nm] = t_nm;
                    opt = SEM ? opt + t_nm : t_nm;
                }
                if (DEP) {
                    const float t_dm = (float)(atomicAdd(dep_sum, 0.0) * (double)p.g_dm);
                    p.terms[p.slot_dm] = t_dm;
                    opt = (SEM || NRM) ? opt + t_dm : t_dm;
                }
                atomicAdd(p.terms, opt);
            }
        } else
            atomicAdd(p.terms, t0 + t1 + t2);
        atomicAdd(p.terms + 1, t0);
        atomicAdd(p.terms + 2, t1);
        atomicAdd(p.terms + 3, t2);
        atomicAdd(reinterpret_cast<unsigned long long*>(p.vr_samples), tn);
    }
}

// Inputs of RefLoss (rendering.py:243-245): normals_diff = (n_raw - n_pred)^2,
// normals_ori = max(<n_raw, normalize(dir)>, 0)^2
__global__ void refloss_inputs_kernel(const float* __restrict__ n_raw, const float* __restrict__ n_pred,
                                      const float* __restrict__ dirs, int64_t n, float* __restrict__ ndiff,
                                      float* __restrict__ nori)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float rx = n_raw[3 * i], ry = n_raw[3 * i + 1], rz = n_raw[3 * i + 2];
    const float ex = rx - n_pred[3 * i], ey = ry - n_pred[3 * i + 1], ez = rz - n_pred[3 * i + 2];
    ndiff[3 * i] = ex * ex; ndiff[3 * i + 1] = ey * ey; ndiff[3 * i + 2] = ez * ez;
    const float dx = dirs[3 * i], dy = dirs[3 * i + 1], dz = dirs[3 * i + 2];
    const float inv = 1.0f / fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-6f);
    const float dot = fmaxf((rx * dx + ry * dy + rz * dz) * inv, 0.0f);
    nori[i] = dot * dot;
}

// y = -normalize(x * scale, eps=1e-6)  (F.normalize semantics: x / max(|x|, eps)); rows of 3
__global__ void neg_normalize_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ scale3,
                                     int64_t n, float* __restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = x[i * ldx], b = x[i * ldx + 1], c = x[i * ldx + 2];
    if (scale3) { a *= scale3[0]; b *= scale3[1]; c *= scale3[2]; }
    const float inv = -1.0f / fmaxf(sqrtf(a * a + b * b + c * c), 1e-6f);
    y[3 * i] = a * inv; y[3 * i + 1] = b * inv; y[3 * i + 2] = c * inv;
}

// backward of y = -x/max(|x|,eps):  dx = -(g - u <u,g>)/|x| with u = x/|x|   (|x| > eps)
__global__ void neg_normalize_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ g,
                                         int64_t n, float* __restrict__ dx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = x[i * ldx], b = x[i * ldx + 1], c = x[i * ldx + 2];
    const float ga = g[3 * i], gb = g[3 * i + 1], gc = g[3 * i + 2];
    const float nrm = sqrtf(a * a + b * b + c * c);
    if (nrm > 1e-6f) {
        const float inv = 1.0f / nrm;
        const float ua = a * inv, ub = b * inv, uc = c * inv;
        const float dot = ua * ga + ub * gb + uc * gc;
        dx[3 * i] = -(ga - ua * dot) * inv; dx[3 * i + 1] = -(gb - ub * dot) * inv; dx[3 * i + 2] = -(gc - uc * dot) * inv;
    } else {
        dx[3 * i] = -ga * 1e6f; dx[3 * i + 1] = -gb * 1e6f; dx[3 * i + 2] = -gc * 1e6f;
    }
}

// backward of y = -x / max(|x|, eps) for one row, neg_normalize_bwd_kernel's arithmetic (the <= eps branch included)
__device__ __forceinline__ void neg_normalize_bwd_row(float a, float b, float c, float ga, float gb, float gc, float& da,
                                                      float& db, float& dc)
{
    const float nrm = sqrtf(a * a + b * b + c * c);
    if (nrm > 1e-6f) {
        const float inv = 1.0f / nrm;
        const float ua = a * inv, ub = b * inv, uc = c * inv;
        const float dot = ua * ga + ub * gb + uc * gc;
        da = -(ga - ua * dot) * inv; db = -(gb - ub * dot) * inv; dc = -(gc - uc * dot) * inv;
    } else {
        da = -ga * 1e6f; db = -gb * 1e6f; dc = -gc * 1e6f;
    }
}

// The Ro / Rp terms of NeRFLoss(normal_ref=True) behind a fused tail: the tail has left ws (RefLoss composites with
// detached sigmas: its weights are constants here), so the gradients of lambda_rp mean(Rp) + lambda_ro mean(Ro) w.r.t.
// d(sigma)/dx and the normal head's raw output are per-sample expressions.  32 lanes per rays_a row.
__global__ void normal_ref_tail_kernel(const float* __restrict__ dsig_dx, const float* __restrict__ scale3,
                                       const float* __restrict__ np_raw, int64_t ld_np, const float* __restrict__ dirs,
                                       const float* __restrict__ ws, const int64_t* __restrict__ rays_a, int n_rays,
                                       float g_rp, float g_ro, int add_head, float* __restrict__ d_grads,
                                       float* __restrict__ d_np)
{
    Seg sg; int lane;
    if (!seg_load(rays_a, n_rays, sg, lane)) return;
    const float sc0 = scale3 ? scale3[0] : 1.0f, sc1 = scale3 ? scale3[1] : 1.0f, sc2 = scale3 ? scale3[2] : 1.0f;
    for (int k = lane; k < sg.n; k += 32) {
        const int64_t s = sg.start + k;
        const float w = ws[s];
        const float Gp = g_rp * w, Go = g_ro * w;
        // normals_raw = -normalize(d sigma/dx * scale3), normals_pred = -normalize(head), eps 1e-6: the tail's own forms
        const float xx = dsig_dx[3 * s] * sc0, xy = dsig_dx[3 * s + 1] * sc1, xz = dsig_dx[3 * s + 2] * sc2;
        float inv = -1.0f / fmaxf(sqrtf(xx * xx + xy * xy + xz * xz), 1e-6f);
        const float gx = xx * inv, gy = xy * inv, gz = xz * inv;
        const float px = np_raw[s * ld_np], py = np_raw[s * ld_np + 1], pz = np_raw[s * ld_np + 2];
        inv = -1.0f / fmaxf(sqrtf(px * px + py * py + pz * pz), 1e-6f);
        const float hx = px * inv, hy = py * inv, hz = pz * inv;
        const float ex = gx - hx, ey = gy - hy, ez = gz - hz;
        float dx = dirs[3 * s], dy = dirs[3 * s + 1], dz = dirs[3 * s + 2];
        const float dinv = 1.0f / fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-6f);
        dx *= dinv; dy *= dinv; dz *= dinv;
        const float dot = fmaxf(gx * dx + gy * dy + gz * dz, 0.0f);
        const float tp = 2.0f * Gp, to = 2.0f * dot * Go;
        const float rx = ex * tp + dx * to, ry = ey * tp + dy * to, rz = ez * tp + dz * to;   // dL/d normals_raw
        float ax, ay, az;
        neg_normalize_bwd_row(xx, xy, xz, rx, ry, rz, ax, ay, az);
        d_grads[3 * s] = ax * sc0; d_grads[3 * s + 1] = ay * sc1; d_grads[3 * s + 2] = az * sc2;
        neg_normalize_bwd_row(px, py, pz, -ex * tp, -ey * tp, -ez * tp, ax, ay, az);         // dL/d normals_pred = -2 e G_p
        if (add_head) { d_np[3 * s] += ax; d_np[3 * s + 1] += ay; d_np[3 * s + 2] += az; }
        else { d_np[3 * s] = ax; d_np[3 * s + 1] = ay; d_np[3 * s + 2] = az; }
    }
}

// ref_terms = [lambda_rp mean(Rp), lambda_ro mean(Ro)] over the rays rays_a names (3 n_rays and n_rays values): one
// workgroup, a lane takes every 256th row in order, then a tree over the lanes: the same bits on every run
__global__ void __launch_bounds__(256) normal_ref_terms_kernel(const int64_t* __restrict__ rays_a, int n_rays,
                                                               const float* __restrict__ loss_o, const float* __restrict__ loss_p,
                                                               float lambda_rp, float lambda_ro, float* __restrict__ ref_terms)
{
    __shared__ double sp[256], so[256];
    double p = 0.0, o = 0.0;
    for (int i = threadIdx.x; i < n_rays; i += 256) {
        const size_t r = (size_t)rays_a[3 * (size_t)i];
        p += ((double)loss_p[3 * r] + (double)loss_p[3 * r + 1]) + (double)loss_p[3 * r + 2];
        o += (double)loss_o[r];
    }
    sp[threadIdx.x] = p; so[threadIdx.x] = o;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) { sp[threadIdx.x] += sp[threadIdx.x + h]; so[threadIdx.x] += so[threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ref_terms[0] = (float)((double)lambda_rp * sp[0] / (3.0 * (double)n_rays));
        ref_terms[1] = (float)((double)lambda_ro * so[0] / (double)n_rays);
    }
}

inline dim3 seg_grid(int n_rays) { return dim3(ngp_blocks((int64_t)n_rays * 32, 256)); }

} // namespace

extern "C" {

int ngp_composite_alpha_fw(const float* sigmas, const float* deltas, const int64_t* rays_a, float T_threshold,
                           int n_rays, float* alphas, float* ws, void* stream)
{
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!sigmas || !deltas || !rays_a || !alphas || !ws) return NGP_EINVAL;
    hipLaunchKernelGGL(composite_alpha_fw_kernel, seg_grid(n_rays), dim3(256), 0, (hipStream_t)stream,
                       sigmas, deltas, rays_a, T_threshold, n_rays, alphas, ws);
    return ngp_check_launch();
}

int ngp_composite_train_fw(const float* sigmas, const float* rgbs, const float* normals_pred, const float* sems,
                           const float* deltas, const float* ts, const int64_t* rays_a, float T_threshold,
                           int classes, int n_rays, int64_t* total_samples, float* opacity, float* depth,
                           float* rgb, float* normal_pred, float* sem, float* ws, void* stream)
{
    if (n_rays < 0 || classes < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!rays_a || !total_samples || !opacity || !depth || !rgb || !normal_pred || (classes && !sem)) return NGP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH_FW(CM, CL)                                                                                          \
    hipLaunchKernelGGL(composite_train_fw_kernel<CM>, seg_grid(n_rays), dim3(256), 0, st, sigmas, rgbs,            \
                       normals_pred, sems, deltas, ts, rays_a, T_threshold, CL, n_rays, total_samples, opacity,    \
                       depth, rgb, normal_pred, sem, ws)
    if (classes == 0) LAUNCH_FW(0, 0);
    else if (classes <= 8) LAUNCH_FW(8, classes);
    else if (classes <= 16) LAUNCH_FW(16, classes);
    else if (classes <= 32) LAUNCH_FW(32, classes);
    else {
        LAUNCH_FW(0, 0);
        hipLaunchKernelGGL(composite_sem_fw_kernel, seg_grid(n_rays), dim3(256), 0, st, ws, sems, rays_a, classes,
                           n_rays, sem);
    }
#undef LAUNCH_FW
    return ngp_check_launch();
}

int ngp_composite_train_bw(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb,
                           const float* dL_dnormal_pred, const float* dL_dsem, const float* dL_dws,
                           const float* sigmas, const float* rgbs, const float* normals_pred, const float* ws,
                           const float* deltas, const float* ts, const int64_t* rays_a, const float* opacity,
                           const float* depth, const float* rgb, const float* normal_pred, float T_threshold,
                           int classes, int n_rays, float* dL_dsigmas, float* dL_drgbs, float* dL_dnormals_pred,
                           float* dL_dsems, void* stream)
{
    (void)normals_pred; (void)normal_pred;
    if (n_rays < 0 || classes < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!rays_a || !dL_dsigmas || !dL_drgbs) return NGP_EINVAL;
    if ((dL_dnormals_pred && !dL_dnormal_pred) || (dL_dsems && classes && !dL_dsem)) return NGP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH_BW(CM, CL)                                                                                          \
    hipLaunchKernelGGL(composite_train_bw_kernel<CM>, seg_grid(n_rays), dim3(256), 0, st, dL_dopacity, dL_ddepth,  \
                       dL_drgb, dL_dnormal_pred, dL_dsem, dL_dws, sigmas, rgbs, ws, deltas, ts, rays_a, opacity,   \
                       depth, rgb, T_threshold, CL, n_rays, dL_dsigmas, dL_drgbs, dL_dnormals_pred, dL_dsems)
    if (classes == 0) LAUNCH_BW(0, 0);
    else if (classes <= 8) LAUNCH_BW(8, classes);
    else if (classes <= 16) LAUNCH_BW(16, classes);
    else if (classes <= 32) LAUNCH_BW(32, classes);
    else {
        // ws saved by the forward is exactly the effective weight (zero behind the stop)
        LAUNCH_BW(0, 0);
        if (dL_dsems)
            hipLaunchKernelGGL(composite_sem_bw_kernel, seg_grid(n_rays), dim3(256), 0, st, dL_dsem, ws, rays_a, classes,
                               n_rays, dL_dsems);
    }
#undef LAUNCH_BW
    return ngp_check_launch();
}

int ngp_composite_test_fw(const float* sigmas, const float* rgbs, const float* normals, const float* normals_raw,
                          const float* sems, const float* deltas, const float* ts, const float* hits_t,
                          int64_t* alive_indices, float T_threshold, int classes, const int32_t* n_eff_samples,
                          int n_alive, int n_samples, float* opacity, float* depth, float* rgb, float* normal,
                          float* normal_raw, float* sem, void* stream)
{
    (void)hits_t;
    if (n_alive < 0 || classes < 0 || n_samples < 1) return NGP_EINVAL;
    if (n_alive == 0) return NGP_OK;
    if (!sigmas || !rgbs || !normals || !normals_raw || !deltas || !ts || !alive_indices || !n_eff_samples ||
        !opacity || !depth || !rgb || !normal || !normal_raw || (classes && (!sem || !sems))) return NGP_EINVAL;
    hipLaunchKernelGGL(composite_test_fw_kernel, dim3(ngp_blocks(n_alive, 64)), dim3(64), 0, (hipStream_t)stream,
                       sigmas, rgbs, normals, normals_raw, sems, deltas, ts, alive_indices, T_threshold, classes,
                       n_eff_samples, n_alive, n_samples, opacity, depth, rgb, normal, normal_raw, sem);
    return ngp_check_launch();
}

int ngp_composite_refloss_fw(const float* sigmas, const float* normals_diff, const float* normals_ori,
                             const float* deltas, const float* ts, const int64_t* rays_a, float T_threshold,
                             int n_rays, float* loss_o, float* loss_p, void* stream)
{
    (void)ts;
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!rays_a || !loss_o || !loss_p) return NGP_EINVAL;
    hipLaunchKernelGGL(refloss_fw_kernel, seg_grid(n_rays), dim3(256), 0, (hipStream_t)stream, sigmas, normals_diff,
                       normals_ori, deltas, rays_a, T_threshold, n_rays, loss_o, loss_p);
    return ngp_check_launch();
}

int ngp_composite_refloss_bw(const float* dL_dloss_o, const float* dL_dloss_p, const float* sigmas,
                             const float* normals_diff, const float* normals_ori, const float* deltas,
                             const float* ts, const int64_t* rays_a, const float* loss_o, const float* loss_p,
                             float T_threshold, int n_rays, float* dL_dsigmas, float* dL_dnormals_diff,
                             float* dL_dnormals_ori, void* stream)
{
    (void)ts;
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!rays_a || !dL_dsigmas || !dL_dnormals_diff || !dL_dnormals_ori) return NGP_EINVAL;
    hipLaunchKernelGGL(refloss_bw_kernel, seg_grid(n_rays), dim3(256), 0, (hipStream_t)stream, dL_dloss_o, dL_dloss_p,
                       sigmas, normals_diff, normals_ori, deltas, rays_a, loss_o, loss_p, T_threshold, n_rays,
                       dL_dsigmas, dL_dnormals_diff, dL_dnormals_ori);
    return ngp_check_launch();
}

int ngp_distortion_loss_fw(const float* ws, const float* deltas, const float* ts, const int64_t* rays_a, int n_rays,
                           float* loss, float* ws_inclusive_scan, float* wts_inclusive_scan, void* stream)
{
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!rays_a || !loss || !ws_inclusive_scan || !wts_inclusive_scan) return NGP_EINVAL;
    hipLaunchKernelGGL(distortion_fw_kernel, seg_grid(n_rays), dim3(256), 0, (hipStream_t)stream, ws, deltas, ts,
                       rays_a, n_rays, loss, ws_inclusive_scan, wts_inclusive_scan);
    return ngp_check_launch();
}

int ngp_distortion_loss_bw(const float* dL_dloss, const float* ws_inclusive_scan, const float* wts_inclusive_scan,
                           const float* ws, const float* deltas, const float* ts, const int64_t* rays_a, int n_rays,
                           float* dL_dws, void* stream)
{
    if (n_rays < 0) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!rays_a || !dL_dloss || !dL_dws) return NGP_EINVAL;
    hipLaunchKernelGGL(distortion_bw_kernel, seg_grid(n_rays), dim3(256), 0, (hipStream_t)stream, dL_dloss,
                       ws_inclusive_scan, wts_inclusive_scan, ws, deltas, ts, rays_a, n_rays, dL_dws);
    return ngp_check_launch();
}

int ngp_nerf_loss(const float* rgb, const float* target_rgb, const float* opacity, const float* distortion,
                  int n_rays, float lambda_opacity, float lambda_distortion, float* terms, float* d_rgb,
                  float* d_opacity, void* stream)
{
    if (n_rays < 1 || !rgb || !target_rgb || !opacity || !terms || !d_rgb || !d_opacity) return NGP_EINVAL;
    hipLaunchKernelGGL(nerf_loss_kernel, dim3(ngp_blocks(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, rgb,
                       target_rgb, opacity, distortion, n_rays, 1.0f / (3.0f * n_rays), lambda_opacity / n_rays,
                       lambda_distortion / n_rays, terms, d_rgb, d_opacity);
    return ngp_check_launch();
}

// ---- the fused render + loss tail: seven entries on one host path: tail_args, tail_check with the entry's own extra checks,
// tail_clear, the pre-kernels (the label count, the depth fit), the entry's few fields, tail_launch.  The four entries with
// optional terms share one body for all of it (render_loss_fused_terms).

// the one place that fills RenderLossArgs from the arguments every entry shares; every optional field is set to "absent"
static RenderLossArgs tail_args(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                                const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                                const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                                const float* target_rgb, const float* rgb_bg, float T_threshold, int classes, int n_rays,
                                float lambda_opacity, float lambda_distortion, int64_t* total_samples, int64_t* vr_samples,
                                float* opacity, float* depth, float* rgb, float* normal_pred, float* sem, float* ws,
                                float* loss_o, float* loss_p, float* terms, float* dL_dsigmas, float* dL_drgbs)
{
    RenderLossArgs a;
    a.sigmas = sigmas; a.rgbs = rgbs; a.dsig_dx = dsigma_dx; a.np_raw = normal_head; a.sem_logits = sem_logits;
    a.dirs = dirs; a.deltas = deltas; a.ts = ts; a.gt = target_rgb; a.scale3 = scale3; a.rays_a = rays_a; a.bg = rgb_bg;
    a.ld_np = ld_normal; a.ld_sem = ld_sem; a.T_thr = T_threshold;
    a.g_rgb = 1.0f / (3.0f * n_rays); a.g_op = lambda_opacity / n_rays; a.g_dist = lambda_distortion / n_rays;
    a.classes = classes; a.n_rays = n_rays; a.total_samples = total_samples; a.vr_samples = vr_samples;
    a.opacity = opacity; a.depth = depth; a.rgb = rgb; a.normal = normal_pred; a.sem = sem; a.ws = ws;
    a.Ro = loss_o; a.Rp = loss_p; a.terms = terms; a.d_sigmas = dL_dsigmas; a.d_rgbs = dL_drgbs;
    a.mask = nullptr; a.g_ms = 0.0f; a.d_mask = nullptr;
    a.labels = nullptr; a.sem_ws = nullptr; a.lam_sem = a.g_sky = 0.0f; a.d_sem = nullptr;
    a.nrm_gt = nullptr; a.nrm_ws = nullptr; a.g_nm = 0.0f; a.d_np = nullptr;
    a.dep_gt = nullptr; a.dep_ws = nullptr; a.g_dm = 0.0f; a.dm_scale = 1.0f;
    a.d_bg = nullptr;
    a.slot_nm = a.slot_dm = 4;
    return a;
}

// The checks every entry shares, in the order every entry answers them: the ranges (a bad one is refused for an empty
// batch too), an empty batch is NGP_OK, then the pointers.  `ranges_ok` and `ptrs_ok` are the entry's own checks of either
// kind; TAIL_GO: neither refused nor empty, the entry goes on.
constexpr int TAIL_GO = 1;
static int tail_check(const RenderLossArgs& a, int classes_min, int classes_max, bool ranges_ok, bool ptrs_ok)
{
    if (!ranges_ok || a.n_rays < 0 || a.classes < classes_min || a.classes > classes_max || a.ld_np < 3 ||
        a.ld_sem < a.classes) return NGP_EINVAL;
    if (a.n_rays == 0) return NGP_OK;
    if (!ptrs_ok || !a.rays_a || !a.gt || !a.total_samples || !a.vr_samples || !a.opacity || !a.depth || !a.rgb ||
        !a.normal || (a.classes && !a.sem) || !a.Ro || !a.Rp || !a.terms) return NGP_EINVAL;
    return TAIL_GO;
}

// what the entries with an optional term ask on top: every gradient and ws, the workspace 8-byte aligned (it holds doubles)
static bool tail_trained_ok(const RenderLossArgs& a, const int* term_ws)
{
    return a.d_sigmas && a.d_rgbs && a.ws && term_ws && !(reinterpret_cast<uintptr_t>(term_ws) & 7);
}

// terms (n_terms floats), vr_samples (an int64) and the workspace (ws_ints int32; NULL: none to clear) start at 0.  One
// fill when vr_samples sits vr_at floats behind terms and the workspace ws_at floats behind them, else one fill each.
static int tail_clear(float* terms, size_t n_terms, size_t vr_at, int64_t* vr_samples, int* ws, size_t ws_at, size_t ws_ints,
                      hipStream_t st)
{
    char* base = reinterpret_cast<char*>(terms);
    if (reinterpret_cast<char*>(vr_samples) == base + vr_at * sizeof(float) &&
        (!ws || reinterpret_cast<char*>(ws) == base + ws_at * sizeof(float))) {
        if (hipMemsetAsync(terms, 0, (ws ? ws_at + ws_ints : vr_at + 2) * sizeof(float), st) != hipSuccess) return NGP_ELAUNCH;
        return NGP_OK;
    }
    if (hipMemsetAsync(terms, 0, n_terms * sizeof(float), st) != hipSuccess) return NGP_ELAUNCH;
    if (hipMemsetAsync(vr_samples, 0, sizeof(int64_t), st) != hipSuccess) return NGP_ELAUNCH;
    if (ws && hipMemsetAsync(ws, 0, ws_ints * sizeof(int), st) != hipSuccess) return NGP_ELAUNCH;
    return NGP_OK;
}

// the 14 instantiations of the tail: the default, the masked and the per-ray-background (a.d_bg set) one, and every
// non-empty set of the three optional terms, those with the semantic term at 8 and at 16 classes
static int tail_launch(bool masked, int term_mask, int classes, int n_rays, hipStream_t st, const RenderLossArgs& a)
{
    const dim3 grid = seg_grid(n_rays), block(256);
    if (a.d_bg) {
        hipLaunchKernelGGL((render_loss_fused_kernel<8, false, false, false, false, true>), grid, block, 0, st, a);
        return ngp_check_launch();
    }
#define NGP_TAIL(CM, M, S, N, D) hipLaunchKernelGGL((render_loss_fused_kernel<CM, M, S, N, D>), grid, block, 0, st, a)
    const bool wide = classes > 8;   // (only with SEM: the entries check it)
    switch (masked ? -1 : term_mask) {
    case -1: NGP_TAIL(8, true, false, false, false); break;
    case 0: NGP_TAIL(8, false, false, false, false); break;
    case NGP_TERM_SEM: if (wide) NGP_TAIL(16, false, true, false, false); else NGP_TAIL(8, false, true, false, false); break;
    case NGP_TERM_NRM: NGP_TAIL(8, false, false, true, false); break;
    case NGP_TERM_DEP: NGP_TAIL(8, false, false, false, true); break;
    case NGP_TERM_SEM | NGP_TERM_NRM:
        if (wide) NGP_TAIL(16, false, true, true, false); else NGP_TAIL(8, false, true, true, false); break;
    case NGP_TERM_SEM | NGP_TERM_DEP:
        if (wide) NGP_TAIL(16, false, true, false, true); else NGP_TAIL(8, false, true, false, true); break;
    case NGP_TERM_NRM | NGP_TERM_DEP: NGP_TAIL(8, false, false, true, true); break;
    default: if (wide) NGP_TAIL(16, false, true, true, true); else NGP_TAIL(8, false, true, true, true); break;
    }
#undef NGP_TAIL
    return ngp_check_launch();
}

// shared body of ngp_render_loss_fused / ngp_render_loss_fused_masked (mask == NULL: the unmasked kernel, 4 terms)
static int render_loss_fused_launch(RenderLossArgs a, const float* mask, float size_delta, float* dL_dmask, void* stream)
{
    const int rc = tail_check(a, 0, 8, true, true);
    if (rc != TAIL_GO) return rc;
    hipStream_t st = (hipStream_t)stream;
    // (an int64 behind 5 floats sits at float 6)
    if (tail_clear(a.terms, mask ? 5 : 4, mask ? 6 : 4, a.vr_samples, nullptr, 0, 0, st) != NGP_OK) return NGP_ELAUNCH;
    a.mask = mask; a.g_ms = size_delta / a.n_rays; a.d_mask = dL_dmask;
    return tail_launch(mask != nullptr, 0, a.classes, a.n_rays, st, a);
}

int ngp_render_loss_fused(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                          const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                          const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                          const float* target_rgb, const float* rgb_bg, float T_threshold, int classes, int n_rays, float lambda_opacity,
                          float lambda_distortion, int64_t* total_samples, int64_t* vr_samples, float* opacity,
                          float* depth, float* rgb, float* normal_pred, float* sem, float* ws, float* loss_o,
                          float* loss_p, float* terms, float* dL_dsigmas, float* dL_drgbs, void* stream)
{
    return render_loss_fused_launch(
        tail_args(sigmas, rgbs, dsigma_dx, scale3, normal_head, ld_normal, sem_logits, ld_sem, dirs, deltas, ts, rays_a,
                  target_rgb, rgb_bg, T_threshold, classes, n_rays, lambda_opacity, lambda_distortion, total_samples,
                  vr_samples, opacity, depth, rgb, normal_pred, sem, ws, loss_o, loss_p, terms, dL_dsigmas, dL_drgbs),
        nullptr, 0.0f, nullptr, stream);
}

int ngp_render_loss_fused_sky(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                              const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                              const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                              const float* target_rgb, const float* rgb_bg, float T_threshold, int classes, int n_rays,
                              float lambda_opacity, float lambda_distortion, int64_t* total_samples, int64_t* vr_samples,
                              float* opacity, float* depth, float* rgb, float* normal_pred, float* sem, float* ws,
                              float* loss_o, float* loss_p, float* terms, float* dL_dsigmas, float* dL_drgbs,
                              float* dL_drgb_bg, void* stream)
{
    RenderLossArgs a = tail_args(sigmas, rgbs, dsigma_dx, scale3, normal_head, ld_normal, sem_logits, ld_sem, dirs, deltas, ts,
                                 rays_a, target_rgb, rgb_bg, T_threshold, classes, n_rays, lambda_opacity, lambda_distortion,
                                 total_samples, vr_samples, opacity, depth, rgb, normal_pred, sem, ws, loss_o, loss_p, terms,
                                 dL_dsigmas, dL_drgbs);
    const int rc = tail_check(a, 0, 8, true, rgb_bg && dL_drgb_bg);
    if (rc != TAIL_GO) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (tail_clear(a.terms, 4, 4, a.vr_samples, nullptr, 0, 0, st) != NGP_OK) return NGP_ELAUNCH;
    a.d_bg = dL_drgb_bg;
    return tail_launch(false, 0, a.classes, a.n_rays, st, a);
}

int ngp_render_loss_fused_masked(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                                 const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                                 const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                                 const float* target_rgb, const float* rgb_bg, const float* mask, float size_delta,
                                 float T_threshold, int classes, int n_rays, float lambda_opacity, float lambda_distortion,
                                 int64_t* total_samples, int64_t* vr_samples, float* opacity, float* depth, float* rgb,
                                 float* normal_pred, float* sem, float* ws, float* loss_o, float* loss_p, float* terms,
                                 float* dL_dsigmas, float* dL_drgbs, float* dL_dmask, void* stream)
{
    if (n_rays > 0 && (!mask || !dL_dmask)) return NGP_EINVAL;
    return render_loss_fused_launch(
        tail_args(sigmas, rgbs, dsigma_dx, scale3, normal_head, ld_normal, sem_logits, ld_sem, dirs, deltas, ts, rays_a,
                  target_rgb, rgb_bg, T_threshold, classes, n_rays, lambda_opacity, lambda_distortion, total_samples,
                  vr_samples, opacity, depth, rgb, normal_pred, sem, ws, loss_o, loss_p, terms, dL_dsigmas, dL_drgbs),
        mask, size_delta, dL_dmask, stream);
}

// The multi workspace, NGP_MULTI_WS_INTS = 30 int32, 8-byte aligned: the three single workspaces back to back
constexpr int MULTI_WS_NRM = NGP_SEM_WS_INTS, MULTI_WS_DEP = NGP_SEM_WS_INTS + NGP_NRM_WS_INTS;   // (the semantic one: at 0)
static_assert(MULTI_WS_DEP + NGP_DEP_WS_INTS == NGP_MULTI_WS_INTS && NGP_MULTI_WS_INTS % 2 == 0 && MULTI_WS_NRM % 2 == 0 &&
              MULTI_WS_DEP % 2 == 0, "the multi workspace is the three single ones, each 8-byte aligned");

// Where an entry with optional terms keeps what the launch accumulates into: terms (n_terms floats), vr_samples vr_at
// floats and the entry's workspace ws_at floats behind terms (an int64 behind 5 floats sits at float 6), how much of the
// workspace to clear (ws_clear int32; 0: none, the label count clears the semantic one), where the normal_mono and
// depth_mono blocks sit in it (the semantic block: at 0) and the slots of the two rounded terms.
struct TailLayout { size_t n_terms, vr_at, ws_at, ws_clear; int at_nrm, at_dep, slot_nm, slot_dm; };
constexpr TailLayout LAYOUT_SEM = {6, 6, 0, 0, 0, 0, 4, 4}, LAYOUT_NRM = {5, 6, 8, NGP_NRM_WS_INTS, 0, 0, 4, 4},
                     LAYOUT_DEP = {5, 6, 8, NGP_DEP_WS_INTS, 0, 0, 4, 4},
                     LAYOUT_MULTI = {8, 8, 10, NGP_MULTI_WS_INTS, MULTI_WS_NRM, MULTI_WS_DEP, 6, 7};

// shared body of ngp_render_loss_fused_sem / _nrm / _dep / _multi: term_mask names the terms to build, term_ws is the entry's
// workspace; the inputs and the gradient output of a term that is not built are not looked at (NULL)
static int render_loss_fused_terms(RenderLossArgs a, int term_mask, const int64_t* labels, float lambda_sem, float lambda_sky,
                                   const float* normals_gt, float lambda_nm, const float* depth_gt, float lambda_dm,
                                   float scene_scale, int* term_ws, float* dL_dsem_logits, float* dL_dnormal_head,
                                   const TailLayout& lay, void* stream)
{
    const bool SEM = term_mask & NGP_TERM_SEM, NRM = term_mask & NGP_TERM_NRM, DEP = term_mask & NGP_TERM_DEP;
    // (the semantic term's instantiations hold 1..16 classes, the others' 0..8)
    const int rc = tail_check(a, SEM ? 1 : 0, SEM ? 16 : 8, !DEP || scene_scale > 0.0f,
                              tail_trained_ok(a, term_ws) && (!SEM || (labels && a.sem_logits && dL_dsem_logits)) &&
                                  (!NRM || (normals_gt && a.np_raw && dL_dnormal_head)) && (!DEP || depth_gt));
    if (rc != TAIL_GO) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (tail_clear(a.terms, lay.n_terms, lay.vr_at, a.vr_samples, lay.ws_clear ? term_ws : nullptr, lay.ws_at, lay.ws_clear,
                   st) != NGP_OK) return NGP_ELAUNCH;
    int *sem_ws = term_ws, *nrm_ws = term_ws + lay.at_nrm, *dep_ws = term_ws + lay.at_dep;
    // what every seed needs of the whole batch, on the same stream ahead of the tail: n_valid, which depends on the labels
    // alone (the count also clears the semantic workspace), and the fit's scale and shift, which need every ray's depth
    if (SEM)
        hipLaunchKernelGGL(count_valid_labels_kernel, dim3(1), dim3(1024), 0, st, labels, a.rays_a, a.n_rays, a.classes, sem_ws);
    if (DEP)
        hipLaunchKernelGGL(depth_fit_kernel, seg_grid(a.n_rays), dim3(256), 0, st, a.sigmas, a.deltas, a.ts, a.rays_a, depth_gt,
                           a.n_rays, a.T_thr, dep_ws);
    a.slot_nm = lay.slot_nm; a.slot_dm = lay.slot_dm;
    if (SEM) { a.labels = labels; a.sem_ws = sem_ws; a.lam_sem = lambda_sem; a.g_sky = lambda_sky / a.n_rays; a.d_sem = dL_dsem_logits; }
    if (NRM) { a.nrm_gt = normals_gt; a.nrm_ws = nrm_ws; a.g_nm = lambda_nm / (3.0f * a.n_rays); a.d_np = dL_dnormal_head; }
    if (DEP) { a.dep_gt = depth_gt; a.dep_ws = dep_ws; a.g_dm = lambda_dm / a.n_rays; a.dm_scale = scene_scale; }
    return tail_launch(false, term_mask, a.classes, a.n_rays, st, a);
}

int ngp_render_loss_fused_sem(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                              const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                              const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                              const float* target_rgb, const float* rgb_bg, const int64_t* labels, float lambda_sem,
                              float lambda_sky, float T_threshold, int classes, int n_rays, float lambda_opacity,
                              float lambda_distortion, int64_t* total_samples, int64_t* vr_samples, float* opacity,
                              float* depth, float* rgb, float* normal_pred, float* sem, float* ws, float* loss_o,
                              float* loss_p, float* terms, float* dL_dsigmas, float* dL_drgbs, int* sem_ws,
                              float* dL_dsem_logits, void* stream)
{
    return render_loss_fused_terms(
        tail_args(sigmas, rgbs, dsigma_dx, scale3, normal_head, ld_normal, sem_logits, ld_sem, dirs, deltas, ts, rays_a,
                  target_rgb, rgb_bg, T_threshold, classes, n_rays, lambda_opacity, lambda_distortion, total_samples,
                  vr_samples, opacity, depth, rgb, normal_pred, sem, ws, loss_o, loss_p, terms, dL_dsigmas, dL_drgbs),
        NGP_TERM_SEM, labels, lambda_sem, lambda_sky, nullptr, 0.0f, nullptr, 0.0f, 1.0f, sem_ws, dL_dsem_logits, nullptr,
        LAYOUT_SEM, stream);
}

int ngp_render_loss_fused_nrm(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                              const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                              const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                              const float* target_rgb, const float* rgb_bg, const float* normals_gt, float lambda_nm,
                              float T_threshold, int classes, int n_rays, float lambda_opacity, float lambda_distortion,
                              int64_t* total_samples, int64_t* vr_samples, float* opacity, float* depth, float* rgb,
                              float* normal_pred, float* sem, float* ws, float* loss_o, float* loss_p, float* terms,
                              float* dL_dsigmas, float* dL_drgbs, int* nrm_ws, float* dL_dnormal_head, void* stream)
{
    return render_loss_fused_terms(
        tail_args(sigmas, rgbs, dsigma_dx, scale3, normal_head, ld_normal, sem_logits, ld_sem, dirs, deltas, ts, rays_a,
                  target_rgb, rgb_bg, T_threshold, classes, n_rays, lambda_opacity, lambda_distortion, total_samples,
                  vr_samples, opacity, depth, rgb, normal_pred, sem, ws, loss_o, loss_p, terms, dL_dsigmas, dL_drgbs),
        NGP_TERM_NRM, nullptr, 0.0f, 0.0f, normals_gt, lambda_nm, nullptr, 0.0f, 1.0f, nrm_ws, nullptr, dL_dnormal_head,
        LAYOUT_NRM, stream);
}

int ngp_render_loss_fused_dep(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                              const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                              const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                              const float* target_rgb, const float* rgb_bg, const float* depth_gt, float lambda_dm,
                              float scene_scale, float T_threshold, int classes, int n_rays, float lambda_opacity,
                              float lambda_distortion, int64_t* total_samples, int64_t* vr_samples, float* opacity,
                              float* depth, float* rgb, float* normal_pred, float* sem, float* ws, float* loss_o,
                              float* loss_p, float* terms, float* dL_dsigmas, float* dL_drgbs, int* dep_ws, void* stream)
{
    return render_loss_fused_terms(
        tail_args(sigmas, rgbs, dsigma_dx, scale3, normal_head, ld_normal, sem_logits, ld_sem, dirs, deltas, ts, rays_a,
                  target_rgb, rgb_bg, T_threshold, classes, n_rays, lambda_opacity, lambda_distortion, total_samples,
                  vr_samples, opacity, depth, rgb, normal_pred, sem, ws, loss_o, loss_p, terms, dL_dsigmas, dL_drgbs),
        NGP_TERM_DEP, nullptr, 0.0f, 0.0f, nullptr, 0.0f, depth_gt, lambda_dm, scene_scale, dep_ws, nullptr, nullptr,
        LAYOUT_DEP, stream);
}

int ngp_render_loss_fused_multi(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                                const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                                const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                                const float* target_rgb, const float* rgb_bg, int term_mask, const int64_t* labels,
                                float lambda_sem, float lambda_sky, const float* normals_gt, float lambda_nm,
                                const float* depth_gt, float lambda_dm, float scene_scale, float T_threshold, int classes,
                                int n_rays, float lambda_opacity, float lambda_distortion, int64_t* total_samples,
                                int64_t* vr_samples, float* opacity, float* depth, float* rgb, float* normal_pred,
                                float* sem, float* ws, float* loss_o, float* loss_p, float* terms, float* dL_dsigmas,
                                float* dL_drgbs, int* multi_ws, float* dL_dsem_logits, float* dL_dnormal_head, void* stream)
{
    // (a zero mask names nothing to compute: refused with rays to process; an empty batch is valid whatever it names)
    if (term_mask < 0 || (term_mask & ~(NGP_TERM_SEM | NGP_TERM_NRM | NGP_TERM_DEP)) || (term_mask == 0 && n_rays != 0))
        return NGP_EINVAL;
    // (a term's workspace is its block of multi_ws; one bit alone launches that term's own instantiation)
    return render_loss_fused_terms(
        tail_args(sigmas, rgbs, dsigma_dx, scale3, normal_head, ld_normal, sem_logits, ld_sem, dirs, deltas, ts, rays_a,
                  target_rgb, rgb_bg, T_threshold, classes, n_rays, lambda_opacity, lambda_distortion, total_samples,
                  vr_samples, opacity, depth, rgb, normal_pred, sem, ws, loss_o, loss_p, terms, dL_dsigmas, dL_drgbs),
        term_mask, labels, lambda_sem, lambda_sky, normals_gt, lambda_nm, depth_gt, lambda_dm, scene_scale,
        multi_ws, dL_dsem_logits, dL_dnormal_head, LAYOUT_MULTI, stream);
}

int ngp_refloss_inputs(const float* normals_raw, const float* normals_pred, const float* dirs, int64_t n,
                       float* normals_diff, float* normals_ori, void* stream)
{
    if (n < 0) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!normals_raw || !normals_pred || !dirs || !normals_diff || !normals_ori) return NGP_EINVAL;
    hipLaunchKernelGGL(refloss_inputs_kernel, dim3(ngp_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, normals_raw,
                       normals_pred, dirs, n, normals_diff, normals_ori);
    return ngp_check_launch();
}

int ngp_neg_normalize(const float* x, int64_t ldx, const float* scale3, int64_t n, float* y, void* stream)
{
    if (n < 0 || ldx < 3) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!x || !y) return NGP_EINVAL;
    hipLaunchKernelGGL(neg_normalize_kernel, dim3(ngp_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx,
                       scale3, n, y);
    return ngp_check_launch();
}

int ngp_neg_normalize_bwd(const float* x, int64_t ldx, const float* dL_dy, int64_t n, float* dL_dx, void* stream)
{
    if (n < 0 || ldx < 3) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!x || !dL_dy || !dL_dx) return NGP_EINVAL;
    hipLaunchKernelGGL(neg_normalize_bwd_kernel, dim3(ngp_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx,
                       dL_dy, n, dL_dx);
    return ngp_check_launch();
}

int ngp_normal_ref_tail(const float* dsigma_dx, const float* scale3, const float* normal_head, int64_t ld_normal_head,
                        const float* dirs, const float* ws, const int64_t* rays_a, int n_rays, const float* loss_o,
                        const float* loss_p, float lambda_rp, float lambda_ro, int add_to_normal_head, float* dL_dgrads,
                        float* dL_dnormal_head, float* ref_terms, void* stream)
{
    if (n_rays < 0 || ld_normal_head < 3) return NGP_EINVAL;
    if (n_rays == 0) return NGP_OK;
    if (!dsigma_dx || !normal_head || !dirs || !ws || !rays_a || !loss_o || !loss_p || !dL_dgrads || !dL_dnormal_head ||
        !ref_terms)
        return NGP_EINVAL;
    hipLaunchKernelGGL(normal_ref_tail_kernel, seg_grid(n_rays), dim3(256), 0, (hipStream_t)stream, dsigma_dx, scale3,
                       normal_head, ld_normal_head, dirs, ws, rays_a, n_rays, lambda_rp / (3.0f * (float)n_rays),
                       lambda_ro / (float)n_rays, add_to_normal_head, dL_dgrads, dL_dnormal_head);
    if (ngp_check_launch() != NGP_OK) return NGP_ELAUNCH;
    hipLaunchKernelGGL(normal_ref_terms_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rays_a, n_rays, loss_o, loss_p,
                       lambda_rp, lambda_ro, ref_terms);
    return ngp_check_launch();
}

int ngp_segment_csr_sum(const float* src, const int64_t* indptr, int n_seg, int width, float* out, void* stream)
{
    if (n_seg < 0 || width < 1) return NGP_EINVAL;
    if (n_seg == 0) return NGP_OK;
    if (!indptr || !out) return NGP_EINVAL;
    hipLaunchKernelGGL(segment_csr_kernel, seg_grid(n_seg), dim3(256), 0, (hipStream_t)stream, src, indptr, n_seg,
                       width, out);
    return ngp_check_launch();
}

} // extern "C"
