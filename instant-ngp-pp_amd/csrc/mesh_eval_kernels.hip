// Mesh evaluation (M4 of include/ngp_hip.h): area-weighted surface samples, a uniform grid of triangle references and
// the exact closest-triangle query on it: mesh.py sample_surface / closest_on_mesh / mesh_distance, tools/eval_mesh.py.
// Built with -ffp-contract=off: the samples, the cell coordinates and the squared distances are the f32 expressions
// of the numpy restatement (tests/mesh_eval_reference.py), bit for bit.
//
// Sampler: one thread per sample, a pure function of (seed, i): three hashed words pick the face (binary search of
// the caller's cdf in double) and the barycentric pair (folded at r1 + r2 > 1, no square root).
//
// Grid: a dense grid in compressed-row form.  Count and fill run one thread per face over the box of cells its
// corners span and use integer atomicAdd only; a thread learns about the others only through what its atomics return
// (another workgroup's plain stores may not be visible inside a launch: per-CU L1s and per-XCD L2s are not
// coherent), and the tables are read by later launches.  The order inside a cell is whatever the atomics gave.
//
// Query: one thread per point (the caller sorts the points by cell, so neighbouring lanes walk the same cells and
// their triangle loads are broadcasts served by L2).  From the point's own cell coordinate c (unclamped: the point
// may lie outside the grid) the thread visits the cells of Chebyshev distance r = r0, r0 + 1, ... (r0: the first ring
// that meets the grid), each ring clipped to the grid, and keeps the smallest (d2, face) pair, so neither the grid nor
// the order inside a cell shows in the result.
//
// The walk, its stop rule and its ring cap: ring_walk.h (shared with the point clouds of cloud_kernels.hip).
#include "common.h"
#include "ring_walk.h"

#include <math.h>

namespace {

constexpr int ME_BLOCK = 256;                 // threads per workgroup (4 waves)
constexpr int64_t ME_MAX_SAMPLES = 1 << 30;   // 3 i + 3 stays below 2^32
enum { ME_ERR_FINITE = 1, ME_ERR_OUTSIDE = 2 };

__device__ __forceinline__ uint32_t me_fmix32(uint32_t h)   // the 32-bit finaliser of MurmurHash3
{
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

__global__ void __launch_bounds__(ME_BLOCK) me_sample_kernel(const float* __restrict__ verts,
                                                             const int32_t* __restrict__ faces, int n_faces,
                                                             const double* __restrict__ cdf, double total, int64_t n,
                                                             uint32_t seed, float* __restrict__ points,
                                                             int32_t* __restrict__ face)
{
    const int64_t i = (int64_t)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t u[3];
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) u[k] = me_fmix32(seed + 0x9E3779B9u * (3u * (uint32_t)i + k + 1u));
    const double t = (((double)u[0] + 0.5) * 0x1p-32) * total;
    int lo = 0, hi = n_faces;   // first f with cdf[f] > t; each step halves hi - lo
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cdf[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    int last = 0, top = n_faces - 1;   // first f with cdf[f] >= total: the last face that added area
    while (last < top) {
        const int mid = last + (top - last) / 2;
        if (cdf[mid] >= total) top = mid;
        else last = mid + 1;
    }
    const int f = lo < last ? lo : last;
    float r1 = (float)(u[1] >> 8) * 0x1p-24f, r2 = (float)(u[2] >> 8) * 0x1p-24f;
    if (r1 + r2 > 1.f) {
        r1 = 1.f - r1;
        r2 = 1.f - r2;
    }
    const float* v0 = verts + 3 * (int64_t)faces[3 * (int64_t)f];
    const float* v1 = verts + 3 * (int64_t)faces[3 * (int64_t)f + 1];
    const float* v2 = verts + 3 * (int64_t)faces[3 * (int64_t)f + 2];
#pragma unroll
    for (int a = 0; a < 3; a++) points[3 * i + a] = (v0[a] + r1 * (v1[a] - v0[a])) + r2 * (v2[a] - v0[a]);
    face[i] = f;
}

// ------------------------------------------------------------------------------------------------------------ grid
// the box of cells [lo, hi] face f is referenced from; false: referenced nowhere (err says why, if it is an error)
__device__ __forceinline__ bool me_face_box(const float* __restrict__ verts, const int32_t* __restrict__ faces, int f,
                                            const MeGrid& G, int lo[3], int hi[3], int& err)
{
    float p[3][3];
    bool finite = true;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const float* v = verts + 3 * (int64_t)faces[3 * (int64_t)f + q];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            p[q][a] = v[a];
            finite &= isfinite(p[q][a]);
        }
    }
    if (!finite) {
        err |= ME_ERR_FINITE;
        return false;
    }
    const float e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const float e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const float n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2],
                n2 = e1[0] * e2[1] - e1[1] * e2[0];
    if (n0 == 0.f && n1 == 0.f && n2 == 0.f) return false;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float c0 = floorf((p[0][a] - G.o[a]) * G.inv), c1 = floorf((p[1][a] - G.o[a]) * G.inv),
                    c2 = floorf((p[2][a] - G.o[a]) * G.inv);
        const float mn = fminf(c0, fminf(c1, c2)), mx = fmaxf(c0, fmaxf(c1, c2));
        const float top = (float)(G.d[a] - 1);
        inside &= mn >= 0.f && mx <= top;
        lo[a] = (int)fminf(fmaxf(mn, 0.f), top);   // in the grid whatever the input
        hi[a] = (int)fminf(fmaxf(mx, 0.f), top);
    }
    if (!inside) {
        err |= ME_ERR_OUTSIDE;
        return false;
    }
    return true;
}

__global__ void __launch_bounds__(ME_BLOCK) me_zero_totals_kernel(unsigned long long* __restrict__ totals)
{
    if (threadIdx.x < 2) totals[threadIdx.x] = 0ull;
}

__global__ void __launch_bounds__(ME_BLOCK) me_grid_count_kernel(const float* __restrict__ verts,
                                                                 const int32_t* __restrict__ faces, int n_faces,
                                                                 MeGrid G, int32_t* __restrict__ cell_count,
                                                                 unsigned long long* __restrict__ totals)
{
    const int f = blockIdx.x * ME_BLOCK + threadIdx.x;
    int err = 0;
    unsigned long long refs = 0;
    int lo[3], hi[3];
    if (f < n_faces && me_face_box(verts, faces, f, G, lo, hi, err)) {
        for (int x = lo[0]; x <= hi[0]; x++)
            for (int y = lo[1]; y <= hi[1]; y++)
                for (int z = lo[2]; z <= hi[2]; z++) atomicAdd(&cell_count[me_cell_index(G, x, y, z)], 1);
        refs = (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned)(hi[1] - lo[1] + 1) * (unsigned)(hi[2] - lo[2] + 1);
    }
    // one pair of atomics per wave
#pragma unroll
    for (int o = NGP_WAVE / 2; o > 0; o >>= 1) {
        refs += __shfl_xor(refs, o, NGP_WAVE);
        err |= __shfl_xor(err, o, NGP_WAVE);
    }
    if ((threadIdx.x & (NGP_WAVE - 1)) == 0) {
        if (refs) atomicAdd(&totals[0], refs);
        if (err) atomicOr(&totals[1], (unsigned long long)err);
    }
}

__global__ void __launch_bounds__(ME_BLOCK) me_grid_fill_kernel(const float* __restrict__ verts,
                                                                const int32_t* __restrict__ faces, int n_faces,
                                                                MeGrid G, const int32_t* __restrict__ cell_offset,
                                                                int32_t* __restrict__ cell_cursor,
                                                                int32_t* __restrict__ cell_faces)
{
    const int f = blockIdx.x * ME_BLOCK + threadIdx.x;
    int err = 0;
    int lo[3], hi[3];
    if (f >= n_faces || !me_face_box(verts, faces, f, G, lo, hi, err)) return;
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int y = lo[1]; y <= hi[1]; y++)
            for (int z = lo[2]; z <= hi[2]; z++) {
                const int64_t cell = me_cell_index(G, x, y, z);
                const int at = atomicAdd(&cell_cursor[cell], 1);
                const int begin = cell_offset[cell];
                // a cursor that the caller did not zero, or offsets of another grid, must not write past the row
                if (at >= 0 && at < cell_offset[cell + 1] - begin) cell_faces[begin + at] = f;
            }
}

// ----------------------------------------------------------------------------------------------------------- query
__device__ __forceinline__ float me_dot(const float x[3], const float y[3])
{
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// squared distance from p to the triangle (a, b, c): the sequence of include/ngp_hip.h M4, operation for operation
__device__ __forceinline__ float me_tri_d2(const float p[3], const float a[3], const float b[3], const float c[3])
{
    float ab[3], ac[3], ap[3], bp[3], cp[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ab[k] = b[k] - a[k];
        ac[k] = c[k] - a[k];
        ap[k] = p[k] - a[k];
        bp[k] = p[k] - b[k];
        cp[k] = p[k] - c[k];
    }
    const float d1 = me_dot(ab, ap), d2 = me_dot(ac, ap);
    const float d3 = me_dot(ab, bp), d4 = me_dot(ac, bp);
    const float d5 = me_dot(ab, cp), d6 = me_dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.f && d2 <= 0.f) {
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = a[k];
    } else if (d3 >= 0.f && d4 <= d3) {
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = b[k];
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        const float v = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = a[k] + ab[k] * v;
    } else if (d6 >= 0.f && d5 <= d6) {
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = c[k];
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        const float w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = a[k] + ac[k] * w;
    } else if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) {
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = b[k] + (c[k] - b[k]) * w;
    } else {
        const float den = 1.f / ((va + vb) + vc);
        const float v = vb * den, w = vc * den;
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
    }
    const float e[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    return me_dot(e, e);
}

__global__ void __launch_bounds__(ME_BLOCK) me_clip_all_kernel(int64_t n, float md2, float* __restrict__ d2,
                                                               int32_t* __restrict__ face)
{
    const int64_t i = (int64_t)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (i >= n) return;
    d2[i] = md2;
    face[i] = -1;
}

__global__ void __launch_bounds__(ME_BLOCK) me_closest_kernel(const float* __restrict__ points, int64_t n,
                                                              const float* __restrict__ verts,
                                                              const int32_t* __restrict__ faces, MeGrid G,
                                                              const int32_t* __restrict__ cell_offset,
                                                              const int32_t* __restrict__ cell_faces, float max_dist,
                                                              float* __restrict__ d2_out, int32_t* __restrict__ face_out)
{
    const int64_t i = (int64_t)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    const float md2 = max_dist * max_dist;
    float best = INFINITY;
    int best_f = -1;
    auto visit = [&](int x, int y, int za, int zb) {
        const int64_t cell = me_cell_index(G, x, y, za);
        const int end = cell_offset[cell + (zb - za) + 1];
        for (int k = cell_offset[cell]; k < end; k++) {
            const int f = cell_faces[k];
            if (f == best_f) continue;   // a face spans several cells
            const float* a = verts + 3 * (int64_t)faces[3 * (int64_t)f];
            const float* b = verts + 3 * (int64_t)faces[3 * (int64_t)f + 1];
            const float* cc = verts + 3 * (int64_t)faces[3 * (int64_t)f + 2];
            const float va[3] = {a[0], a[1], a[2]}, vb[3] = {b[0], b[1], b[2]}, vc[3] = {cc[0], cc[1], cc[2]};
            const float d = me_tri_d2(p, va, vb, vc);
            if (d < best || (d == best && f < best_f)) {
                best = d;
                best_f = f;
            }
        }
    };
    me_ring_walk(G, p, max_dist, best, visit);
    const bool clipped = best_f < 0 || best > md2;
    d2_out[i] = clipped ? md2 : best;
    face_out[i] = clipped ? -1 : best_f;
}

bool me_mesh_ok(int n_verts, int n_faces) { return n_verts >= 0 && n_faces >= 0 && n_faces <= INT32_MAX / 3; }

}  // namespace

extern "C" {

int ngp_mesh_sample_surface(const float* verts, int n_verts, const int32_t* faces, int n_faces, const double* cdf,
                            double total, int64_t n, uint32_t seed, float* points, int32_t* face, void* stream)
{
    if (n < 0 || n > ME_MAX_SAMPLES) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!me_mesh_ok(n_verts, n_faces) || n_faces == 0 || n_verts == 0) return NGP_EINVAL;
    if (!verts || !faces || !cdf || !points || !face) return NGP_EINVAL;
    if (!(total > 0.0) || !isfinite(total)) return NGP_EINVAL;
    hipLaunchKernelGGL(me_sample_kernel, dim3(ngp_blocks(n, ME_BLOCK)), dim3(ME_BLOCK), 0, (hipStream_t)stream, verts,
                       faces, n_faces, cdf, total, n, seed, points, face);
    return ngp_check_launch();
}

int ngp_mesh_grid_count(const float* verts, int n_verts, const int32_t* faces, int n_faces, const float* origin3,
                        float inv_cell, const int32_t* dims3, int32_t* cell_count, int64_t* totals, void* stream)
{
    if (!me_mesh_ok(n_verts, n_faces)) return NGP_EINVAL;
    if (n_faces == 0) return NGP_OK;
    MeGrid G;
    if (!verts || !faces || !cell_count || !totals || !me_grid(origin3, inv_cell, dims3, &G)) return NGP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(me_zero_totals_kernel, dim3(1), dim3(ME_BLOCK), 0, st, (unsigned long long*)totals);
    hipLaunchKernelGGL(me_grid_count_kernel, dim3(ngp_blocks(n_faces, ME_BLOCK)), dim3(ME_BLOCK), 0, st, verts, faces,
                       n_faces, G, cell_count, (unsigned long long*)totals);
    return ngp_check_launch();
}

int ngp_mesh_grid_fill(const float* verts, int n_verts, const int32_t* faces, int n_faces, const float* origin3,
                       float inv_cell, const int32_t* dims3, const int32_t* cell_offset, int32_t* cell_cursor,
                       int32_t* cell_faces, void* stream)
{
    if (!me_mesh_ok(n_verts, n_faces)) return NGP_EINVAL;
    if (n_faces == 0) return NGP_OK;
    MeGrid G;
    if (!verts || !faces || !cell_offset || !cell_cursor || !cell_faces || !me_grid(origin3, inv_cell, dims3, &G))
        return NGP_EINVAL;
    hipLaunchKernelGGL(me_grid_fill_kernel, dim3(ngp_blocks(n_faces, ME_BLOCK)), dim3(ME_BLOCK), 0,
                       (hipStream_t)stream, verts, faces, n_faces, G, cell_offset, cell_cursor, cell_faces);
    return ngp_check_launch();
}

int ngp_mesh_closest(const float* points, int64_t n, const float* verts, int n_verts, const int32_t* faces,
                     int n_faces, const float* origin3, float inv_cell, const int32_t* dims3,
                     const int32_t* cell_offset, const int32_t* cell_faces, float max_dist, float* d2, int32_t* face,
                     void* stream)
{
    if (n < 0 || n > INT32_MAX) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (!me_mesh_ok(n_verts, n_faces) || !points || !d2 || !face || !(max_dist >= 0.f)) return NGP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ngp_blocks(n, ME_BLOCK)), block(ME_BLOCK);
    if (n_faces == 0) {
        hipLaunchKernelGGL(me_clip_all_kernel, grid, block, 0, st, n, max_dist * max_dist, d2, face);
        return ngp_check_launch();
    }
    MeGrid G;
    if (!verts || !faces || !cell_offset || !cell_faces || !me_grid(origin3, inv_cell, dims3, &G)) return NGP_EINVAL;
    hipLaunchKernelGGL(me_closest_kernel, grid, block, 0, st, points, n, verts, faces, G, cell_offset, cell_faces,
                       max_dist, d2, face);
    return ngp_check_launch();
}

}  // extern "C"
