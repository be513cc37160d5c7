// Point clouds (M5 of include/ngp_hip.h): the nearest point of a cloud with the sums a registration step needs, the
// ordered sum of those, and the mean of every voxel of a sorted cloud: cloud.py nearest_points / icp / voxel_downsample,
// tools/eval_mesh.py --ref_points.  Built with -ffp-contract=off: the transformed query, the cell coordinates, the
// squared distances and the voxel means are the expressions of the numpy restatement (tests/cloud_reference.py), bit
// for bit.
//
// Grid: M4's dense compressed-row grid.  The host sorts the cloud by cell (stable), so a cell's points are one range
// of the sorted copy and no reference table is needed: cell_offset indexes the rows themselves.  A row is 16 bytes,
// (x, y, z, the bits of the point's original index): one dwordx4 load per candidate, and the lanes of a wave, whose
// queries the host sorted by cell as well, mostly ask for the same row (a broadcast).  The alternative, 12-byte rows
// and a separate index table, costs two loads per candidate and was not measured.
//
// Query: one thread per query on ring_walk.h's walk, stop rule and ring cap, unchanged.  Why that bound holds for
// points: a point is a face whose three corners coincide, so its box is the one cell the host's sort put it in (the
// same f32 cell coordinate), and the argument "an unseen item differs by more than r cells on some axis, hence lies
// farther than (r - slack) / inv" applies as it stands.  The allowance eta = 32 ulp(M) was sized for the triangle
// routine, which may fall short of the true distance by a few ulp(M); here d2 = (dx dx + dy dy) + dz dz of exact
// operands, where each difference is off by at most half an ulp(M) and the three products and two sums by 2^-24
// relative each, so the computed distance is short by less than ulp(M) + 2^-22 |p - q|: inside eta and the factor
// 1 + 2^-20 on best with room to spare.  The bound is conservative for points, never tight.
//
// Sums: every thread holds its query's 18 terms in double (zero unless it matched); wave_sum<double> adds each over the
// wave, lane 0 leaves the wave's 18 in LDS and, behind one barrier, thread e < 18 adds the 4 waves in order and stores
// entry e of the workgroup's own row.  ngp_cloud_sum_partials is a second launch of ONE workgroup: accumulator g of 14
// takes the rows g, g + 14, ... in rising order, then thread e adds the 14 in order.  No atomics, and no workgroup
// reads what another stored inside a launch: the same bytes on every run.
#include "common.h"
#include "ring_walk.h"

#include <math.h>

namespace {

constexpr int CL_BLOCK = 256;                  // threads per workgroup (4 waves)
constexpr int CL_WAVES = CL_BLOCK / NGP_WAVE;
constexpr int CL_SUMS = 18;                    // count, sum p (3), sum q (3), sum p q^T (9), sum |p|^2, sum d2
constexpr int CL_LANES = 14;                   // accumulators of the ordered sum: 14 * 18 = 252 threads of 256

struct ClXform {
    float m[12];   // row-major 3 x 4
    float c[3];    // the centre the sums are taken about
    int on;        // 0: the queries are used as they are
};

__global__ void __launch_bounds__(CL_BLOCK) cl_nearest_kernel(const float* __restrict__ queries, int64_t n,
                                                              const float4* __restrict__ cloud4, int n_cloud, MeGrid G,
                                                              const int32_t* __restrict__ cell_offset, float max_dist,
                                                              ClXform X, float* __restrict__ d2_out,
                                                              int32_t* __restrict__ index_out,
                                                              double* __restrict__ partials)
{
    const int64_t i = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool live = i < n;   // no early return: every thread reaches the barrier of the sums
    float p[3] = {0.f, 0.f, 0.f}, best_q[3] = {0.f, 0.f, 0.f};
    float best = INFINITY;
    int best_i = -1;
    const float md2 = max_dist * max_dist;
    if (live) {
        const float x = queries[3 * i], y = queries[3 * i + 1], z = queries[3 * i + 2];
        if (X.on) {
#pragma unroll
            for (int a = 0; a < 3; a++) p[a] = ((X.m[4 * a] * x + X.m[4 * a + 1] * y) + X.m[4 * a + 2] * z) + X.m[4 * a + 3];
        } else {
            p[0] = x;
            p[1] = y;
            p[2] = z;
        }
        if (n_cloud > 0) {
            auto visit = [&](int cx, int cy, int za, int zb) {
                const int64_t cell = me_cell_index(G, cx, cy, za);
                // offsets of another cloud must not read past this one
                const int begin = max(cell_offset[cell], 0), end = min(cell_offset[cell + (zb - za) + 1], n_cloud);
                for (int k = begin; k < end; k++) {
                    const float4 q = cloud4[k];
                    const int qi = __float_as_int(q.w);
                    const float dx = p[0] - q.x, dy = p[1] - q.y, dz = p[2] - q.z;
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    if (d < best || (d == best && qi < best_i)) {
                        best = d;
                        best_i = qi;
                        best_q[0] = q.x;
                        best_q[1] = q.y;
                        best_q[2] = q.z;
                    }
                }
            };
            me_ring_walk(G, p, max_dist, best, visit);
        }
    }
    const bool matched = live && best_i >= 0 && !(best > md2);
    if (live) {
        if (d2_out) d2_out[i] = matched ? best : md2;
        if (index_out) index_out[i] = matched ? best_i : -1;
    }
    if (!partials) return;   // uniform over the launch

    double t[CL_SUMS];
#pragma unroll
    for (int e = 0; e < CL_SUMS; e++) t[e] = 0.0;
    if (matched) {
        double pc[3], qc[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            pc[a] = (double)p[a] - (double)X.c[a];
            qc[a] = (double)best_q[a] - (double)X.c[a];
        }
        t[0] = 1.0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            t[1 + a] = pc[a];
            t[4 + a] = qc[a];
#pragma unroll
            for (int b = 0; b < 3; b++) t[7 + 3 * a + b] = pc[a] * qc[b];
        }
        t[16] = (pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2];
        t[17] = (double)best;
    }
    __shared__ double wave_sums[CL_WAVES][CL_SUMS];
    const int lane = threadIdx.x & (NGP_WAVE - 1), wave = threadIdx.x / NGP_WAVE;
#pragma unroll
    for (int e = 0; e < CL_SUMS; e++) {
        const double s = wave_sum<double>(t[e]);
        if (lane == 0) wave_sums[wave][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < CL_SUMS) {
        double s = wave_sums[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CL_WAVES; w++) s += wave_sums[w][threadIdx.x];
        partials[(int64_t)blockIdx.x * CL_SUMS + threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(CL_BLOCK) cl_sum_partials_kernel(const double* __restrict__ partials, int64_t rows,
                                                                   double* __restrict__ sums18)
{
    __shared__ double acc[CL_LANES][CL_SUMS];
    const int g = threadIdx.x / CL_SUMS, e = threadIdx.x % CL_SUMS;
    if (g < CL_LANES) {
        double s = 0.0;
        for (int64_t r = g; r < rows; r += CL_LANES) s += partials[r * CL_SUMS + e];   // the workgroup reads 252 doubles in a row
        acc[g][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < CL_SUMS) {
        double s = acc[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < CL_LANES; k++) s += acc[k][threadIdx.x];
        sums18[threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(CL_BLOCK) cl_voxel_mean_kernel(const float* __restrict__ points,
                                                                 const float* __restrict__ normals,
                                                                 const uint8_t* __restrict__ colors, int64_t n,
                                                                 const int64_t* __restrict__ offsets, int64_t n_voxels,
                                                                 float* __restrict__ points_out,
                                                                 float* __restrict__ normals_out,
                                                                 uint8_t* __restrict__ colors_out)
{
    const int64_t v = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (v >= n_voxels) return;
    // whatever the offsets hold, the run stays inside the input
    const int64_t begin = min(max(offsets[v], (int64_t)0), n), end = min(max(offsets[v + 1], begin), n);
    const double count = (double)(end - begin);
    double sp[3] = {0.0, 0.0, 0.0}, sn[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
    for (int64_t k = begin; k < end; k++) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            sp[a] += (double)points[3 * k + a];
            if (normals) sn[a] += (double)normals[3 * k + a];
            if (colors) sc[a] += (double)colors[3 * k + a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const bool any = end > begin;   // an empty run (offsets that repeat) writes zeros
        points_out[3 * v + a] = any ? (float)(sp[a] / count) : 0.f;
        if (normals) normals_out[3 * v + a] = any ? (float)(sn[a] / count) : 0.f;
        if (colors) colors_out[3 * v + a] = any ? (uint8_t)floor(sc[a] / count + 0.5) : (uint8_t)0;
    }
}

}  // namespace

extern "C" {

int ngp_cloud_nearest(const float* queries, int64_t n, const float* cloud4, int n_cloud, const float* origin3,
                      float inv_cell, const int32_t* dims3, const int32_t* cell_offset, float max_dist,
                      const float* xform12, const float* centre3, float* d2, int32_t* index, double* partials,
                      void* stream)
{
    if (n < 0 || n > INT32_MAX) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (n_cloud < 0 || !queries || !(max_dist >= 0.f)) return NGP_EINVAL;
    if (partials && !centre3) return NGP_EINVAL;
    MeGrid G = {};
    if (n_cloud > 0 && (!cloud4 || !aligned16(cloud4) || !cell_offset || !me_grid(origin3, inv_cell, dims3, &G)))
        return NGP_EINVAL;
    ClXform X = {};
    if (xform12) {
        for (int k = 0; k < 12; k++) X.m[k] = xform12[k];
        X.on = 1;
    }
    if (centre3)
        for (int a = 0; a < 3; a++) {
            if (!isfinite(centre3[a])) return NGP_EINVAL;
            X.c[a] = centre3[a];
        }
    hipLaunchKernelGGL(cl_nearest_kernel, dim3(ngp_blocks(n, CL_BLOCK)), dim3(CL_BLOCK), 0, (hipStream_t)stream,
                       queries, n, (const float4*)cloud4, n_cloud, G, cell_offset, max_dist, X, d2, index, partials);
    return ngp_check_launch();
}

int ngp_cloud_sum_partials(const double* partials, int64_t rows, double* sums18, void* stream)
{
    if (rows < 0 || rows > INT32_MAX) return NGP_EINVAL;
    if (!sums18 || (rows > 0 && !partials)) return NGP_EINVAL;
    hipLaunchKernelGGL(cl_sum_partials_kernel, dim3(1), dim3(CL_BLOCK), 0, (hipStream_t)stream, partials, rows, sums18);
    return ngp_check_launch();
}

int ngp_cloud_voxel_mean(const float* points, const float* normals, const uint8_t* colors, int64_t n,
                         const int64_t* offsets, int64_t n_voxels, float* points_out, float* normals_out,
                         uint8_t* colors_out, void* stream)
{
    if (n < 0 || n > INT32_MAX) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (n_voxels < 0 || n_voxels > n) return NGP_EINVAL;
    if (n_voxels == 0) return NGP_OK;
    if (!points || !offsets || !points_out || (normals && !normals_out) || (colors && !colors_out)) return NGP_EINVAL;
    hipLaunchKernelGGL(cl_voxel_mean_kernel, dim3(ngp_blocks(n_voxels, CL_BLOCK)), dim3(CL_BLOCK), 0,
                       (hipStream_t)stream, points, normals, colors, n, offsets, n_voxels, points_out, normals_out,
                       colors_out);
    return ngp_check_launch();
}

}  // extern "C"
