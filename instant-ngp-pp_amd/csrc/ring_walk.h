// The dense uniform grid of M4 and M5 (include/ngp_hip.h) and the walk over it that both nearest queries share:
// ngp_mesh_closest (mesh_eval_kernels.hip, the grid holds face references) and ngp_cloud_nearest (cloud_kernels.hip,
// it holds points).  Files that include this are built with -ffp-contract=off: the cell coordinates are the f32
// expressions of their numpy restatements.
//
// The walk.  From the point's own cell coordinate c (unclamped: the point may lie outside the grid) the thread visits
// the cells of Chebyshev distance r = r0, r0 + 1, ... (r0: the first ring that meets the grid), each ring clipped to
// the grid, and the caller's `visit` keeps the smallest (d2, item) pair in `best`, so neither the grid nor the order
// inside a cell shows in the result.
//
// The stop rule.  After ring r every face not seen yet has, on some axis, a cell range that misses [c - r, c + r].
// Its closest point q lies in the box of its corners, and x -> floorf((x - o) * inv) is monotone in f32, so q's cell
// coordinate on that axis differs from the point's by at least r + 1.  With u(x) the f32 value before the floor and
// s(x) = (x - o) * inv in real numbers that gives |u(q) - u(p)| > r, and |u - s| <= |s| * (2^-23 + 2^-47) (two
// roundings).  q is inside the grid, |s(q)| <= 1024 (the dims cap), so its share is below 2^-13; the point's is below
// |u(p)| * 2^-22.  Hence |q - p| > (r - slack) / inv with slack = 2^-13 + |u(p)| * 2^-22 cells: below 2^-10 for any
// point within 3000 cells of the origin, and growing with the point's own rounding beyond that.  The f32 distance
// routine itself returns |p - q'|^2 for a q' that is a rounded convex combination of the corners: it can fall short
// of the true distance by a few ulp of the largest coordinate M (1.9 ulp measured in tests/test_mesh_eval_host.py);
// the bound allows eta = 32 ulp(M) = 2^-19 * M, M over the grid's corners and the point.  The walk stops when
// lb = (r - slack) / inv - eta is positive and lb^2 exceeds best * (1 + 2^-20): no unseen face can then reach the
// best d2, not even tie with it.  The same allowance widens the ring cap of max_dist:
// ceil(max_dist * inv + slack + eta * inv) + 1 rings, beyond which everything is clipped anyway.  The bound is formed
// in double once per ring.  The cell coordinate is clamped to +-2^20 before the conversion to int (toward the grid, so
// the ranges above only grow; fmaxf(NaN, x) = x, so a NaN coordinate lands on the clamp as well); rings are counted
// from r0, so a far point costs no empty rings.  (A point of a cloud is a face whose box is one cell: cloud_kernels.hip
// says why the bound holds for it with room to spare.)
#pragma once
#include "common.h"

#include <math.h>

constexpr int ME_MAX_DIM = 1024;              // cells per axis
constexpr int64_t ME_MAX_CELLS = 1 << 24;
constexpr float ME_COORD_LIMIT = 1048576.f;   // 2^20: point cell coordinates are clamped to +-this

struct MeGrid {
    float o[3], inv;
    int d[3];
    float coord_max;   // the largest |coordinate| of the grid's corners
};

__device__ __forceinline__ int64_t me_cell_index(const MeGrid& G, int x, int y, int z)
{
    return ((int64_t)x * G.d[1] + y) * G.d[2] + z;
}

// the grid of the caller's host arrays, checked: false = NGP_EINVAL
static inline bool me_grid(const float* origin3, float inv_cell, const int32_t* dims3, MeGrid* G)
{
    if (!origin3 || !dims3 || !(inv_cell > 0.f) || !isfinite(inv_cell)) return false;
    int64_t cells = 1;
    double m = 0.0;
    for (int a = 0; a < 3; a++) {
        if (dims3[a] < 1 || dims3[a] > ME_MAX_DIM || !isfinite(origin3[a])) return false;
        cells *= dims3[a];
        G->o[a] = origin3[a];
        G->d[a] = dims3[a];
        m = fmax(m, fmax(fabs((double)origin3[a]), fabs((double)origin3[a] + dims3[a] / (double)inv_cell)));
    }
    G->inv = inv_cell;
    G->coord_max = (float)fmin(m * (1.0 + 0x1p-20), 3.0e38);   // rounded up or not: eta has a factor of 16 to spare
    return cells <= ME_MAX_CELLS;
}

// visit(x, y, za, zb): the cells (x, y, za .. zb), neighbours in the table, so their items are one range of it (an
// empty column of any length costs two loads); it updates `best`, the smallest d2 so far, which the stop rule reads.
// Every loop bound is fixed before its loop starts.
template <typename Visit>
__device__ __forceinline__ void me_ring_walk(const MeGrid& G, const float p[3], float max_dist, const float& best,
                                             Visit visit)
{
    int c[3];
    double u_max = 0.0, p_max = (double)G.coord_max;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float u = (p[a] - G.o[a]) * G.inv;
        u_max = u == u ? fmax(u_max, fabs((double)u)) : INFINITY;   // a NaN point never stops early, and is clipped
        p_max = fmax(p_max, fabs((double)p[a]));
        c[a] = (int)fminf(fmaxf(floorf(u), -ME_COORD_LIMIT), ME_COORD_LIMIT);   // fmaxf(NaN, x) = x
    }
    int r0 = 0, r_grid = 0;   // the first ring that meets the grid, the last that does
#pragma unroll
    for (int a = 0; a < 3; a++) {
        r0 = max(r0, max(-c[a], c[a] - (G.d[a] - 1)));
        r_grid = max(r_grid, max(c[a], G.d[a] - 1 - c[a]));
    }
    const double inv = (double)G.inv, slack = 0x1p-13 + u_max * 0x1p-22, eta = 0x1p-19 * p_max;
    const double r_cap = ceil((double)max_dist * inv + slack + eta * inv) + 1.0;
    const int r_end = r_cap < (double)r_grid ? (int)r_cap : r_grid;   // r_cap NaN or infinite: the grid bounds the walk

    for (int r = r0; r <= r_end; r++) {
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, G.d[0] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, G.d[1] - 1);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, G.d[2] - 1);
        for (int x = x0; x <= x1; x++)
            for (int y = y0; y <= y1; y++) {
                if (abs(x - c[0]) == r || abs(y - c[1]) == r) {   // a whole column of the shell
                    if (z0 <= z1) visit(x, y, z0, z1);
                } else {   // its two end caps
                    if (c[2] - r >= 0 && c[2] - r < G.d[2]) visit(x, y, c[2] - r, c[2] - r);
                    if (c[2] + r >= 0 && c[2] + r < G.d[2]) visit(x, y, c[2] + r, c[2] + r);
                }
            }
        const double lb = ((double)r - slack) / inv - eta;
        if (lb > 0.0 && lb * lb > (double)best * (1.0 + 0x1p-20)) break;
    }
}
