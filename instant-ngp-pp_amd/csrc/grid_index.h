// The hash-grid level rule (tcnn Grid/Hash encoding semantics): the per-level record, the cell of
// a position on a level, the table row of a cell corner and its trilinear weight.  The one copy behind the grid kernels
// (grid_kernels.hip) and the mask field (mask_kernels.hip).
#pragma once
#include "common.h"

namespace {

struct GridMeta {
    uint32_t n_levels, n_features;
    uint32_t offset[NGP_MAX_LEVELS];
    uint32_t size[NGP_MAX_LEVELS];   // rows in the level
    uint32_t res[NGP_MAX_LEVELS];
    uint32_t flags[NGP_MAX_LEVELS];  // bit0: hashed, bit1: size is a power of two
    float scale[NGP_MAX_LEVELS];
};

struct LevelInfo {
    uint32_t offset, size, res, flags;
    float scale;
};

__device__ __forceinline__ LevelInfo level_info(const GridMeta& m, uint32_t l)
{
    LevelInfo li;
    li.offset = m.offset[l]; li.size = m.size[l]; li.res = m.res[l]; li.flags = m.flags[l]; li.scale = m.scale[l];
    return li;
}

// Negative coordinates take tiny-cuda-nn's route: (uint32_t)(int)floorf(p) and unsigned wrap in the dense index and
// in the hash.
__device__ __forceinline__ uint32_t row_index(const LevelInfo& li, uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t idx;
    if (li.flags & 1u) {
        idx = x ^ (y * 2654435761u) ^ (z * 805459861u);
        idx = (li.flags & 2u) ? (idx & (li.size - 1u)) : (idx % li.size);
    } else {
        idx = x + y * li.res + z * li.res * li.res;
        if (idx >= li.size) idx %= li.size;
    }
    return li.offset + idx;
}

struct Cell {
    uint32_t g[3];
    float w[3];
};

__device__ __forceinline__ Cell cell_of(float scale, float px, float py, float pz)
{
    const float p[3] = {fmaf(scale, px, 0.5f), fmaf(scale, py, 0.5f), fmaf(scale, pz, 0.5f)};
    Cell c;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float fl = floorf(p[k]);
        c.g[k] = (uint32_t)(int)fl;
        c.w[k] = p[k] - fl;
    }
    return c;
}

__device__ __forceinline__ Cell cell_of(const float* __restrict__ x, int64_t sample, float scale)
{
    return cell_of(scale, x[3 * sample], x[3 * sample + 1], x[3 * sample + 2]);
}

// corner k of a cell: bit 0 / 1 / 2 of k = the upper neighbour in x / y / z
__device__ __forceinline__ uint32_t corner_row(const LevelInfo& li, const Cell& c, int k)
{
    return row_index(li, c.g[0] + (k & 1), c.g[1] + ((k >> 1) & 1), c.g[2] + ((k >> 2) & 1));
}

__device__ __forceinline__ float corner_weight(float w0, float w1, float w2, int k)
{
    return ((k & 1) ? w0 : 1 - w0) * ((k & 2) ? w1 : 1 - w1) * ((k & 4) ? w2 : 1 - w2);
}

// host: the level records of a layout (false: not a layout the kernels take)
inline bool make_meta(const ngp_grid_desc* d, GridMeta& m)
{
    if (!d || d->n_levels < 1 || d->n_levels > NGP_MAX_LEVELS) return false;
    const uint32_t F = d->n_features;
    if (!(F == 1 || F == 2 || F == 4 || F == 8)) return false;
    m.n_levels = d->n_levels; m.n_features = F;
    for (uint32_t l = 0; l < NGP_MAX_LEVELS; l++) {
        m.offset[l] = 0; m.size[l] = 1; m.res[l] = 1; m.flags[l] = 0; m.scale[l] = 0;
    }
    for (uint32_t l = 0; l < d->n_levels; l++) {
        const uint32_t size = d->offsets[l + 1] - d->offsets[l], res = d->resolution[l];
        if (size == 0) return false;
        // tcnn's index loop: accumulate dims while stride <= size; hashed iff size < final stride
        uint64_t stride = 1;
        for (int k = 0; k < 3 && stride <= size; k++) stride *= res;
        uint32_t flags = 0;
        if (size < stride) flags |= 1u;
        if ((size & (size - 1)) == 0) flags |= 2u;
        m.offset[l] = d->offsets[l]; m.size[l] = size; m.res[l] = res; m.flags[l] = flags; m.scale[l] = d->scale[l];
    }
    return true;
}

}  // namespace
