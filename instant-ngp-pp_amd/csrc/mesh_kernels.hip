// Marching cubes on a dense lattice (mesh export: mesh.py, tools/extract_mesh.py).
//
// Compiled with -ffp-contract=off (build.py): a vertex position is origin + (idx + t) * spacing evaluated as written,
// so the CPU restatement in tests/mesh_reference.py reproduces it bit for bit.
//
// Layout.  The volume is C-order (nx, ny, nz), z fastest; lattice point p = (i*ny + j)*nz + k.  Point p owns the
// lattice edges from p toward +x, +y, +z, and the cell whose lowest corner it is.  Every owned edge whose end points
// classify differently (inside iff v > level; NaN is outside) gets exactly one vertex, so the mesh is welded by
// construction: vertices are numbered point-major, x < y < z edge within a point, and triangles cell-major, in
// table order within a cell.  No atomics: the output is the same from run to run.
//
// Three launches.  mc_count_kernel (one thread per point) classifies, counts the point's vertices and its cell's
// triangles, scans the vertex counts inside the workgroup and stores one word per point, (local vertex offset << 3 |
// crossing mask), plus the workgroup's two sums.  mc_scan_blocks_kernel scans the workgroup sums (one workgroup,
// 64-bit running sums) into workgroup offsets and the totals.  mc_emit_kernel recomputes the counts, scans the triangle
// counts inside the workgroup, writes the point's vertices, and resolves its cell's triangle corners through the words
// of the points that own those edges.
#include "common.h"

namespace {

constexpr int MC_BLOCK = 256;            // threads per workgroup of the count / emit passes (4 waves)
constexpr int MC_SCAN_THREADS = 1024;    // the single workgroup of the block-sum scan

// ---- the case table ----------------------------------------------------------------------------------------------
// Corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) from its lowest corner; bit c of the case
// index is set iff corner c is inside.  Edge e = 4*a + m runs along axis a from its low corner, whose coordinate on
// axis (a+1)%3 is m & 1 and on axis (a+2)%3 is m >> 1.
//
// The table is generated here from one face-local rule.  Walk each of the 6 faces counter-clockwise about its
// outward normal; a boundary segment runs from every outside->inside edge to the next inside->outside edge.  On an
// ambiguous face (inside corners diagonal) each inside corner is thus cut off on its own ("inside corners are
// separated").  Both cells sharing a face see the same corners and draw the same segments (in opposite directions,
// as their outward normals are opposite), so surfaces away from the volume boundary are closed, consistently
// oriented 2-manifolds.  Each crossing edge is entered on one face and left on another, so the segments chain into
// disjoint loops; each loop is fanned from a vertex whose chords all run through the cell's interior.  A loop runs
// counter-clockwise about the normal that points from inside to outside, so (v1-v0) x (v2-v0) points toward lower
// density.
struct McTables {
    int8_t tri[256][16];      // up to 5 triangles (edge triples), -1 terminated
    int8_t ntri[256];
    int8_t edge_corner[12][2];
};

constexpr int mc_corner(const int o[3]) { return o[0] | o[1] << 1 | o[2] << 2; }

constexpr int mc_edge_between(const int8_t ec[12][2], int c0, int c1)
{
    for (int e = 0; e < 12; e++)
        if ((ec[e][0] == c0 && ec[e][1] == c1) || (ec[e][0] == c1 && ec[e][1] == c0)) return e;
    return -1;
}

constexpr bool mc_on_face(const int f[4], int c) { return f[0] == c || f[1] == c || f[2] == c || f[3] == c; }

constexpr bool mc_share_face(const int face[6][4], const int8_t ec[12][2], int e0, int e1)
{
    for (int f = 0; f < 6; f++)
        if (mc_on_face(face[f], ec[e0][0]) && mc_on_face(face[f], ec[e0][1]) && mc_on_face(face[f], ec[e1][0]) &&
            mc_on_face(face[f], ec[e1][1]))
            return true;
    return false;
}

constexpr McTables mc_make_tables()
{
    McTables t{};
    for (int a = 0; a < 3; a++)
        for (int m = 0; m < 4; m++) {
            int o[3] = {0, 0, 0};
            o[(a + 1) % 3] = m & 1;
            o[(a + 2) % 3] = m >> 1;
            t.edge_corner[4 * a + m][0] = (int8_t)mc_corner(o);
            o[a] = 1;
            t.edge_corner[4 * a + m][1] = (int8_t)mc_corner(o);
        }
    // faces: 4 corners counter-clockwise about the outward normal (axis b=(a+1)%3, c=(a+2)%3: e_b x e_c = e_a)
    int face[6][4] = {};
    const int ccw[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
    for (int a = 0; a < 3; a++)
        for (int s = 0; s < 2; s++)
            for (int q = 0; q < 4; q++) {
                const int* uv = ccw[s ? q : 3 - q];
                int o[3] = {0, 0, 0};
                o[a] = s;
                o[(a + 1) % 3] = uv[0];
                o[(a + 2) % 3] = uv[1];
                face[2 * a + s][q] = mc_corner(o);
            }
    for (int cs = 0; cs < 256; cs++) {
        int next[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
        for (int f = 0; f < 6; f++)
            for (int q = 0; q < 4; q++) {
                const int c0 = face[f][q], c1 = face[f][(q + 1) & 3];
                if ((cs >> c0 & 1) || !(cs >> c1 & 1)) continue;       // not an outside -> inside edge
                int r = (q + 1) & 3;
                while (cs >> face[f][(r + 1) & 3] & 1) r = (r + 1) & 3;  // end of the inside run
                next[mc_edge_between(t.edge_corner, c0, c1)] =
                    mc_edge_between(t.edge_corner, face[f][r], face[f][(r + 1) & 3]);
            }
        bool seen[12] = {};
        int n = 0;
        for (int e = 0; e < 12; e++) {
            if (next[e] < 0 || seen[e]) continue;
            int loop[12] = {}, len = 0;
            for (int x = e; !seen[x]; x = next[x]) {
                seen[x] = true;
                loop[len++] = x;
            }
            // fan apex: the first loop vertex none of whose chords lies on a cube face (there always is one).  A
            // chord between two vertices of an ambiguous face could also be drawn by the neighbouring cell, and the
            // edge would then bound four triangles.
            int apex = 0;
            for (int i = 0; i < len; i++) {
                bool safe = true;
                for (int j = 0; j < len; j++)
                    if (j != i && j != (i + 1) % len && j != (i + len - 1) % len &&
                        mc_share_face(face, t.edge_corner, loop[i], loop[j]))
                        safe = false;
                if (safe) {
                    apex = i;
                    break;
                }
            }
            for (int i = 1; i + 1 < len; i++) {
                t.tri[cs][3 * n] = (int8_t)loop[apex];
                t.tri[cs][3 * n + 1] = (int8_t)loop[(apex + i) % len];
                t.tri[cs][3 * n + 2] = (int8_t)loop[(apex + i + 1) % len];
                n++;
            }
        }
        t.ntri[cs] = (int8_t)n;
        for (int i = 3 * n; i < 16; i++) t.tri[cs][i] = -1;
    }
    return t;
}

constexpr McTables kMcTables = mc_make_tables();
static_assert(kMcTables.ntri[0] == 0 && kMcTables.ntri[255] == 0, "empty cases");
static_assert(kMcTables.ntri[0x69] == 4 && kMcTables.ntri[0x96] == 4, "checkerboard cases: four separated corners");

__constant__ McTables c_mc = kMcTables;

struct McLattice {
    int nx, ny, nz, n;   // n = nx*ny*nz < 2^31
    float level;
};

// classification of the point's owned edges (bit a: edge toward +axis a crosses) and, when the point owns a cell,
// its case (else -1)
__device__ __forceinline__ void mc_classify(const float* __restrict__ vol, const McLattice& L, int p, int& mask,
                                            int& cs)
{
    const int k = p % L.nz, r = p / L.nz, j = r % L.ny, i = r / L.ny;
    const int sy = L.nz, sx = L.ny * L.nz;
    const bool hx = i + 1 < L.nx, hy = j + 1 < L.ny, hz = k + 1 < L.nz;
    const float lv = L.level;
    const int c0 = vol[p] > lv;
    mask = 0;
    cs = -1;
    if (hx && hy && hz) {
        const int c1 = vol[p + sx] > lv, c2 = vol[p + sy] > lv, c3 = vol[p + sx + sy] > lv;
        const int c4 = vol[p + 1] > lv, c5 = vol[p + sx + 1] > lv, c6 = vol[p + sy + 1] > lv;
        const int c7 = vol[p + sx + sy + 1] > lv;
        cs = c0 | c1 << 1 | c2 << 2 | c3 << 3 | c4 << 4 | c5 << 5 | c6 << 6 | c7 << 7;
        mask = (c0 != c1) | (c0 != c2) << 1 | (c0 != c4) << 2;
    } else {
        if (hx) mask |= (vol[p + sx] > lv) != c0;
        if (hy) mask |= ((vol[p + sy] > lv) != c0) << 1;
        if (hz) mask |= ((vol[p + 1] > lv) != c0) << 2;
    }
}

__global__ void __launch_bounds__(MC_BLOCK) mc_count_kernel(const float* __restrict__ vol, McLattice L,
                                                            int32_t* __restrict__ word, int32_t* __restrict__ block_sums)
{
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    int mask = 0, cs = -1;
    if (p < L.n) mc_classify(vol, L, p, mask, cs);
    const int nv = __popc(mask), nt = cs >= 0 ? c_mc.ntri[cs] : 0;
    // vertex counts in the low 16 bits, triangle counts in the high ones (per workgroup at most 768 and 1280)
    int tot;
    const int off = block_excl_scan<MC_BLOCK>(nv | nt << 16, &tot);
    if (p < L.n) word[p] = (off & 0xffff) << 3 | mask;
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

// exclusive scan of the packed workgroup sums -> workgroup vertex / triangle offsets; totals[0] = V, totals[1] = F.
// A total above INT32_MAX cannot be indexed by int32 faces: it is reported as -1 and status[0] = 1 stops the emit.
__global__ void __launch_bounds__(MC_SCAN_THREADS) mc_scan_blocks_kernel(const int32_t* __restrict__ block_sums,
                                                                         int nb, int32_t* __restrict__ off_v,
                                                                         int32_t* __restrict__ off_t,
                                                                         int32_t* __restrict__ status,
                                                                         int32_t* __restrict__ totals)
{
    // the two halves of the packed sums, one after the other (a tile sums to at most 1024 * 1280: int32)
    const auto clamped = [](int64_t e) { return (int32_t)(e < INT32_MAX ? e : INT32_MAX); };
    const int64_t carry_v = block_carry_scan<MC_SCAN_THREADS, int64_t>(
        nb, [&](int b) { return block_sums[b] & 0xffff; }, [&](int b, int64_t excl) { off_v[b] = clamped(excl); });
    const int64_t carry_t = block_carry_scan<MC_SCAN_THREADS, int64_t>(
        nb, [&](int b) { return block_sums[b] >> 16; }, [&](int b, int64_t excl) { off_t[b] = clamped(excl); });
    if (threadIdx.x == 0) {
        const bool over = carry_v > INT32_MAX || carry_t > INT32_MAX;
        status[0] = over ? 1 : 0;
        totals[0] = carry_v > INT32_MAX ? -1 : (int32_t)carry_v;
        totals[1] = carry_t > INT32_MAX ? -1 : (int32_t)carry_t;
    }
}

struct McPlace {
    float o[3], s[3];
};

__device__ __forceinline__ int mc_vertex_index(const int32_t* __restrict__ word, const int32_t* __restrict__ off_v,
                                               int q, int axis)
{
    const int w = word[q];
    return off_v[q / MC_BLOCK] + (w >> 3) + __popc(w & ((1 << axis) - 1));
}

__global__ void __launch_bounds__(MC_BLOCK) mc_emit_kernel(const float* __restrict__ vol, McLattice L, McPlace P,
                                                           const int32_t* __restrict__ word,
                                                           const int32_t* __restrict__ off_v,
                                                           const int32_t* __restrict__ off_t,
                                                           const int32_t* __restrict__ status,
                                                           float* __restrict__ verts, int32_t* __restrict__ faces)
{
    if (status[0]) return;   // totals overflowed int32: the caller has no buffers for this mesh
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    int mask = 0, cs = -1;
    if (p < L.n) mc_classify(vol, L, p, mask, cs);
    const int nt = cs >= 0 ? c_mc.ntri[cs] : 0;
    const int toff = block_excl_scan<MC_BLOCK>(nt) + off_t[blockIdx.x];
    if (p >= L.n) return;

    const int k = p % L.nz, r = p / L.nz, j = r % L.ny, i = r / L.ny;
    const int stride[3] = {L.ny * L.nz, L.nz, 1};
    if (mask) {
        const float lv = L.level, v0 = vol[p];
        const float idx[3] = {(float)i, (float)j, (float)k};
        int64_t slot = (int64_t)off_v[blockIdx.x] + (word[p] >> 3);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!(mask >> a & 1)) continue;
            const float v1 = vol[p + stride[a]];
            float t = (lv - v0) / (v1 - v0);
            t = fminf(fmaxf(t, 0.0f), 1.0f);   // NaN -> 0: the vertex stays on its edge
            float* out = verts + 3 * slot;
#pragma unroll
            for (int c = 0; c < 3; c++) out[c] = P.o[c] + (c == a ? idx[c] + t : idx[c]) * P.s[c];
            slot++;
        }
    }
    if (nt) {
        const int corner_off[8] = {0,
                                   stride[0],
                                   stride[1],
                                   stride[0] + stride[1],
                                   1,
                                   stride[0] + 1,
                                   stride[1] + 1,
                                   stride[0] + stride[1] + 1};
        int32_t* out = faces + 3 * (int64_t)toff;
        for (int q = 0; q < 3 * nt; q++) {
            const int e = c_mc.tri[cs][q];
            out[q] = mc_vertex_index(word, off_v, p + corner_off[c_mc.edge_corner[e][0]], e >> 2);
        }
    }
}

int mc_check(int nx, int ny, int nz, int* n)
{
    if (nx < 0 || ny < 0 || nz < 0) return NGP_EINVAL;
    const int64_t pts = (int64_t)nx * ny * nz;
    if (pts >= (1ll << 31)) return NGP_EINVAL;
    *n = (int)pts;
    return NGP_OK;
}

bool mc_empty(int nx, int ny, int nz) { return nx < 2 || ny < 2 || nz < 2; }

}  // namespace

extern "C" {

int64_t ngp_mc_workspace(int nx, int ny, int nz)
{
    int n = 0;
    if (mc_check(nx, ny, nz, &n) != NGP_OK) return NGP_EINVAL;
    if (mc_empty(nx, ny, nz)) return 0;
    const int64_t nb = (n + MC_BLOCK - 1) / MC_BLOCK;
    return (int64_t)n + 3 * nb + 4;
}

int ngp_mc_tables(int8_t* tri_table, int8_t* tri_count, int8_t* edge_corner)
{
    if (!tri_table || !tri_count || !edge_corner) return NGP_EINVAL;
    for (int c = 0; c < 256; c++) {
        for (int q = 0; q < 16; q++) tri_table[16 * c + q] = kMcTables.tri[c][q];
        tri_count[c] = kMcTables.ntri[c];
    }
    for (int e = 0; e < 12; e++) {
        edge_corner[2 * e] = kMcTables.edge_corner[e][0];
        edge_corner[2 * e + 1] = kMcTables.edge_corner[e][1];
    }
    return NGP_OK;
}

int ngp_mc_count(const float* volume, int nx, int ny, int nz, float level, int32_t* workspace, int32_t* totals,
                 void* stream)
{
    int n = 0;
    if (mc_check(nx, ny, nz, &n) != NGP_OK) return NGP_EINVAL;
    if (mc_empty(nx, ny, nz)) return NGP_OK;
    if (!volume || !workspace || !totals) return NGP_EINVAL;
    const int nb = (n + MC_BLOCK - 1) / MC_BLOCK;
    int32_t* word = workspace;
    int32_t* block_sums = word + n;
    int32_t* off_v = block_sums + nb;
    int32_t* off_t = off_v + nb;
    int32_t* status = off_t + nb;
    const McLattice L{nx, ny, nz, n, level};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_count_kernel, dim3(nb), dim3(MC_BLOCK), 0, st, volume, L, word, block_sums);
    hipLaunchKernelGGL(mc_scan_blocks_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, st, block_sums, nb, off_v, off_t,
                       status, totals);
    return ngp_check_launch();
}

int ngp_mc_emit(const float* volume, int nx, int ny, int nz, float level, const float* origin3,
                const float* spacing3, const int32_t* workspace, float* verts, int32_t* faces, void* stream)
{
    int n = 0;
    if (mc_check(nx, ny, nz, &n) != NGP_OK) return NGP_EINVAL;
    if (mc_empty(nx, ny, nz)) return NGP_OK;
    if (!volume || !origin3 || !spacing3 || !workspace || !verts || !faces) return NGP_EINVAL;
    const int nb = (n + MC_BLOCK - 1) / MC_BLOCK;
    const int32_t* word = workspace;
    const int32_t* off_v = word + n + nb;
    const int32_t* off_t = off_v + nb;
    const int32_t* status = off_t + nb;
    const McLattice L{nx, ny, nz, n, level};
    const McPlace P{{origin3[0], origin3[1], origin3[2]}, {spacing3[0], spacing3[1], spacing3[2]}};
    hipLaunchKernelGGL(mc_emit_kernel, dim3(nb), dim3(MC_BLOCK), 0, (hipStream_t)stream, volume, L, P, word, off_v,
                       off_t, status, verts, faces);
    return ngp_check_launch();
}

}  // extern "C"
