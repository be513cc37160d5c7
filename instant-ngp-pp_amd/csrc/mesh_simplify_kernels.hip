// Mesh simplification by uniform vertex clustering (Rossignac-Borrel) with one quadric solve per cell (Lindstrom):
// mesh.py simplify_mesh, tools/extract_mesh.py.  Built with -ffp-contract=off: the cell keys are the f32 expression
// floorf((v - origin) * inv) of the numpy restatement, bit for bit.
//
// Count (ngp_mesh_simplify_count), eight launches, nothing summed and no output but the totals:
//   fill     every table word to ~0 (an empty key, an empty face slot, the identity of the unsigned atomicMin);
//   insert   one thread per vertex: its key (21 bits per axis) goes into an open-addressing table of 64-bit keys with
//            atomicCAS, and atomicMin lowers the slot's member word to the vertex index; the thread keeps its slot;
//   flag     a vertex is its cluster's smallest member iff the slot's member word is its own index; the flags are
//            scanned inside each workgroup (local offset << 1 | flag) and the workgroup sums in one workgroup, so
//            clusters are numbered in ascending order of their smallest member;
//   number   cluster[v] = the number of the slot's smallest member;
//   faces    one thread per face: corners -> cluster numbers; a face with two equal corners is degenerate; every
//            other face goes into a second table whose slots hold the index of SOME face of that unordered triple
//            (atomicCAS claims an empty slot; a claimed slot's face is compared through its own corners, which are
//            inputs of this launch), and atomicMin lowers the slot's face word;
//   keep     a face stays iff it is not degenerate and its slot's face word is its own index; flags scanned as above.
// Every probe loop runs at most `capacity` steps; a table that has no room (it cannot happen at >= 2x the element
// count, but no loop may depend on that) sets an error bit instead of spinning.  Within a launch threads learn about
// each other ONLY through the return values of atomics (another workgroup's plain stores may not be visible: per-CU
// L1s and per-XCD L2s are not coherent); every lookup of a table happens in a later launch.
//
// Emit.  ngp_mesh_simplify_groups writes the cluster number of every vertex and of every face corner; the caller
// sorts each array once (stable), so that the members of a cluster are contiguous and in ascending index order.
// ngp_mesh_simplify_place runs one thread per cluster over its members in that order, all sums in double and none of
// them by atomics: the same bytes from run to run.  ngp_mesh_simplify_faces writes the kept faces in their original
// order and winding and counts, per cluster, the kept corners that use it (integer atomics; only > 0 is read), which
// is what ngp_mesh_compact_* (M2) needs to drop the clusters no kept face uses.
#include "common.h"

#include <math.h>

namespace {

constexpr int SM_BLOCK = 256;           // threads per workgroup of every per-element pass (4 waves)
constexpr int SM_SCAN_THREADS = 1024;   // the single workgroup of the block-sum scan
constexpr int SM_MAX_ELEMS = 1 << 28;   // vertices or faces: table capacities and 3 * n_faces stay below 2^31
constexpr float SM_KEY_LIMIT = 2097152.f;   // 2^21 cells per axis
constexpr unsigned long long SM_EMPTY_KEY = ~0ull;   // no valid key: a key has 63 bits

enum { SM_T_CLUSTERS = 0, SM_T_KEPT = 1, SM_T_DEGENERATE = 2, SM_T_ERROR = 3, SM_N_TOTALS = 4 };
enum { SM_ERR_KEY = 1, SM_ERR_FULL = 2 };

struct SmLayout {   // workspace: int32 words; the four tables first (one fill), the 64-bit one at the front
    unsigned long long* vkey;   // (cap_v) cell key of the slot, or SM_EMPTY_KEY
    unsigned* vmin;             // (cap_v) smallest vertex index inserted at the slot
    int32_t* fany;              // (cap_f) some face of the slot's corner triple, or -1
    unsigned* fmin;             // (cap_f) smallest face index inserted at the slot
    int32_t* slot_v;            // (n_verts) the vertex's slot, or -1 (bad key, no room)
    int32_t* word_v;            // (n_verts) local offset << 1 | smallest member of its cluster
    int32_t* cluster;           // (n_verts) cluster number
    int32_t* slot_f;            // (n_faces) the face's slot, or -1 (degenerate, no room)
    int32_t* word_f;            // (n_faces) local offset << 1 | kept
    int32_t* sums_v;            // (nb_v) workgroup sums and (offs) their exclusive scans
    int32_t* offs_v;
    int32_t* sums_f;            // (nb_f)
    int32_t* offs_f;
    int cap_v, cap_f, nb_v, nb_f;
    int64_t table_words, words;
};

int sm_blocks(int n) { return (n + SM_BLOCK - 1) / SM_BLOCK; }

int sm_capacity(int n)   // a power of two >= 2n (n <= SM_MAX_ELEMS: at most 2^29)
{
    int c = 2;
    while (c < 2 * (int64_t)n) c <<= 1;
    return c;
}

bool sm_sizes_ok(int n_verts, int n_faces)
{
    return n_verts >= 0 && n_faces >= 0 && n_verts <= SM_MAX_ELEMS && n_faces <= SM_MAX_ELEMS;
}

SmLayout sm_layout(int32_t* ws, int n_verts, int n_faces)
{
    SmLayout L;
    L.cap_v = sm_capacity(n_verts);
    L.cap_f = sm_capacity(n_faces);
    L.nb_v = sm_blocks(n_verts);
    L.nb_f = sm_blocks(n_faces);
    int64_t at = 0;
    auto take = [&](int64_t n) {   // ws == nullptr: only the sizes are wanted
        int32_t* p = ws ? ws + at : nullptr;
        at += n;
        return p;
    };
    L.vkey = (unsigned long long*)take(2 * (int64_t)L.cap_v);
    L.vmin = (unsigned*)take(L.cap_v);
    L.fany = take(L.cap_f);
    L.fmin = (unsigned*)take(L.cap_f);
    L.table_words = at;
    L.slot_v = take(n_verts);
    L.word_v = take(n_verts);
    L.cluster = take(n_verts);
    L.slot_f = take(n_faces);
    L.word_f = take(n_faces);
    L.sums_v = take(L.nb_v);
    L.offs_v = take(L.nb_v);
    L.sums_f = take(L.nb_f);
    L.offs_f = take(L.nb_f);
    L.words = at;
    return L;
}

__global__ void __launch_bounds__(SM_BLOCK) sm_fill_kernel(int32_t* __restrict__ tables, int64_t n,
                                                           int32_t* __restrict__ totals)
{
    const int64_t stride = (int64_t)gridDim.x * SM_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < n; i += stride) tables[i] = -1;
    if (blockIdx.x == 0 && threadIdx.x < SM_N_TOTALS) totals[threadIdx.x] = 0;
}

__device__ __forceinline__ unsigned sm_mix(unsigned long long k)   // the 64-bit finaliser of MurmurHash3
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k;
}

// the cell key of a position, one f32 expression per axis; false: a non-finite coordinate or a key outside [0, 2^21)
__device__ __forceinline__ bool sm_cell(const float* __restrict__ p, float o0, float o1, float o2, float inv,
                                        unsigned q[3])
{
    const float o[3] = {o0, o1, o2};
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float c = floorf((p[a] - o[a]) * inv);
        const bool in = c >= 0.f && c < SM_KEY_LIMIT;   // false for NaN
        ok &= in;
        q[a] = in ? (unsigned)c : 0u;
    }
    return ok;
}

// one word per wave that has a failing lane
__device__ __forceinline__ void sm_raise(int32_t* __restrict__ totals, int err)
{
    if (__any(err != 0)) {
        int all = err;
#pragma unroll
        for (int o = NGP_WAVE / 2; o > 0; o >>= 1) all |= __shfl_xor(all, o, NGP_WAVE);
        if ((threadIdx.x & (NGP_WAVE - 1)) == 0) atomicOr(&totals[SM_T_ERROR], all);
    }
}

__global__ void __launch_bounds__(SM_BLOCK) sm_insert_verts_kernel(const float* __restrict__ verts, int n_verts,
                                                                   float o0, float o1, float o2, float inv,
                                                                   SmLayout L, int32_t* __restrict__ totals)
{
    const int v = blockIdx.x * SM_BLOCK + threadIdx.x;
    int err = 0;
    if (v < n_verts) {
        unsigned q[3];
        int slot = -1;
        if (!sm_cell(verts + 3 * (int64_t)v, o0, o1, o2, inv, q)) {
            err = SM_ERR_KEY;
        } else {
            const unsigned long long key = (unsigned long long)q[0] << 42 | (unsigned long long)q[1] << 21 | q[2];
            const unsigned mask = (unsigned)L.cap_v - 1;
            unsigned h = sm_mix(key) & mask;
            for (int step = 0; step < L.cap_v; step++) {   // bounded by the capacity
                const unsigned long long was = atomicCAS(&L.vkey[h], SM_EMPTY_KEY, key);
                if (was == SM_EMPTY_KEY || was == key) {
                    slot = (int)h;
                    break;
                }
                h = (h + 1) & mask;
            }
            if (slot >= 0) atomicMin(&L.vmin[slot], (unsigned)v);
            else err = SM_ERR_FULL;
        }
        L.slot_v[v] = slot;
    }
    sm_raise(totals, err);
}

// the smallest member of v's cluster (v itself where it has no slot: the call is an error then, and stays in bounds)
__device__ __forceinline__ int sm_smallest(const SmLayout& L, int v)
{
    const int s = L.slot_v[v];
    return s < 0 ? v : (int)L.vmin[s];
}

__global__ void __launch_bounds__(SM_BLOCK) sm_flag_verts_kernel(int n_verts, SmLayout L)
{
    const int v = blockIdx.x * SM_BLOCK + threadIdx.x;
    const int flag = v < n_verts && sm_smallest(L, v) == v;
    int tot;
    const int off = block_excl_scan<SM_BLOCK>(flag, &tot);
    if (v < n_verts) L.word_v[v] = off << 1 | flag;
    if (threadIdx.x == 0) L.sums_v[blockIdx.x] = tot;
}

// offs = exclusive scan of sums (nb words), *total = their sum; one workgroup
__global__ void __launch_bounds__(SM_SCAN_THREADS) sm_scan_blocks_kernel(const int32_t* __restrict__ sums,
                                                                         int32_t* __restrict__ offs, int nb,
                                                                         int32_t* __restrict__ total)
{
    // the carry is at most n_verts or n_faces
    const int tot = block_carry_scan<SM_SCAN_THREADS, int>(
        nb, [&](int b) { return sums[b]; }, [&](int b, int excl) { offs[b] = excl; });
    if (threadIdx.x == 0) *total = tot;
}

__global__ void __launch_bounds__(SM_BLOCK) sm_number_kernel(int n_verts, SmLayout L)
{
    const int v = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (v >= n_verts) return;
    const int r = sm_smallest(L, v);
    L.cluster[v] = L.offs_v[r / SM_BLOCK] + (L.word_v[r] >> 1);
}

struct SmTriple {
    int c[3];   // cluster numbers of the corners, in corner order
    int s[3];   // the same, ascending
};

__device__ __forceinline__ SmTriple sm_triple(const int32_t* __restrict__ faces, const int32_t* __restrict__ cluster,
                                              int f)
{
    SmTriple t;
#pragma unroll
    for (int q = 0; q < 3; q++) t.c[q] = cluster[faces[3 * (int64_t)f + q]];
    const int lo = min(t.c[0], min(t.c[1], t.c[2])), hi = max(t.c[0], max(t.c[1], t.c[2]));
    t.s[0] = lo;
    t.s[1] = (int)((int64_t)t.c[0] + t.c[1] + t.c[2] - lo - hi);
    t.s[2] = hi;
    return t;
}

__global__ void __launch_bounds__(SM_BLOCK) sm_insert_faces_kernel(const int32_t* __restrict__ faces, int n_faces,
                                                                   SmLayout L, int32_t* __restrict__ totals)
{
    const int f = blockIdx.x * SM_BLOCK + threadIdx.x;
    int err = 0;
    bool degenerate = false;
    if (f < n_faces) {
        const SmTriple t = sm_triple(faces, L.cluster, f);
        int slot = -1;
        degenerate = t.s[0] == t.s[1] || t.s[1] == t.s[2];
        if (!degenerate) {
            const unsigned mask = (unsigned)L.cap_f - 1;
            const unsigned long long s0 = (unsigned)t.s[0], s1 = (unsigned)t.s[1], s2 = (unsigned)t.s[2];
            unsigned h = sm_mix(s0 << 42 ^ s1 << 21 ^ s2) & mask;
            for (int step = 0; step < L.cap_f; step++) {   // bounded by the capacity
                const int was = atomicCAS(&L.fany[h], -1, f);
                bool mine = was == -1 || was == f;
                if (!mine) {   // the slot's face: its corners and their clusters were written by earlier launches
                    const SmTriple u = sm_triple(faces, L.cluster, was);
                    mine = u.s[0] == t.s[0] && u.s[1] == t.s[1] && u.s[2] == t.s[2];
                }
                if (mine) {
                    slot = (int)h;
                    break;
                }
                h = (h + 1) & mask;
            }
            if (slot >= 0) atomicMin(&L.fmin[slot], (unsigned)f);
            else err = SM_ERR_FULL;
        }
        L.slot_f[f] = slot;
    }
    const unsigned long long deg = __ballot(degenerate);
    if (deg && (threadIdx.x & (NGP_WAVE - 1)) == 0) atomicAdd(&totals[SM_T_DEGENERATE], (int)__popcll(deg));
    sm_raise(totals, err);
}

__global__ void __launch_bounds__(SM_BLOCK) sm_flag_faces_kernel(int n_faces, SmLayout L)
{
    const int f = blockIdx.x * SM_BLOCK + threadIdx.x;
    int flag = 0;
    if (f < n_faces) {
        const int s = L.slot_f[f];
        flag = s >= 0 && (int)L.fmin[s] == f;
    }
    int tot;
    const int off = block_excl_scan<SM_BLOCK>(flag, &tot);
    if (f < n_faces) L.word_f[f] = off << 1 | flag;
    if (threadIdx.x == 0) L.sums_f[blockIdx.x] = tot;
}

// ------------------------------------------------------------------------------------------------------------ emit
__global__ void __launch_bounds__(SM_BLOCK) sm_groups_kernel(const int32_t* __restrict__ faces, int n_faces,
                                                             int n_verts, SmLayout L,
                                                             int32_t* __restrict__ vert_cluster,
                                                             int32_t* __restrict__ corner_cluster)
{
    const int64_t i = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i < n_verts) vert_cluster[i] = L.cluster[i];
    if (i < 3 * (int64_t)n_faces) corner_cluster[i] = L.cluster[faces[i]];
}

// first index i of the ascending array a (n) with a[i] >= c
__device__ __forceinline__ int sm_lower_bound(const int32_t* __restrict__ a, int n, int c)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (a[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct SmPlace {
    const float* verts;
    const int32_t* faces;
    const int32_t* sorted_v;   // (n_verts) cluster numbers, ascending
    const int32_t* order_v;    // (n_verts) the vertex of each entry: ascending inside a cluster
    const int32_t* sorted_c;   // (3 n_faces) cluster numbers of the corners, ascending
    const int32_t* order_c;    // (3 n_faces) 3 * face + corner of each entry: ascending inside a cluster
    const float* normals;      // (n_verts, 3) or NULL
    const uint8_t* colors;     // (n_verts, 3) or NULL
    float* verts_out;          // (n_clusters, 3)
    float* normals_out;
    uint8_t* colors_out;
    int n_verts, n_corners, n_clusters, quadric;
    float o[3], cell, inv;
    double regularization;
};

// x of the symmetric positive definite system A x = r by Cholesky (A: xx xy xz yy yz zz); false: not positive
__device__ __forceinline__ bool sm_solve_spd(const double A[6], const double r[3], double x[3])
{
    const double d0 = A[0];
    if (!(d0 > 0.0)) return false;
    const double l00 = sqrt(d0), l10 = A[1] / l00, l20 = A[2] / l00;
    const double d1 = A[3] - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = sqrt(d1), l21 = (A[4] - l20 * l10) / l11;
    const double d2 = A[5] - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) return false;
    const double l22 = sqrt(d2);
    const double y0 = r[0] / l00, y1 = (r[1] - l10 * y0) / l11, y2 = (r[2] - l20 * y0 - l21 * y1) / l22;
    x[2] = y2 / l22;
    x[1] = (y1 - l21 * x[2]) / l11;
    x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
    return true;
}

__global__ void __launch_bounds__(SM_BLOCK) sm_place_kernel(SmPlace P)
{
    const int c = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (c >= P.n_clusters) return;
    // members, ascending vertex index
    int i = sm_lower_bound(P.sorted_v, P.n_verts, c);
    double m[3] = {0, 0, 0}, ns[3] = {0, 0, 0};
    long long cs[3] = {0, 0, 0}, count = 0;
    unsigned key[3] = {0, 0, 0};
    for (; i < P.n_verts && P.sorted_v[i] == c; i++) {
        const int64_t v = P.order_v[i];
        if (count == 0) sm_cell(P.verts + 3 * v, P.o[0], P.o[1], P.o[2], P.inv, key);
        count++;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            m[a] += (double)P.verts[3 * v + a];
            if (P.normals) ns[a] += (double)P.normals[3 * v + a];
            if (P.colors) cs[a] += P.colors[3 * v + a];
        }
    }
    if (count == 0) return;   // every cluster has a member; an inconsistent sort writes nothing
    double x[3];
#pragma unroll
    for (int a = 0; a < 3; a++) x[a] = m[a] = m[a] / (double)count;
    if (P.quadric) {
        // corners, ascending (face, corner): each adds its face's n n^T and d n
        double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
        for (int j = sm_lower_bound(P.sorted_c, P.n_corners, c); j < P.n_corners && P.sorted_c[j] == c; j++) {
            const int64_t f = P.order_c[j] / 3;
            double p[3][3];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const int64_t v = P.faces[3 * f + q];
#pragma unroll
                for (int a = 0; a < 3; a++) p[q][a] = (double)P.verts[3 * v + a];
            }
            const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
            const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
            const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                                 e1[0] * e2[1] - e1[1] * e2[0]};
            const double d = n[0] * p[0][0] + n[1] * p[0][1] + n[2] * p[0][2];
            A[0] += n[0] * n[0];
            A[1] += n[0] * n[1];
            A[2] += n[0] * n[2];
            A[3] += n[1] * n[1];
            A[4] += n[1] * n[2];
            A[5] += n[2] * n[2];
#pragma unroll
            for (int a = 0; a < 3; a++) b[a] += d * n[a];
        }
        const double t = A[0] + A[3] + A[5];
        if (t != 0.0 && isfinite(t)) {
            const double lam = P.regularization * t / 3.0;
            const double M[6] = {A[0] + lam, A[1], A[2], A[3] + lam, A[4], A[5] + lam};
            const double r[3] = {b[0] + lam * m[0], b[1] + lam * m[1], b[2] + lam * m[2]};
            double s[3];
            if (sm_solve_spd(M, r, s)) {
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const double lo = (double)P.o[a] + (double)key[a] * (double)P.cell;
                    const double hi = (double)P.o[a] + ((double)key[a] + 1.0) * (double)P.cell;
                    x[a] = fmin(fmax(s[a], lo), hi);
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) P.verts_out[3 * (int64_t)c + a] = (float)x[a];
    if (P.normals) {
        const double mean[3] = {ns[0] / (double)count, ns[1] / (double)count, ns[2] / (double)count};
        const double len = sqrt(mean[0] * mean[0] + mean[1] * mean[1] + mean[2] * mean[2]);
#pragma unroll
        for (int a = 0; a < 3; a++)
            P.normals_out[3 * (int64_t)c + a] = len > 0.0 && isfinite(len) ? (float)(mean[a] / len) : 0.f;
    }
    if (P.colors) {
#pragma unroll
        for (int a = 0; a < 3; a++)   // floor(mean + 0.5) in integers
            P.colors_out[3 * (int64_t)c + a] = (uint8_t)((2 * cs[a] + count) / (2 * count));
    }
}

__global__ void __launch_bounds__(SM_BLOCK) sm_emit_faces_kernel(const int32_t* __restrict__ faces, int n_faces,
                                                                 SmLayout L, int32_t* __restrict__ faces_out,
                                                                 int32_t* __restrict__ used)
{
    const int f = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int w = L.word_f[f];
    if (!(w & 1)) return;
    const int64_t slot = (int64_t)L.offs_f[f / SM_BLOCK] + (w >> 1);
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int c = L.cluster[faces[3 * (int64_t)f + q]];
        faces_out[3 * slot + q] = c;
        atomicAdd(&used[c], 1);   // spread over the clusters: at most a few faces meet at one
    }
}

}  // namespace

extern "C" {

int64_t ngp_mesh_simplify_workspace(int n_verts, int n_faces)
{
    if (!sm_sizes_ok(n_verts, n_faces)) return NGP_EINVAL;
    return sm_layout(nullptr, n_verts, n_faces).words;
}

int ngp_mesh_simplify_count(const float* verts, int n_verts, const int32_t* faces, int n_faces, const float* origin3,
                            float inv_cell, int32_t* workspace, int32_t* totals, void* stream)
{
    if (!sm_sizes_ok(n_verts, n_faces)) return NGP_EINVAL;
    if (n_verts == 0) return NGP_OK;
    if (!verts || !origin3 || !workspace || !totals || (n_faces && !faces)) return NGP_EINVAL;
    if (!(inv_cell > 0.f) || !isfinite(inv_cell) || (uintptr_t)workspace % 8) return NGP_EINVAL;
    const SmLayout L = sm_layout(workspace, n_verts, n_faces);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(SM_BLOCK);
    const unsigned fill_blocks = ngp_blocks(L.table_words, SM_BLOCK * 16);   // grid-stride: 16 words per thread or more
    hipLaunchKernelGGL(sm_fill_kernel, dim3(fill_blocks < 4096u ? fill_blocks : 4096u), block, 0, st, workspace,
                       L.table_words, totals);
    hipLaunchKernelGGL(sm_insert_verts_kernel, dim3(L.nb_v), block, 0, st, verts, n_verts, origin3[0], origin3[1],
                       origin3[2], inv_cell, L, totals);
    hipLaunchKernelGGL(sm_flag_verts_kernel, dim3(L.nb_v), block, 0, st, n_verts, L);
    hipLaunchKernelGGL(sm_scan_blocks_kernel, dim3(1), dim3(SM_SCAN_THREADS), 0, st, L.sums_v, L.offs_v, L.nb_v,
                       totals + SM_T_CLUSTERS);
    hipLaunchKernelGGL(sm_number_kernel, dim3(L.nb_v), block, 0, st, n_verts, L);
    if (n_faces) {
        hipLaunchKernelGGL(sm_insert_faces_kernel, dim3(L.nb_f), block, 0, st, faces, n_faces, L, totals);
        hipLaunchKernelGGL(sm_flag_faces_kernel, dim3(L.nb_f), block, 0, st, n_faces, L);
        hipLaunchKernelGGL(sm_scan_blocks_kernel, dim3(1), dim3(SM_SCAN_THREADS), 0, st, L.sums_f, L.offs_f, L.nb_f,
                           totals + SM_T_KEPT);
    }
    return ngp_check_launch();
}

int ngp_mesh_simplify_groups(const int32_t* faces, int n_faces, int n_verts, const int32_t* workspace,
                             int32_t* vert_cluster, int32_t* corner_cluster, void* stream)
{
    if (!sm_sizes_ok(n_verts, n_faces)) return NGP_EINVAL;
    if (n_verts == 0) return NGP_OK;
    if (!workspace || !vert_cluster || (n_faces && (!faces || !corner_cluster))) return NGP_EINVAL;
    const SmLayout L = sm_layout((int32_t*)workspace, n_verts, n_faces);
    const int64_t n = 3 * (int64_t)n_faces > n_verts ? 3 * (int64_t)n_faces : n_verts;
    hipLaunchKernelGGL(sm_groups_kernel, dim3(ngp_blocks(n, SM_BLOCK)), dim3(SM_BLOCK), 0, (hipStream_t)stream, faces,
                       n_faces, n_verts, L, vert_cluster, corner_cluster);
    return ngp_check_launch();
}

int ngp_mesh_simplify_place(const float* verts, int n_verts, const int32_t* faces, int n_faces,
                            const float* origin3, float cell, float inv_cell, double regularization, int quadric,
                            int n_clusters, const int32_t* sorted_v, const int32_t* order_v, const int32_t* sorted_c,
                            const int32_t* order_c, const float* normals, const uint8_t* colors, float* verts_out,
                            float* normals_out, uint8_t* colors_out, void* stream)
{
    if (!sm_sizes_ok(n_verts, n_faces) || n_clusters < 0 || n_clusters > n_verts) return NGP_EINVAL;
    if (n_verts == 0 || n_clusters == 0) return NGP_OK;
    if (!verts || !origin3 || !sorted_v || !order_v || !verts_out) return NGP_EINVAL;
    if (n_faces && (!faces || !sorted_c || !order_c)) return NGP_EINVAL;
    if ((normals && !normals_out) || (colors && !colors_out)) return NGP_EINVAL;
    if (!(cell > 0.f) || !(inv_cell > 0.f) || !isfinite(cell) || !isfinite(inv_cell)) return NGP_EINVAL;
    if (!(regularization > 0.0) || !isfinite(regularization)) return NGP_EINVAL;
    SmPlace P;
    P.verts = verts;
    P.faces = faces;
    P.sorted_v = sorted_v;
    P.order_v = order_v;
    P.sorted_c = sorted_c;
    P.order_c = order_c;
    P.normals = normals;
    P.colors = colors;
    P.verts_out = verts_out;
    P.normals_out = normals_out;
    P.colors_out = colors_out;
    P.n_verts = n_verts;
    P.n_corners = 3 * n_faces;
    P.n_clusters = n_clusters;
    P.quadric = quadric != 0;
    for (int a = 0; a < 3; a++) P.o[a] = origin3[a];
    P.cell = cell;
    P.inv = inv_cell;
    P.regularization = regularization;
    hipLaunchKernelGGL(sm_place_kernel, dim3(sm_blocks(n_clusters)), dim3(SM_BLOCK), 0, (hipStream_t)stream, P);
    return ngp_check_launch();
}

int ngp_mesh_simplify_faces(const int32_t* faces, int n_faces, int n_verts, const int32_t* workspace,
                            int32_t* faces_out, int32_t* used, void* stream)
{
    if (!sm_sizes_ok(n_verts, n_faces)) return NGP_EINVAL;
    if (n_verts == 0 || n_faces == 0) return NGP_OK;
    if (!faces || !workspace || !faces_out || !used) return NGP_EINVAL;
    const SmLayout L = sm_layout((int32_t*)workspace, n_verts, n_faces);
    hipLaunchKernelGGL(sm_emit_faces_kernel, dim3(L.nb_f), dim3(SM_BLOCK), 0, (hipStream_t)stream, faces, n_faces, L,
                       faces_out, used);
    return ngp_check_launch();
}

}  // extern "C"
