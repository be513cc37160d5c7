// Connected components and compaction of a triangle mesh (mesh cleaning: mesh.py clean_mesh, tools/extract_mesh.py).
//
// Labels.  labels[v] ends as the smallest vertex index of v's component (two faces are connected when they share a
// vertex; a vertex in no face keeps its own index), so the result does not depend on thread order.  No launch relies
// on one workgroup seeing another's stores within that launch (per-CU L1s and per-XCD L2s are not coherent): every
// value a thread reads is either current or an older value of the same slot, and every write only moves a label down
// to another index of the same component.  A round is two launches:
//   hook  one thread per face: the labels a, b, c of its corners are each lowered to m = min(a, b, c) with atomicMin
//         (a label read that is already <= m is skipped: a stale read is never below the slot's current value);
//   jump  one thread per vertex: labels[v] = labels[labels[v]], followed for at most CC_JUMP_STEPS links;
// and either sets *changed when it lowered some label.  The host reads the word after each round and stops at the
// first round that changed nothing: then every label is a root and every face's corners share it, so each root is its
// component's smallest index.  Each changing round lowers the sum of the labels, so the loop ends.
//
// Sizes.  Faces per component by integer atomics at the root's slot, aggregated per wave (a big component would
// otherwise serialise one atomic per face on one word).
//
// Compaction.  Two calls, as ngp_mc_count / ngp_mc_emit.  The count call flags each kept vertex (its component is
// kept and has a face) and each kept face (its component is kept), scans the flags inside each workgroup (one word
// per element: local offset << 1 | flag) and scans the workgroup sums in one workgroup into offsets and the totals.
// The emit calls copy kept vertex rows (any row width: positions, normals, colours) and kept faces, with their
// corners renumbered, in their original order.
#include "common.h"

namespace {

constexpr int CC_BLOCK = 256;           // threads per workgroup of every per-element pass (4 waves)
constexpr int CC_SCAN_THREADS = 1024;   // the single workgroup of the block-sum scan
constexpr int CC_JUMP_STEPS = 8;        // links a jump thread follows per launch (bounded: no wait on other threads)

__global__ void __launch_bounds__(CC_BLOCK) cc_init_kernel(int32_t* __restrict__ labels, int n_verts)
{
    const int v = blockIdx.x * CC_BLOCK + threadIdx.x;
    if (v < n_verts) labels[v] = v;
}

__global__ void __launch_bounds__(CC_BLOCK) cc_hook_kernel(const int32_t* __restrict__ faces, int n_faces,
                                                           int32_t* labels, int32_t* __restrict__ changed)
{
    const int f = blockIdx.x * CC_BLOCK + threadIdx.x;
    bool lowered = false;
    if (f < n_faces) {
        const int64_t o = 3 * (int64_t)f;
        const int a = labels[faces[o]], b = labels[faces[o + 1]], c = labels[faces[o + 2]];
        const int m = min(a, min(b, c));
        const int r[3] = {a, b, c};
#pragma unroll
        for (int q = 0; q < 3; q++) {
            if (r[q] == m || labels[r[q]] <= m) continue;
            lowered |= atomicMin(&labels[r[q]], m) > m;
        }
    }
    if (__any(lowered) && (threadIdx.x & (NGP_WAVE - 1)) == 0) changed[0] = 1;
}

__global__ void __launch_bounds__(CC_BLOCK) cc_jump_kernel(int32_t* labels, int n_verts,
                                                           int32_t* __restrict__ changed)
{
    const int v = blockIdx.x * CC_BLOCK + threadIdx.x;
    bool lowered = false;
    if (v < n_verts) {
        const int p0 = labels[v];   // only this thread writes labels[v] in this launch
        int p = p0;
        for (int s = 0; s < CC_JUMP_STEPS; s++) {
            const int q = labels[p];
            if (q == p) break;
            p = q;
        }
        if (p != p0) {
            labels[v] = p;
            lowered = true;
        }
    }
    if (__any(lowered) && (threadIdx.x & (NGP_WAVE - 1)) == 0) changed[0] = 1;
}

__global__ void __launch_bounds__(CC_BLOCK) cc_zero_kernel(int32_t* __restrict__ x, int n)
{
    const int i = blockIdx.x * CC_BLOCK + threadIdx.x;
    if (i < n) x[i] = 0;
}

__global__ void __launch_bounds__(CC_BLOCK) cc_face_count_kernel(const int32_t* __restrict__ faces, int n_faces,
                                                                 const int32_t* __restrict__ labels,
                                                                 int32_t* __restrict__ face_counts)
{
    const int f = blockIdx.x * CC_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (NGP_WAVE - 1);
    int lab = f < n_faces ? labels[faces[3 * (int64_t)f]] : -1;
    // one atomic per distinct label of the wave: each pass retires the lanes of the lowest active lane's label
    unsigned long long todo = __ballot(lab >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int want = __shfl(lab, leader, NGP_WAVE);
        const unsigned long long same = __ballot(lab == want) & todo;
        if (lane == leader) atomicAdd(&face_counts[want], (int)__popcll(same));
        todo &= ~same;
    }
}

struct CcLayout {   // workspace of the compaction: int32 words
    int32_t* word_v;      // (n_verts)  local offset << 1 | kept
    int32_t* word_f;      // (n_faces)
    int32_t* sums;        // (nb_v + nb_f) workgroup sums, vertex workgroups first
    int32_t* offs;        // (nb_v + nb_f) their exclusive scans, each part on its own
    int nb_v, nb_f;
};

int cc_blocks(int n) { return (n + CC_BLOCK - 1) / CC_BLOCK; }

CcLayout cc_layout(int32_t* ws, int n_verts, int n_faces)
{
    CcLayout L;
    L.nb_v = cc_blocks(n_verts);
    L.nb_f = cc_blocks(n_faces);
    L.word_v = ws;
    L.word_f = ws + n_verts;
    L.sums = L.word_f + n_faces;
    L.offs = L.sums + L.nb_v + L.nb_f;
    return L;
}

// workgroups [0, nb_v) flag vertices, [nb_v, nb_v + nb_f) faces
__global__ void __launch_bounds__(CC_BLOCK) cc_flag_kernel(const int32_t* __restrict__ faces, int n_faces, int n_verts,
                                                           const int32_t* __restrict__ labels,
                                                           const int32_t* __restrict__ face_counts,
                                                           const uint8_t* __restrict__ keep, CcLayout L)
{
    const bool is_v = (int)blockIdx.x < L.nb_v;
    const int i = (is_v ? blockIdx.x : blockIdx.x - L.nb_v) * CC_BLOCK + threadIdx.x;
    int flag = 0;
    if (is_v && i < n_verts) {
        const int lab = labels[i];
        flag = keep[lab] && face_counts[lab] > 0;
    } else if (!is_v && i < n_faces) {
        flag = keep[labels[faces[3 * (int64_t)i]]] != 0;
    }
    int tot;
    const int off = block_excl_scan<CC_BLOCK>(flag, &tot);
    if (is_v && i < n_verts) L.word_v[i] = off << 1 | flag;
    if (!is_v && i < n_faces) L.word_f[i] = off << 1 | flag;
    if (threadIdx.x == 0) L.sums[blockIdx.x] = tot;
}

// exclusive scans of the vertex and face workgroup sums; totals[0] = kept vertices, totals[1] = kept faces
__global__ void __launch_bounds__(CC_SCAN_THREADS) cc_scan_blocks_kernel(CcLayout L, int32_t* __restrict__ totals)
{
    for (int part = 0; part < 2; part++) {
        const int32_t* sums = L.sums + (part ? L.nb_v : 0);
        int32_t* offs = L.offs + (part ? L.nb_v : 0);
        // the carry is at most n_verts or n_faces < 2^31
        const int tot = block_carry_scan<CC_SCAN_THREADS, int>(
            part ? L.nb_f : L.nb_v, [&](int b) { return sums[b]; }, [&](int b, int excl) { offs[b] = excl; });
        if (threadIdx.x == 0) totals[part] = tot;
    }
}

// kept vertex rows, row_bytes each, copied in 4-byte words when rows and buffers allow it
template <typename T>
__global__ void __launch_bounds__(CC_BLOCK) cc_emit_rows_kernel(const T* __restrict__ src, int row_elems, int n_verts,
                                                                CcLayout L, T* __restrict__ dst)
{
    const int v = blockIdx.x * CC_BLOCK + threadIdx.x;
    if (v >= n_verts) return;
    const int w = L.word_v[v];
    if (!(w & 1)) return;
    const int64_t slot = (int64_t)L.offs[v / CC_BLOCK] + (w >> 1);
    const T* s = src + (int64_t)v * row_elems;
    T* d = dst + slot * row_elems;
    for (int e = 0; e < row_elems; e++) d[e] = s[e];
}

__global__ void __launch_bounds__(CC_BLOCK) cc_emit_faces_kernel(const int32_t* __restrict__ faces, int n_faces,
                                                                 CcLayout L, int32_t* __restrict__ faces_out)
{
    const int f = blockIdx.x * CC_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int w = L.word_f[f];
    if (!(w & 1)) return;
    const int64_t slot = (int64_t)L.offs[L.nb_v + f / CC_BLOCK] + (w >> 1);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int v = faces[3 * (int64_t)f + c];
        faces_out[3 * slot + c] = L.offs[v / CC_BLOCK] + (L.word_v[v] >> 1);
    }
}

}  // namespace

extern "C" {

int64_t ngp_mesh_clean_workspace(int n_verts, int n_faces)
{
    if (n_verts < 0 || n_faces < 0) return NGP_EINVAL;
    if (n_faces > INT32_MAX / 3) return NGP_EINVAL;   // 3 * n_faces indices are addressed by the callers as int32
    return (int64_t)n_verts + n_faces + 2 * ((int64_t)cc_blocks(n_verts) + cc_blocks(n_faces));
}

int ngp_mesh_labels_init(int32_t* labels, int n_verts, void* stream)
{
    if (n_verts < 0) return NGP_EINVAL;
    if (n_verts == 0) return NGP_OK;
    if (!labels) return NGP_EINVAL;
    hipLaunchKernelGGL(cc_init_kernel, dim3(cc_blocks(n_verts)), dim3(CC_BLOCK), 0, (hipStream_t)stream, labels,
                       n_verts);
    return ngp_check_launch();
}

int ngp_mesh_labels_round(const int32_t* faces, int n_faces, int n_verts, int32_t* labels, int32_t* changed,
                          void* stream)
{
    if (n_verts < 0 || n_faces < 0) return NGP_EINVAL;
    if (n_verts == 0 || n_faces == 0) return NGP_OK;
    if (!faces || !labels || !changed) return NGP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_hook_kernel, dim3(cc_blocks(n_faces)), dim3(CC_BLOCK), 0, st, faces, n_faces, labels,
                       changed);
    hipLaunchKernelGGL(cc_jump_kernel, dim3(cc_blocks(n_verts)), dim3(CC_BLOCK), 0, st, labels, n_verts, changed);
    return ngp_check_launch();
}

int ngp_mesh_face_counts(const int32_t* faces, int n_faces, int n_verts, const int32_t* labels, int32_t* face_counts,
                         void* stream)
{
    if (n_verts < 0 || n_faces < 0) return NGP_EINVAL;
    if (n_verts == 0) return NGP_OK;
    if (!labels || !face_counts || (n_faces && !faces)) return NGP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_zero_kernel, dim3(cc_blocks(n_verts)), dim3(CC_BLOCK), 0, st, face_counts, n_verts);
    if (n_faces)
        hipLaunchKernelGGL(cc_face_count_kernel, dim3(cc_blocks(n_faces)), dim3(CC_BLOCK), 0, st, faces, n_faces,
                           labels, face_counts);
    return ngp_check_launch();
}

int ngp_mesh_compact_count(const int32_t* faces, int n_faces, int n_verts, const int32_t* labels,
                           const int32_t* face_counts, const uint8_t* keep, int32_t* workspace, int32_t* totals,
                           void* stream)
{
    if (ngp_mesh_clean_workspace(n_verts, n_faces) < 0) return NGP_EINVAL;
    if (n_verts == 0) return NGP_OK;
    if (!labels || !face_counts || !keep || !workspace || !totals || (n_faces && !faces)) return NGP_EINVAL;
    const CcLayout L = cc_layout(workspace, n_verts, n_faces);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_flag_kernel, dim3(L.nb_v + L.nb_f), dim3(CC_BLOCK), 0, st, faces, n_faces, n_verts, labels,
                       face_counts, keep, L);
    hipLaunchKernelGGL(cc_scan_blocks_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, L, totals);
    return ngp_check_launch();
}

int ngp_mesh_compact_rows(const void* src, int row_bytes, int n_verts, int n_faces, const int32_t* workspace,
                          void* dst, void* stream)
{
    if (ngp_mesh_clean_workspace(n_verts, n_faces) < 0 || row_bytes < 0) return NGP_EINVAL;
    if (n_verts == 0 || row_bytes == 0) return NGP_OK;
    if (!src || !workspace || !dst) return NGP_EINVAL;
    const CcLayout L = cc_layout((int32_t*)workspace, n_verts, n_faces);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(L.nb_v), block(CC_BLOCK);
    if (row_bytes % 4 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0)
        hipLaunchKernelGGL(cc_emit_rows_kernel<int32_t>, grid, block, 0, st, (const int32_t*)src, row_bytes / 4,
                           n_verts, L, (int32_t*)dst);
    else
        hipLaunchKernelGGL(cc_emit_rows_kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)src, row_bytes, n_verts,
                           L, (uint8_t*)dst);
    return ngp_check_launch();
}

int ngp_mesh_compact_faces(const int32_t* faces, int n_faces, int n_verts, const int32_t* workspace,
                           int32_t* faces_out, void* stream)
{
    if (ngp_mesh_clean_workspace(n_verts, n_faces) < 0) return NGP_EINVAL;
    if (n_faces == 0 || n_verts == 0) return NGP_OK;
    if (!faces || !workspace || !faces_out) return NGP_EINVAL;
    const CcLayout L = cc_layout((int32_t*)workspace, n_verts, n_faces);
    hipLaunchKernelGGL(cc_emit_faces_kernel, dim3(L.nb_f), dim3(CC_BLOCK), 0, (hipStream_t)stream, faces, n_faces, L,
                       faces_out);
    return ngp_check_launch();
}

}  // extern "C"
