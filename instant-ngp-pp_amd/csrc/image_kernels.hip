// Image-shaped outputs of the test-time renderer: SSIM of rendered frames against ground truth (what the reference's
// validation step logs through torchmetrics, train.py:93,353-386) and the 8-bit frames its render.py writes
// (render.py:17-31,150-185, utils.py:84-95).  Compiled without FMA contraction (build.py): the frame packing is
// compared bit for bit with a float32 numpy restatement.
//
// SSIM (Wang et al. 2004, Gaussian weights).  Images are (H*W, 3) float rows, channel-last, as render() returns them.
// Window 11x11, separable, taps exp(-x^2 / (2 * 1.5^2)) normalised to sum 1 (computed in double on the host, rounded
// once to float, passed by value); valid windows only: (H-10) x (W-10) positions.  One launch forms every moment:
//   a workgroup of 256 threads owns SSIM_TILE x SSIM_TILE window positions; it stages the (TILE+10)^2 input pixels of
//   both images and all three channels in LDS once, then per channel runs the row pass (5 moments per staged row and
//   output column, kept in LDS) and the column pass (one thread per window position), and adds the channel's SSIM
//   into a per-thread sum.  Nothing filtered ever goes to HBM.
// Flat regions.  sigma^2 = E[x^2] - mu^2 cancels catastrophically in float when the patch is nearly constant (a white
//   background: both terms ~1, their difference ~1e-6).  Moments of (x - p) have the same variances and covariance for
//   any constant p, so the staged values are x - p with p the tile's centre pixel (per image and channel): on a flat
//   patch E[(x-p)^2] and mu'^2 are both tiny and the difference is exact enough; mu = p + mu' goes into the luminance
//   term, where nothing cancels.  One pivot serves the whole 26x26 tile: a window that lies on another flat level of a
//   tile straddling an edge is evaluated no better than in plain float32 (measured cases: DESIGN.md section 7).
// Determinism.  The 256 per-thread sums are added in double by a fixed LDS tree into partial[image][tile]; a second
//   launch (one workgroup per image) adds an image's tiles in double in a fixed order and writes mean = sum / (3 *
//   positions) as float.  No atomics: two runs give the same bits, and so does image i of a batch and the same image
//   alone (its tiles, their order and the grid in x and y do not depend on `count`).
//
// Frame packing.  One thread per ray, one launch per frame, every output optional; float32 in the order written in
// include/ngp_hip.h, truncating conversion to uint8 as numpy's astype does for values in [0, 255].
//
// Resampling.  Pillow's 8-bit antialiased bicubic resize (ImagingResample: precomputed 22-bit fixed-point taps, a
// horizontal pass into an 8-bit intermediate, then a vertical pass), for the supersampled frames of
// --anti_aliasing_factor.  Integers only.  One launch: a workgroup owns tile_w x tile_h output pixels, stages the
// input window those need in LDS, writes the row pass to LDS and runs the column pass from there; the intermediate
// image never exists in HBM.  The host picks the tile from the ratio so that window + intermediate fit RS_LDS_BYTES.
#include "common.h"
#include <math.h>

namespace {

constexpr int SSIM_R = 5;                        // window radius: 11 taps
constexpr int SSIM_TAPS = 2 * SSIM_R + 1;
constexpr int SSIM_TILE = 16;                    // window positions per workgroup and axis
constexpr int SSIM_IN = SSIM_TILE + 2 * SSIM_R;  // staged input pixels per axis
constexpr int SSIM_THREADS = SSIM_TILE * SSIM_TILE;
constexpr int SSIM_REDUCE_THREADS = 256;
constexpr int PACK_BLOCK = 256;

struct SsimTaps {
    float w[SSIM_TAPS];
};

// fixed-order sum of one double per thread (THREADS a power of two); the total is returned to thread 0
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* red)
{
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(SSIM_THREADS) ssim_tile_kernel(const float* __restrict__ pred,
                                                                 const float* __restrict__ gt, int H, int W,
                                                                 SsimTaps taps, double* __restrict__ partial)
{
    __shared__ float sx[3][SSIM_IN][SSIM_IN + 1];       // pred - pivot
    __shared__ float sy[3][SSIM_IN][SSIM_IN + 1];       // gt - pivot
    __shared__ float hm[5][SSIM_IN][SSIM_TILE + 1];     // row-filtered moments of one channel
    __shared__ double red[SSIM_THREADS];

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SSIM_TILE, y0 = blockIdx.y * SSIM_TILE;   // first window position = first input pixel
    const int64_t base = (int64_t)blockIdx.z * H * W * 3;
    const float* __restrict__ P = pred + base;
    const float* __restrict__ G = gt + base;

    // the tile's pivots: its centre pixel, clamped into the image
    const int py = min(y0 + SSIM_IN / 2, H - 1), px = min(x0 + SSIM_IN / 2, W - 1);
    const int64_t pv = ((int64_t)py * W + px) * 3;
    const float pvx[3] = {P[pv], P[pv + 1], P[pv + 2]};
    const float pvy[3] = {G[pv], G[pv + 1], G[pv + 2]};

    // stage: rows of SSIM_IN pixels x 3 channels are contiguous in memory
    for (int i = tid; i < SSIM_IN * SSIM_IN * 3; i += SSIM_THREADS) {
        const int r = i / (SSIM_IN * 3), e = i - r * (SSIM_IN * 3);
        const int c = e / 3, ch = e - c * 3;
        const int gy = y0 + r, gx = x0 + c;
        float a = 0.f, b = 0.f;
        if (gy < H && gx < W) {
            const int64_t o = ((int64_t)gy * W + gx) * 3 + ch;
            a = P[o] - pvx[ch];
            b = G[o] - pvy[ch];
        }
        sx[ch][r][c] = a;
        sy[ch][r][c] = b;
    }
    __syncthreads();

    const int tx = tid % SSIM_TILE, ty = tid / SSIM_TILE;
    const bool valid = x0 + tx < W - 2 * SSIM_R && y0 + ty < H - 2 * SSIM_R;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    float acc = 0.f;
    for (int ch = 0; ch < 3; ch++) {
        // rows
        for (int i = tid; i < SSIM_IN * SSIM_TILE; i += SSIM_THREADS) {
            const int r = i / SSIM_TILE, c = i - r * SSIM_TILE;
            float mx = 0.f, my = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
            for (int k = 0; k < SSIM_TAPS; k++) {
                const float w = taps.w[k], a = sx[ch][r][c + k], b = sy[ch][r][c + k];
                const float wa = w * a, wb = w * b;
                mx += wa;
                my += wb;
                xx += wa * a;
                yy += wb * b;
                xy += wa * b;
            }
            hm[0][r][c] = mx;
            hm[1][r][c] = my;
            hm[2][r][c] = xx;
            hm[3][r][c] = yy;
            hm[4][r][c] = xy;
        }
        __syncthreads();
        // columns
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SSIM_TAPS; k++) {
            const float w = taps.w[k];
#pragma unroll
            for (int q = 0; q < 5; q++) m[q] += w * hm[q][ty + k][tx];
        }
        const float mux = pvx[ch] + m[0], muy = pvy[ch] + m[1];
        const float vx = m[2] - m[0] * m[0], vy = m[3] - m[1] * m[1], cxy = m[4] - m[0] * m[1];
        const float num = (2.f * mux * muy + C1) * (2.f * cxy + C2);
        const float den = (mux * mux + muy * muy + C1) * (vx + vy + C2);
        if (valid) acc += num / den;
        __syncthreads();   // hm is rewritten by the next channel
    }
    const double total = block_sum<SSIM_THREADS>((double)acc, red);
    if (tid == 0)
        partial[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

__global__ void __launch_bounds__(SSIM_REDUCE_THREADS) ssim_reduce_kernel(const double* __restrict__ partial,
                                                                          int tiles, double inv_n,
                                                                          float* __restrict__ out)
{
    __shared__ double red[SSIM_REDUCE_THREADS];
    const double* __restrict__ p = partial + (int64_t)blockIdx.x * tiles;
    double s = 0.0;
    for (int i = threadIdx.x; i < tiles; i += SSIM_REDUCE_THREADS) s += p[i];
    const double total = block_sum<SSIM_REDUCE_THREADS>(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(total * inv_n);
}

int ssim_tiles(int v) { return (v - 2 * SSIM_R + SSIM_TILE - 1) / SSIM_TILE; }

// ---------------------------------------------------------------------------------------------------- frame packing
__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ uint8_t u8(float v) { return (uint8_t)(int)(clip01(v) * 255.f); }

struct PackArgs {
    const float* rgb;
    const float* opacity;
    const float* depth;
    const float* normal_pred;
    const float* normal_raw;
    const int64_t* semantic;
    const float* R;
    const uint8_t* lut;
    uint8_t* rgb_u8;
    uint8_t* opacity_u8;
    uint8_t* depth_u8;
    uint8_t* normal_u8;
    uint8_t* normal_raw_u8;
    uint8_t* semantic_u8;
    float depth_scale;
    float level;
};

__device__ __forceinline__ void pack_normal(const float* __restrict__ nrm, const float* R, int64_t i,
                                            uint8_t* __restrict__ out)
{
    const float n0 = nrm[3 * i] + 1e-6f, n1 = nrm[3 * i + 1] + 1e-6f, n2 = nrm[3 * i + 2] + 1e-6f;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float c = (n0 * R[j] + n1 * R[3 + j]) + n2 * R[6 + j];
        out[3 * i + j] = u8((c + 1.f) / 2.f);
    }
}

__device__ __forceinline__ void pack_lut(const uint8_t* __restrict__ lut, float v, int64_t i, uint8_t* __restrict__ out)
{
    const int k = u8(v);
#pragma unroll
    for (int j = 0; j < 3; j++) out[3 * i + j] = lut[3 * k + j];
}

__global__ void __launch_bounds__(PACK_BLOCK) frame_pack_kernel(PackArgs a, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * PACK_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (a.rgb_u8) {
#pragma unroll
        for (int j = 0; j < 3; j++) a.rgb_u8[3 * i + j] = u8(a.rgb[3 * i + j]);
    }
    if (a.opacity_u8) a.opacity_u8[i] = u8(a.opacity[i]);
    if (a.depth_u8) pack_lut(a.lut, a.depth[i] / a.depth_scale, i, a.depth_u8);
    if (a.normal_u8 || a.normal_raw_u8) {
        float R[9];
#pragma unroll
        for (int j = 0; j < 9; j++) R[j] = a.R[j];
        if (a.normal_u8) pack_normal(a.normal_pred, R, i, a.normal_u8);
        if (a.normal_raw_u8) pack_normal(a.normal_raw, R, i, a.normal_raw_u8);
    }
    if (a.semantic_u8) pack_lut(a.lut, a.level * (float)a.semantic[i], i, a.semantic_u8);
}

// ------------------------------------------------------------------------------------------------------- resampling
constexpr int RS_THREADS = 256;
constexpr int RS_BITS = 22;                      // Pillow's PRECISION_BITS for 8-bit images
constexpr int RS_MAX_RATIO = 8;
constexpr int RS_LDS_BYTES = 48 * 1024;          // window + intermediate of the chosen tile stay at or under this

struct ResizeArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* kx;   // (out_w, ksize_x) taps, NULL: the axis is unchanged
    const int32_t* bx;   // (out_w, 2) first input column and tap count
    const int32_t* ky;
    const int32_t* by;
    int in_h, in_w, out_h, out_w, ch;
    int ksize_x, ksize_y;
    int tile_w, tile_h;  // output pixels per workgroup
    int win_w, win_h;    // staged input pixels per workgroup (an upper bound of what any tile needs)
};

__device__ __forceinline__ uint8_t rs_clip8(int acc)
{
    return (uint8_t)min(max(acc >> RS_BITS, 0), 255);
}

// sum over n taps of v[i * stride] * k[i], rounded as Pillow rounds
__device__ __forceinline__ uint8_t rs_filter(const uint8_t* v, int stride, const int32_t* __restrict__ k, int n)
{
    int acc = 1 << (RS_BITS - 1);
    for (int i = 0; i < n; i++) acc += (int)v[i * stride] * k[i];
    return rs_clip8(acc);
}

__global__ void __launch_bounds__(RS_THREADS) resize_bicubic_u8_kernel(ResizeArgs a)
{
    extern __shared__ uint8_t rs_lds[];
    const int C = a.ch;
    const int win_pitch = a.win_w * C, mid_pitch = a.tile_w * C;
    uint8_t* win = rs_lds;                          // [win_h][win_w * C] input window
    uint8_t* mid = rs_lds + a.win_h * win_pitch;    // [win_h][tile_w * C] row-filtered window

    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * a.tile_w, oy0 = blockIdx.y * a.tile_h;
    const int tw = min(a.tile_w, a.out_w - ox0), th = min(a.tile_h, a.out_h - oy0);
    // the first input column / row any output of the tile reads: the bounds do not decrease along an axis.  Every
    // index taken from the bounds is clamped into what was staged, whatever the arrays hold.
    const int ix0 = a.kx ? min(max(a.bx[2 * ox0], 0), a.in_w - 1) : ox0;
    const int iy0 = a.ky ? min(max(a.by[2 * oy0], 0), a.in_h - 1) : oy0;
    const int ww = min(a.win_w, a.in_w - ix0), wh = min(a.win_h, a.in_h - iy0);
    const uint8_t* __restrict__ S = a.src + (int64_t)blockIdx.z * a.in_h * a.in_w * C;
    uint8_t* __restrict__ D = a.dst + (int64_t)blockIdx.z * a.out_h * a.out_w * C;

    // stage: a window row is ww * C contiguous bytes
    const int row_bytes = ww * C;
    for (int i = tid; i < wh * row_bytes; i += RS_THREADS) {
        const int r = i / row_bytes, e = i - r * row_bytes;
        win[r * win_pitch + e] = S[((int64_t)(iy0 + r) * a.in_w + ix0) * C + e];
    }
    __syncthreads();

    // rows: every staged row to the tile's tw output columns
    const int out_bytes = tw * C;
    for (int i = tid; i < wh * out_bytes; i += RS_THREADS) {
        const int r = i / out_bytes, e = i - r * out_bytes;
        uint8_t v;
        if (a.kx) {
            const int c = e / C, ch = e - c * C, xx = ox0 + c;
            const int off = a.bx[2 * xx] - ix0;
            int n = min(a.bx[2 * xx + 1], a.ksize_x);
            n = (off < 0 || off > ww) ? 0 : min(n, ww - off);
            v = rs_filter(win + r * win_pitch + off * C + ch, C, a.kx + (int64_t)xx * a.ksize_x, n);
        } else {
            v = win[r * win_pitch + e];
        }
        mid[r * mid_pitch + e] = v;
    }
    __syncthreads();

    // columns
    for (int i = tid; i < th * out_bytes; i += RS_THREADS) {
        const int r = i / out_bytes, e = i - r * out_bytes;
        uint8_t v;
        if (a.ky) {
            const int yy = oy0 + r;
            const int off = a.by[2 * yy] - iy0;
            int n = min(a.by[2 * yy + 1], a.ksize_y);
            n = (off < 0 || off > wh) ? 0 : min(n, wh - off);
            v = rs_filter(mid + off * mid_pitch + e, mid_pitch, a.ky + (int64_t)yy * a.ksize_y, n);
        } else {
            v = mid[r * mid_pitch + e];
        }
        D[((int64_t)(oy0 + r) * a.out_w + ox0) * C + e] = v;
    }
}

// Pillow's tap count for n_in -> n_out samples
int rs_ksize(int n_in, int n_out)
{
    const double scale = (double)n_in / (double)n_out;
    return (int)ceil(2.0 * (scale > 1.0 ? scale : 1.0)) * 2 + 1;
}

// input samples a tile of `tile` outputs can read: its centres span (tile - 1) * scale, and a row of taps starts no
// earlier than centre - support - 0.5 and ends no later than centre + support + 0.5
int rs_window(int n_in, int n_out, int tile)
{
    if (n_in == n_out) return tile;
    const double scale = (double)n_in / (double)n_out, support = 2.0 * (scale > 1.0 ? scale : 1.0);
    const double span = floor((tile - 1) * scale + 2.0 * support) + 2.0;
    return span < (double)n_in ? (int)span : n_in;
}

}  // namespace

extern "C" {

int64_t ngp_ssim_workspace(int count, int H, int W)
{
    if (count < 0 || H < SSIM_TAPS || W < SSIM_TAPS) return NGP_EINVAL;
    const int64_t tiles = (int64_t)ssim_tiles(H) * ssim_tiles(W);
    if ((int64_t)H * W > INT32_MAX / 3 || ssim_tiles(H) > 65535 || count > 65535) return NGP_EINVAL;
    return tiles * count;
}

int ngp_ssim(const float* pred, const float* gt, int count, int H, int W, double* partial, float* out, void* stream)
{
    if (count < 0) return NGP_EINVAL;
    if (count == 0) return NGP_OK;
    if (ngp_ssim_workspace(count, H, W) < 0 || !pred || !gt || !partial || !out) return NGP_EINVAL;
    SsimTaps taps;
    double g[SSIM_TAPS], sum = 0.0;
    for (int k = 0; k < SSIM_TAPS; k++) {
        const double x = k - SSIM_R;
        g[k] = exp(-x * x / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    for (int k = 0; k < SSIM_TAPS; k++) taps.w[k] = (float)(g[k] / sum);
    const int tx = ssim_tiles(W), ty = ssim_tiles(H);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ssim_tile_kernel, dim3(tx, ty, count), dim3(SSIM_THREADS), 0, st, pred, gt, H, W, taps,
                       partial);
    const double inv_n = 1.0 / (3.0 * (double)(H - 2 * SSIM_R) * (double)(W - 2 * SSIM_R));
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(count), dim3(SSIM_REDUCE_THREADS), 0, st, partial, tx * ty, inv_n,
                       out);
    return ngp_check_launch();
}

int ngp_frame_pack(int64_t n, const float* rgb, const float* opacity, const float* depth, float depth_scale,
                   const float* normal_pred, const float* normal_raw, const float* R, const int64_t* semantic,
                   int classes, const uint8_t* lut, uint8_t* rgb_u8, uint8_t* opacity_u8, uint8_t* depth_u8,
                   uint8_t* normal_u8, uint8_t* normal_raw_u8, uint8_t* semantic_u8, void* stream)
{
    if (n < 0) return NGP_EINVAL;
    if (n == 0) return NGP_OK;
    if (n > INT64_MAX / 3 || (n + PACK_BLOCK - 1) / PACK_BLOCK > INT32_MAX) return NGP_EINVAL;
    if ((rgb_u8 && !rgb) || (opacity_u8 && !opacity) || (depth_u8 && (!depth || !lut)) ||
        (normal_u8 && (!normal_pred || !R)) || (normal_raw_u8 && (!normal_raw || !R)) ||
        (semantic_u8 && (!semantic || !lut || classes < 2)))
        return NGP_EINVAL;
    if (!rgb_u8 && !opacity_u8 && !depth_u8 && !normal_u8 && !normal_raw_u8 && !semantic_u8) return NGP_OK;
    PackArgs a;
    a.rgb = rgb;
    a.opacity = opacity;
    a.depth = depth;
    a.normal_pred = normal_pred;
    a.normal_raw = normal_raw;
    a.semantic = semantic;
    a.R = R;
    a.lut = lut;
    a.rgb_u8 = rgb_u8;
    a.opacity_u8 = opacity_u8;
    a.depth_u8 = depth_u8;
    a.normal_u8 = normal_u8;
    a.normal_raw_u8 = normal_raw_u8;
    a.semantic_u8 = semantic_u8;
    a.depth_scale = depth_scale;
    a.level = classes >= 2 ? 1.0f / (float)(classes - 1) : 0.f;
    hipLaunchKernelGGL(frame_pack_kernel, dim3((unsigned)((n + PACK_BLOCK - 1) / PACK_BLOCK)), dim3(PACK_BLOCK), 0,
                       (hipStream_t)stream, a, n);
    return ngp_check_launch();
}

int ngp_resize_bicubic_u8(const uint8_t* src, int count, int in_h, int in_w, int channels, uint8_t* dst, int out_h,
                          int out_w, const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky,
                          const int32_t* by, int ksize_y, void* stream)
{
    if (count < 0) return NGP_EINVAL;
    if (count == 0) return NGP_OK;
    if (channels != 1 && channels != 3) return NGP_EINVAL;
    if (in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 || count > 65535) return NGP_EINVAL;
    if ((int64_t)in_h > (int64_t)RS_MAX_RATIO * out_h || (int64_t)in_w > (int64_t)RS_MAX_RATIO * out_w)
        return NGP_EINVAL;
    const bool pass_x = in_w != out_w, pass_y = in_h != out_h;
    if (!src || !dst || (pass_x && (!kx || !bx)) || (pass_y && (!ky || !by))) return NGP_EINVAL;
    if ((pass_x && ksize_x != rs_ksize(in_w, out_w)) || (pass_y && ksize_y != rs_ksize(in_h, out_h)))
        return NGP_EINVAL;
    ResizeArgs a;
    a.src = src;
    a.dst = dst;
    a.kx = pass_x ? kx : nullptr;
    a.bx = pass_x ? bx : nullptr;
    a.ky = pass_y ? ky : nullptr;
    a.by = pass_y ? by : nullptr;
    a.in_h = in_h;
    a.in_w = in_w;
    a.out_h = out_h;
    a.out_w = out_w;
    a.ch = channels;
    a.ksize_x = ksize_x;
    a.ksize_y = ksize_y;
    // the largest tile whose window and intermediate fit the budget: 32 x 16 up to ratio 4 on both axes with three
    // channels, 16 x 8 (45.9 KB) at ratio 8
    static const int tiles[][2] = {{32, 16}, {32, 8}, {16, 16}, {16, 8}};
    int lds = 0;
    for (const auto& t : tiles) {
        a.tile_w = t[0];
        a.tile_h = t[1];
        a.win_w = rs_window(in_w, out_w, a.tile_w);
        a.win_h = rs_window(in_h, out_h, a.tile_h);
        lds = a.win_h * (a.win_w + a.tile_w) * channels;
        if (lds <= RS_LDS_BYTES) break;
    }
    if (lds > RS_LDS_BYTES) return NGP_EINVAL;
    const int64_t gx = (out_w + a.tile_w - 1) / a.tile_w, gy = (out_h + a.tile_h - 1) / a.tile_h;
    if (gy > 65535) return NGP_EINVAL;
    hipLaunchKernelGGL(resize_bicubic_u8_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)count), dim3(RS_THREADS),
                       (size_t)lds, (hipStream_t)stream, a);
    return ngp_check_launch();
}

}  // extern "C"
