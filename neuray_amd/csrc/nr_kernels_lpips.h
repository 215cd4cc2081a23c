// LPIPS (learned perceptual image patch similarity, VGG variant) of the evaluation protocol - eval.py:16,24-27 lpips.LPIPS(net='vgg') -
// for inference: the pieces around the thirteen 3 x 3 convolutions, twelve of which run on conv2d_x3_kernel (nr_kernels_conv2d.h, with the
// ReLU epilogue).  The network is written from the published formula; its weights come from the caller.
//   stem     input uint8 [n][h][w][3] (decoded image files; eval.py's own arithmetic in fp32: x = u8 / 255f, then x * 2 - 1) or fp32
//            [n][3][h][w] in [-1, 1]; the scaling layer (x - shift[c]) / scale[c]; conv1_1 (3 -> C1, 3 x 3, padding 1) + bias + ReLU,
//            written NCHW.  The zero padding is in the SCALED space (a padded tap contributes 0).  One thread per pixel: its 27 scaled
//            inputs in registers, the weights in LDS (wave-uniform reads), per output channel
//                acc = 0;  for ci, ky, kx (in this order): acc = acc + w[co][ci][ky][kx] * x[ci][ky][kx];  out = max(acc + bias[co], 0)
//            as separate fp32 multiplies and adds (the library is built with contraction off).
//   maxpool  NCHW, window 2, stride 2, floor: out[y][x] = max of in[2y .. 2y + 1][2x .. 2x + 1]; an odd last row / column is dropped.
//   head     one tap: f0, f1 [.][C][h][w], lin [C] -> per pair the mean over the pixels of
//                sum_c lin[c] (f0[c] / s0 - f1[c] / s1)^2,   s = sqrt(sum_c f[c]^2) + 1e-10.
//            Two passes over the channels in fp64 (never the expanded a^2 - 2ab + b^2, which cancels for near-identical images); the
//            division is one fp64 reciprocal per pixel and image and a multiply per channel.  Lanes walk pixels (contiguous in NCHW) and
//            loop over channels in index order.  A workgroup owns kLpTile consecutive pixels of one pair (thread t: pixels t, t + 256, ...
//            in that order), a fixed tree adds its 256 sums, the tile partials are added per pair by a second launch in tile order: no
//            float atomics, a pair's value depends neither on the other pairs of the batch nor on the run.  lin may be negative.
#pragma once
#include "nr_platform.h"

namespace nr {

constexpr int kLpThreads = 256;
constexpr int kLpTile = 4 * kLpThreads;          // pixels per workgroup of the head
constexpr int kLpStemMaxC = 512;                 // widest first layer the stem's LDS plan takes (28 floats per output channel)

struct LpipsStemParams {
    const void* img;         // uint8 [n][h][w][3] or fp32 [n][3][h][w]
    const float* wgt;        // [cout][3][3][3]
    const float* bias;       // [cout]
    float* out;              // [n][cout][h][w]
    float shift[3], scale[3];
    int n, cout, h, w, u8;
};

template <bool U8>
__global__ void __launch_bounds__(kLpThreads) lpips_stem_kernel(LpipsStemParams p) {
    NR_DYNAMIC_SMEM(float, wl);                                            // [cout][27] weights, [cout] bias
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < p.cout * 27; i += kLpThreads) wl[i] = p.wgt[i];
    for (int i = tid; i < p.cout; i += kLpThreads) wl[p.cout * 27 + i] = p.bias[i];
    __syncthreads();
    const size_t plane = (size_t)p.h * p.w;
    const size_t pix = (size_t)blockIdx.x * kLpThreads + tid;             // (n, y, x) of this thread
    if (pix >= (size_t)p.n * plane) return;
    const int img = (int)(pix / plane);
    const int rem = (int)(pix - (size_t)img * plane);
    const int y = rem / p.w, x = rem - y * p.w;
    float v[27];
    NR_PRAGMA_UNROLL
    for (int ci = 0; ci < 3; ++ci)
        NR_PRAGMA_UNROLL
        for (int ky = 0; ky < 3; ++ky)
            NR_PRAGMA_UNROLL
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = y + ky - 1, xx = x + kx - 1;
                float s = 0.0f;
                if (yy >= 0 && yy < p.h && xx >= 0 && xx < p.w) {
                    float t;
                    if constexpr (U8) {
                        const unsigned char u = static_cast<const unsigned char*>(p.img)[((size_t)img * plane + (size_t)yy * p.w + xx) * 3 + ci];
                        t = (float)u / 255.0f;
                        t = t * 2.0f - 1.0f;
                    } else {
                        t = static_cast<const float*>(p.img)[((size_t)img * 3 + ci) * plane + (size_t)yy * p.w + xx];
                    }
                    s = (t - p.shift[ci]) / p.scale[ci];
                }
                v[(ci * 3 + ky) * 3 + kx] = s;
            }
    float* o = p.out + (size_t)img * p.cout * plane + rem;
    const float* bl = wl + p.cout * 27;
    for (int co = 0; co < p.cout; ++co) {
        const float* wc = wl + co * 27;
        float acc = 0.0f;
        NR_PRAGMA_UNROLL
        for (int k = 0; k < 27; ++k) acc = acc + wc[k] * v[k];
        acc = acc + bl[co];
        o[(size_t)co * plane] = acc > 0.0f ? acc : 0.0f;
    }
}

struct MaxPoolParams {
    const float* x;          // [planes][h][w]
    float* out;              // [planes][h / 2][w / 2]
    long long total;         // planes * (h / 2) * (w / 2)
    int h, w;
};

__global__ void __launch_bounds__(kLpThreads) maxpool2x2_kernel(MaxPoolParams p) {
    const long long i = (long long)blockIdx.x * kLpThreads + (int)threadIdx.x;
    if (i >= p.total) return;
    const int oh = p.h / 2, ow = p.w / 2;
    const long long row = i / ow;                        // plane * oh + y
    const int x = (int)(i - row * ow);
    const long long pl = row / oh;
    const int y = (int)(row - pl * oh);
    const float* s = p.x + ((size_t)pl * p.h + 2 * y) * p.w + 2 * x;
    const float2 a = make_float2(s[0], s[1]), b = make_float2(s[p.w], s[p.w + 1]);
    p.out[i] = fmaxf(fmaxf(a.x, a.y), fmaxf(b.x, b.y));
}

struct LpipsHeadParams {
    const float* f0;         // [n][c][h * w]
    const float* f1;         // pair i reads image i * f1_stride
    const float* lin;        // [c]
    double* ws;              // [n][tiles]
    double* out;             // pair i -> out[i * out_stride]
    int n, f1_stride, c, tiles, out_stride;
    long long plane;         // h * w
};

__global__ void __launch_bounds__(kLpThreads) lpips_head_tile_kernel(LpipsHeadParams p) {
    __shared__ double red[kLpThreads];
    const int tid = (int)threadIdx.x;
    const int pair = (int)blockIdx.x / p.tiles, tile = (int)blockIdx.x - pair * p.tiles;
    const float* a = p.f0 + (size_t)pair * p.c * p.plane;
    const float* b = p.f1 + (size_t)pair * p.f1_stride * p.c * p.plane;
    double t = 0.0;
    for (int k = 0; k < kLpTile / kLpThreads; ++k) {
        const long long px = (long long)tile * kLpTile + k * kLpThreads + tid;
        if (px >= p.plane) break;
        const float* pa = a + px;
        const float* pb = b + px;
        double s0 = 0.0, s1 = 0.0;
        NR_PRAGMA_UNROLL4
        for (int c = 0; c < p.c; ++c) {
            const double u = pa[(size_t)c * p.plane], v = pb[(size_t)c * p.plane];
            s0 += u * u;
            s1 += v * v;
        }
        const double r0 = 1.0 / (sqrt(s0) + 1e-10), r1 = 1.0 / (sqrt(s1) + 1e-10);
        double acc = 0.0;
        NR_PRAGMA_UNROLL4
        for (int c = 0; c < p.c; ++c) {
            const double d = (double)pa[(size_t)c * p.plane] * r0 - (double)pb[(size_t)c * p.plane] * r1;
            acc += (double)p.lin[c] * (d * d);
        }
        t += acc;
    }
    red[tid] = t;
    for (int s = kLpThreads / 2; s > 0; s >>= 1) {        // fixed-order tree over the workgroup
        __syncthreads();
        if (tid < s) red[tid] += red[tid + s];
    }
    if (tid == 0) p.ws[(size_t)pair * p.tiles + tile] = red[0];
}

// one workgroup per pair: the tile partials in tile order (thread t: tiles t, t + 64, ...), then a fixed tree over the 64 lanes
__global__ void __launch_bounds__(64) lpips_head_reduce_kernel(LpipsHeadParams p) {
    __shared__ double red[64];
    const int tid = (int)threadIdx.x, pair = (int)blockIdx.x;
    const double* w = p.ws + (size_t)pair * p.tiles;
    double s = 0.0;
    for (int t = tid; t < p.tiles; t += 64) s += w[t];
    red[tid] = s;
    for (int k = 32; k > 0; k >>= 1) {
        __syncthreads();
        if (tid < k) red[tid] += red[tid + k];
    }
    if (tid == 0) p.out[(size_t)pair * p.out_stride] = red[0] / (double)p.plane;
}

}  // namespace nr
