// Image-quality metrics of the reference's validation (network/metrics.py: PSNR_SSIM, compute_psnr, skimage's
// structural_similarity) and evaluation (eval.py: tf.image.ssim), for a batch of n image pairs of one size h x w x 3:
//   quantisation  utils/base_utils.py:496-499 color_map_backward on fp32 input: clip(x * 255f, 0, 255) truncated to uint8
//                 (NaN -> 0), fused into the load; uint8 input (decoded image files) is taken as it is
//   SSE           sum of squared uint8 differences over the region of interest (ROI), exact (integer accumulation)
//   SSIM box11    skimage structural_similarity(win_size=11, data_range=255): 11 x 11 uniform window, sample covariance
//                 (121 / 120).  skimage filters with reflect padding and crops 5 pixels from each side afterwards, so every
//                 surviving window lies inside the image: the mean over the (h-10) (w-10) valid positions, no border handling.
//                 The window sums of x, y, x^2, y^2, xy are 32-bit integers (121 * 255^2 < 2^31), exact; the per-position term
//                 is then one fp64 expression of exact integers.
//   SSIM gauss11  tf.image.ssim(max_val=255 on the integer values; SSIM is scale invariant): the normalised 11 x 11 Gaussian
//                 (sigma 1.5) as two 1-D passes of fp64 weighted sums, VALID positions, biased moments, luminance x cs.
// Both: K1 = 0.01, K2 = 0.03, per channel the mean over the valid window positions inside the ROI, then the channel mean.
// One workgroup per (pair, tile of 16 x 64 window positions): the tile's pixels + 10-pixel halo of both images are staged
// in LDS (quantised on the way in), then per channel the horizontal 11-tap sums go to LDS and each thread sums 11 of them
// vertically per position.  Every sum runs in a fixed order and the tile partials (three fp64 channel sums, one uint64
// SSE) are reduced per pair by a second kernel in tile order: no float atomics, a pair's result does not depend on the
// other pairs of the batch or on the run.
#pragma once
#include "nr_platform.h"

namespace nr {

constexpr int kMetWin = 11;                           // window side (both variants)
constexpr int kMetTH = 16, kMetTW = 64;               // window positions per tile: rows, columns
constexpr int kMetRows = kMetTH + kMetWin - 1;        // staged pixel rows / columns of a tile
constexpr int kMetCols = kMetTW + kMetWin - 1;
constexpr int kMetThreads = 256;
constexpr int kMetStage = (kMetRows * kMetCols * 3 + 15) / 16 * 16;   // bytes of one image's staged tile (uint8)
constexpr int kMetPartial = 4;                        // per tile: fp64 SSIM-term sums of the 3 channels, uint64 SSE

template <bool GAUSS> struct MetAcc { typedef int T; };           // box11: exact integer window sums
template <> struct MetAcc<true> { typedef double T; };            // gauss11: fp64 weighted sums

// LDS of the tile kernel: staged gt / pred, channel sums [3][256] fp64, SSE [256], horizontal sums [5][kMetRows][kMetTW]
template <bool GAUSS>
constexpr size_t metrics_smem_bytes() {
    return 2 * (size_t)kMetStage + 3 * kMetThreads * 8 + kMetThreads * 8 + 5 * (size_t)kMetRows * kMetTW * sizeof(typename MetAcc<GAUSS>::T);
}

struct MetricsParams {
    const void* pred;              // fp32 [n][h*w][3] or uint8 [n][h][w][3]
    const void* gt;                // same type; pair i reads image i * gt_stride
    unsigned char* quant;          // optional uint8 [n][h][w][3]: the quantised pred (ROI pixels)
    unsigned long long* sse;       // [n]
    double* ssim;                  // [n]
    double* ws;                    // [n][tiles][kMetPartial]
    int n, gt_stride, u8, h, w;
    int y0, y1, x0, x1;            // ROI, half-open; at least 11 x 11
    int tiles_y, tiles_x;
    double taps[kMetWin];          // gauss11: the normalised 1-D Gaussian
};

// color_map_backward: one fp32 multiply, clamp to [0, 255], truncation toward zero; NaN -> 0 (numpy's cast on x86-64)
__device__ __forceinline__ unsigned char met_quantise(float x) {
    const float v = x * 255.0f;
    return (unsigned char)(v > 0.0f ? (v < 255.0f ? (int)v : 255) : 0);
}

// skimage's S over one window from the exact integer sums: with A1 = 2 ux uy + C1, A2 = 2 vxy + C2, B1 = ux^2 + uy^2 + C1,
// B2 = vx + vy + C2 (ux = sx / 121, vx = (sxx / 121 - ux^2) 121 / 120, ...) the ratio is A1 A2 / (B1 B2) =
// (2 sx sy + 121^2 C1)(2 (121 sxy - sx sy) + 121 120 C2) / ((sx^2 + sy^2 + 121^2 C1)(121 sxx - sx^2 + 121 syy - sy^2 + 121 120 C2)):
// the four integer parts are exact in int64 (identical images: numerator and denominator are the same doubles, S = 1 exactly)
__device__ __forceinline__ double met_box_term(int sx, int sy, int sxx, int syy, int sxy) {
    const double c1 = (0.01 * 255.0) * (0.01 * 255.0) * 14641.0, c2 = (0.03 * 255.0) * (0.03 * 255.0) * 14520.0;
    const long long x = sx, y = sy;
    const long long n1 = 2 * x * y, d1 = x * x + y * y;
    const long long n2 = 2 * (121 * (long long)sxy - x * y), d2 = (121 * (long long)sxx - x * x) + (121 * (long long)syy - y * y);
    return (((double)n1 + c1) * ((double)n2 + c2)) / (((double)d1 + c1) * ((double)d2 + c2));
}

// tf.image.ssim's _ssim_helper on the window's weighted moments (compensation 1), max_val 255
__device__ __forceinline__ double met_gauss_term(double mx, double my, double mxx, double myy, double mxy) {
    const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
    const double num0 = mx * my * 2.0, den0 = mx * mx + my * my;
    const double lum = (num0 + c1) / (den0 + c1);
    const double num1 = mxy * 2.0, den1 = mxx + myy;
    const double cs = (num1 - num0 + c2) / (den1 - den0 + c2);
    return lum * cs;
}

template <bool GAUSS>
__global__ void __launch_bounds__(kMetThreads) image_metrics_tile_kernel(MetricsParams p) {
    typedef typename MetAcc<GAUSS>::T Acc;
    NR_DYNAMIC_SMEM(unsigned char, lds);
    unsigned char* xs = lds;                                               // gt   [kMetRows][kMetCols][3]
    unsigned char* ys = lds + kMetStage;                                   // pred
    double* red = reinterpret_cast<double*>(lds + 2 * kMetStage);          // [3][kMetThreads]
    unsigned long long* red_sse = reinterpret_cast<unsigned long long*>(red + 3 * kMetThreads);
    Acc* hb = reinterpret_cast<Acc*>(red_sse + kMetThreads);               // [5][kMetRows][kMetTW]
    const int tid = (int)threadIdx.x;
    const int ntiles = p.tiles_y * p.tiles_x;
    const int pair = (int)blockIdx.x / ntiles, tile = (int)blockIdx.x - pair * ntiles;
    const int by = tile / p.tiles_x, bx = tile - by * p.tiles_x;
    const int ty = p.y0 + by * kMetTH, tx = p.x0 + bx * kMetTW;           // first window position (= its top-left pixel)
    const int th_all = p.y1 - (kMetWin - 1) - ty, tw_all = p.x1 - (kMetWin - 1) - tx;      // window positions left in the ROI
    const int th = th_all < kMetTH ? th_all : kMetTH, tw = tw_all < kMetTW ? tw_all : kMetTW;
    const int rows = th + kMetWin - 1, cols = tw + kMetWin - 1;           // staged pixels: all inside the ROI
    // pixels this tile counts for SSE / writes quantised: its window rows and columns, + the last 10 on the ROI's last tile row / column
    const int own_r = by == p.tiles_y - 1 ? rows : th, own_c3 = 3 * (bx == p.tiles_x - 1 ? cols : tw);
    const size_t img = (size_t)p.h * p.w * 3;
    const size_t po = (size_t)pair * img, go = (size_t)pair * p.gt_stride * img;

    unsigned long long sse = 0;
    const int cols3 = 3 * cols;
    for (int i = tid; i < rows * cols3; i += kMetThreads) {
        const int r = i / cols3, k = i - r * cols3;
        const size_t g = ((size_t)(ty + r) * p.w + tx) * 3 + k;
        unsigned char a, b;
        if (p.u8) {
            a = static_cast<const unsigned char*>(p.pred)[po + g];
            b = static_cast<const unsigned char*>(p.gt)[go + g];
        } else {
            a = met_quantise(static_cast<const float*>(p.pred)[po + g]);
            b = met_quantise(static_cast<const float*>(p.gt)[go + g]);
        }
        ys[r * kMetCols * 3 + k] = a;
        xs[r * kMetCols * 3 + k] = b;
        if (r < own_r && k < own_c3) {
            const int d = (int)a - (int)b;
            sse += (unsigned)(d * d);
            if (p.quant) p.quant[po + g] = a;
        }
    }

    for (int c = 0; c < 3; ++c) {
        __syncthreads();                                   // staging / the previous channel's vertical pass is done with hb
        for (int i = tid; i < rows * kMetTW; i += kMetThreads) {
            const int r = i / kMetTW, j = i - r * kMetTW;
            if (j >= tw) continue;
            const unsigned char* xr = xs + (r * kMetCols + j) * 3 + c;
            const unsigned char* yr = ys + (r * kMetCols + j) * 3 + c;
            Acc s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
            NR_PRAGMA_UNROLL
            for (int k = 0; k < kMetWin; ++k) {
                const int x = xr[3 * k], y = yr[3 * k];
                if constexpr (GAUSS) {
                    const double g = p.taps[k];
                    s0 += g * x; s1 += g * y; s2 += g * (x * x); s3 += g * (y * y); s4 += g * (x * y);
                } else {
                    s0 += x; s1 += y; s2 += x * x; s3 += y * y; s4 += x * y;
                }
            }
            Acc* o = hb + r * kMetTW + j;
            o[0] = s0; o[kMetRows * kMetTW] = s1; o[2 * kMetRows * kMetTW] = s2; o[3 * kMetRows * kMetTW] = s3; o[4 * kMetRows * kMetTW] = s4;
        }
        __syncthreads();
        double t = 0.0;                                    // this thread's positions: column tid % 64, rows tid / 64 + 4 m
        const int j = tid & (kMetTW - 1);
        if (j < tw) {
            for (int i = tid / kMetTW; i < th; i += kMetThreads / kMetTW) {
                const Acc* v = hb + i * kMetTW + j;
                Acc s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
                NR_PRAGMA_UNROLL
                for (int k = 0; k < kMetWin; ++k) {
                    const Acc* u = v + k * kMetTW;
                    if constexpr (GAUSS) {
                        const double g = p.taps[k];
                        s0 += g * u[0]; s1 += g * u[kMetRows * kMetTW]; s2 += g * u[2 * kMetRows * kMetTW];
                        s3 += g * u[3 * kMetRows * kMetTW]; s4 += g * u[4 * kMetRows * kMetTW];
                    } else {
                        s0 += u[0]; s1 += u[kMetRows * kMetTW]; s2 += u[2 * kMetRows * kMetTW];
                        s3 += u[3 * kMetRows * kMetTW]; s4 += u[4 * kMetRows * kMetTW];
                    }
                }
                if constexpr (GAUSS) t += met_gauss_term(s0, s1, s2, s3, s4);
                else t += met_box_term(s0, s1, s2, s3, s4);
            }
        }
        red[c * kMetThreads + tid] = t;
    }
    red_sse[tid] = sse;
    for (int s = kMetThreads / 2; s > 0; s >>= 1) {       // fixed-order tree over the workgroup
        __syncthreads();
        if (tid < s) {
            for (int c = 0; c < 3; ++c) red[c * kMetThreads + tid] += red[c * kMetThreads + tid + s];
            red_sse[tid] += red_sse[tid + s];
        }
    }
    if (tid == 0) {
        double* o = p.ws + ((size_t)pair * ntiles + tile) * kMetPartial;
        o[0] = red[0]; o[1] = red[kMetThreads]; o[2] = red[2 * kMetThreads];
        reinterpret_cast<unsigned long long*>(o)[3] = red_sse[0];
    }
}

// one workgroup per pair: the tile partials in tile order (thread t: tiles t, t + 64, ...), then a fixed tree over the 64 lanes
__global__ void __launch_bounds__(64) image_metrics_reduce_kernel(MetricsParams p) {
    NR_DYNAMIC_SMEM(double, red);                          // [3][64] channel sums, [64] SSE (as uint64)
    unsigned long long* red_sse = reinterpret_cast<unsigned long long*>(red + 3 * 64);
    const int tid = (int)threadIdx.x, pair = (int)blockIdx.x;
    const int ntiles = p.tiles_y * p.tiles_x;
    const double* w = p.ws + (size_t)pair * ntiles * kMetPartial;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    unsigned long long e = 0;
    for (int t = tid; t < ntiles; t += 64) {
        s0 += w[t * kMetPartial]; s1 += w[t * kMetPartial + 1]; s2 += w[t * kMetPartial + 2];
        e += reinterpret_cast<const unsigned long long*>(w)[t * kMetPartial + 3];
    }
    red[tid] = s0; red[64 + tid] = s1; red[128 + tid] = s2; red_sse[tid] = e;
    for (int s = 32; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            red[tid] += red[tid + s]; red[64 + tid] += red[64 + tid + s]; red[128 + tid] += red[128 + tid + s];
            red_sse[tid] += red_sse[tid + s];
        }
    }
    if (tid == 0) {
        const double cnt = (double)(p.y1 - p.y0 - (kMetWin - 1)) * (double)(p.x1 - p.x0 - (kMetWin - 1));
        p.sse[pair] = red_sse[0];
        p.ssim[pair] = (red[0] / cnt + red[64] / cnt + red[128] / cnt) / 3.0;
    }
}

}  // namespace nr
