// Plane-sweep stereo (neuray_amd/stereo.py): posed images + a depth range per view -> a depth map per view.  The
// arithmetic is stereo.plane_sweep_numpy's, operation by operation and in its order, in fp32 without contraction (no fmaf in this file).
//
// One workgroup (256 threads, one output pixel each) per 16 x 16 tile of one reference view; it walks all D planes itself and keeps the
// best cost, its two neighbours and the winner in registers: no cost volume is ever in memory.  Per (plane, source):
//   warp      every pixel of the tile plus its halo of r is projected once and the source gray fetched bilinearly into LDS (one gather per
//             LDS pixel, not (2r+1)^2 per output pixel); a pixel outside the reference image, behind the source camera or projecting outside
//             the source image is stored as NaN
//   rows      S_s, S_ss, S_rs of every LDS row for the 16 window columns, added left to right
//   columns   each thread adds its window's 2r+1 row sums top to bottom -> ZNCC cost
// A NaN in a window makes its sums NaN, and every comparison that accepts a cost is false for a NaN: that is the validity count, at no cost.
// The reference image's own sums are made once per tile.  The per-(view, slot) constants M, b, the depth range and nn_ids are read at
// wave-uniform addresses (scalar loads), as nr_kernels_fuse.h reads its cameras.  Two barriers per (plane, source): the warp stage writes
// `src` after every thread has left the previous row stage, the row stage writes `rows` after every thread has left the previous column stage.
//
// Tile skipping.  q = d (M (x, y, 1)) + b is evaluated as d * ((M0 * x + M1 * y) + M2) + b0: every rounded operation is monotone in its
// operands, so the computed q0, q1, q2 are monotone in x for fixed y and in y for fixed x, and over the rectangle of the tile plus halo they
// lie between their values at its four corners - the COMPUTED values, not only the exact ones.  Hence, with min / max over the corners:
// q2max <= 0 makes every pixel's q2 <= 0 (invalid); with q2min > 0, q0max < 0 and q0max / q2max < 0 every pixel's u = q0 / q2 is at most that
// (correctly rounded division is monotone too) and so < 0; q0min / q2max > w - 1 bounds every u from below, past the right edge; rows
// likewise.  In each case every pixel of the tile would have stored NaN, every window sum would be NaN and the source would not count for
// any pixel: skipping the (tile, plane, source) changes no bit.  The decision is made from wave-uniform values only, so the barriers stay
// uniform.  flags bit 0 switches the skip off (tests).
#pragma once
#include "nr_platform.h"

#include <math.h>

namespace nr {

constexpr int kSweepTile = 16, kSweepThreads = kSweepTile * kSweepTile;
constexpr int kSweepMaxSrc = 16, kSweepMaxPlanes = 256, kSweepMaxRadius = 3;
constexpr float kSweepCostNone = 4.0f, kSweepCurvMin = 1e-2f;

struct SweepParams {
    const float* rgb;          // [n][3][h][w] in [0,1]
    float* gray;               // [n][h][w]: workspace, gray - 0.5 of every view
    const float* cams;         // [n][S][12]: M (row-major) and b of every (view, slot)
    const float* range;        // [n][2] near, far
    const int* nn_ids;         // [n][S] source views; -1 or the view itself: an unused slot
    float* depth;              // [v1 - v0][h][w], 0 = none
    float* cost;               // [v1 - v0][h][w], kSweepCostNone = none
    int* plane;                // [v1 - v0][h][w], -1 = none
    int n, h, w, S, D, v0, v1, min_src, flags;
    float var_min;
};

__global__ void __launch_bounds__(256) sweep_gray_kernel(SweepParams p) {
    const size_t plane = (size_t)p.h * p.w, total = plane * (size_t)p.n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t v = i / plane, pix = i - v * plane;
        const float* __restrict__ c = p.rgb + v * 3 * plane + pix;
        p.gray[i] = ((0.299f * c[0] + 0.587f * c[plane]) + 0.114f * c[2 * plane]) - 0.5f;
    }
}

__device__ __forceinline__ float sweep_plane_depth(float t, float inv_near, float inv_far) {
    return 1.0f / ((1.0f - t) * inv_near + t * inv_far);
}

__device__ __forceinline__ void sweep_project(const float* __restrict__ cam, float d, float fx, float fy, float& q0, float& q1, float& q2) {
    q0 = d * ((cam[0] * fx + cam[1] * fy) + cam[2]) + cam[9];
    q1 = d * ((cam[3] * fx + cam[4] * fy) + cam[5]) + cam[10];
    q2 = d * ((cam[6] * fx + cam[7] * fy) + cam[8]) + cam[11];
}

// true: no pixel of the rectangle [xa, xb] x [ya, yb] has a valid warp (the header's argument)
__device__ __forceinline__ bool sweep_tile_outside(const float* __restrict__ cam, float d, float xa, float ya, float xb, float yb, float wm1,
                                                   float hm1) {
    float a0, a1, a2, b0, b1, b2, c0, c1, c2, e0, e1, e2;
    sweep_project(cam, d, xa, ya, a0, a1, a2);
    sweep_project(cam, d, xb, ya, b0, b1, b2);
    sweep_project(cam, d, xa, yb, c0, c1, c2);
    sweep_project(cam, d, xb, yb, e0, e1, e2);
    const float q2max = fmaxf(fmaxf(a2, b2), fmaxf(c2, e2)), q2min = fminf(fminf(a2, b2), fminf(c2, e2));
    if (q2max <= 0.0f) return true;
    if (!(q2min > 0.0f)) return false;
    const float q0max = fmaxf(fmaxf(a0, b0), fmaxf(c0, e0)), q0min = fminf(fminf(a0, b0), fminf(c0, e0));
    const float q1max = fmaxf(fmaxf(a1, b1), fmaxf(c1, e1)), q1min = fminf(fminf(a1, b1), fminf(c1, e1));
    if (q0max < 0.0f && q0max / q2max < 0.0f) return true;
    if (q1max < 0.0f && q1max / q2max < 0.0f) return true;
    if (q0min > 0.0f && q0min / q2max > wm1) return true;
    if (q1min > 0.0f && q1min / q2max > hm1) return true;
    return false;
}

// R: window radius; KEEP: the smallest per-source costs kept per plane (>= ceil(S / 2))
template <int R, int KEEP>
__global__ void __launch_bounds__(kSweepThreads) plane_sweep_kernel(SweepParams p) {
    constexpr int TS = kSweepTile, LW = TS + 2 * R, LN = LW * LW, RN = LW * TS;
    __shared__ float ref[LN];              // the reference gray of the tile plus halo, NaN outside the image
    __shared__ float src[LN];              // the warped source gray, NaN where there is none
    __shared__ float rows[3 * RN];         // row sums [3][LW rows][TS window columns]
    const int tid = (int)threadIdx.x, tx = tid % TS, ty = tid / TS;
    const int view = p.v0 + (int)blockIdx.z;
    const int x0t = (int)blockIdx.x * TS, y0t = (int)blockIdx.y * TS;
    const int x = x0t + tx, y = y0t + ty;
    const int h = p.h, w = p.w, S = p.S, D = p.D;
    const bool inside = x < w && y < h;    // partial tiles: the lane's window holds a NaN, it stores nothing
    const size_t plane = (size_t)h * w;
    const float wm1 = (float)(w - 1), hm1 = (float)(h - 1);
    const float inv_n = 1.0f / (float)((2 * R + 1) * (2 * R + 1));
    const float var_min = p.var_min;

    const float* __restrict__ gray_i = p.gray + (size_t)view * plane;
    for (int i = tid; i < LN; i += kSweepThreads) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = x0t + lx - R, gy = y0t + ly - R;
        ref[i] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? gray_i[(size_t)gy * w + gx] : NAN;
    }
    __syncthreads();
    for (int i = tid; i < RN; i += kSweepThreads) {
        const int ly = i / TS, ox = i - ly * TS;
        const float* __restrict__ a = ref + ly * LW + ox;
        float s1 = a[0], s2 = a[0] * a[0];
        NR_PRAGMA_UNROLL
        for (int d = 1; d <= 2 * R; ++d) { s1 = s1 + a[d]; s2 = s2 + a[d] * a[d]; }
        rows[i] = s1; rows[RN + i] = s2;
    }
    __syncthreads();
    float m_r, v_r;
    {
        const float* __restrict__ c = rows + ty * TS + tx;
        float s1 = c[0], s2 = c[RN];
        NR_PRAGMA_UNROLL
        for (int d = 1; d <= 2 * R; ++d) { s1 = s1 + c[d * TS]; s2 = s2 + c[RN + d * TS]; }
        m_r = s1 * inv_n;
        v_r = s2 * inv_n - m_r * m_r;
    }
    // (no barrier: the first row stage below comes after the first warp stage's barrier)

    int n_used = 0;
    for (int s = 0; s < S; ++s) {
        const int j = p.nn_ids[view * S + s];
        n_used += (j >= 0 && j < p.n && j != view) ? 1 : 0;
    }
    const int need = p.min_src > 0 ? p.min_src : (n_used == 1 ? 1 : 2);
    const float inv_near = 1.0f / p.range[view * 2], inv_far = 1.0f / p.range[view * 2 + 1];
    const float xa = (float)(x0t - R), ya = (float)(y0t - R), xb = (float)(x0t + TS - 1 + R), yb = (float)(y0t + TS - 1 + R);
    const bool skip_on = (p.flags & 1) == 0;

    float best = INFINITY, c_prev = NAN, c_next = NAN, c_last = NAN;
    int best_k = -1;
    for (int k = 0; k < D; ++k) {
        const float d = sweep_plane_depth((float)k / (float)(D - 1), inv_near, inv_far);
        float keep[KEEP];
        NR_PRAGMA_UNROLL
        for (int q = 0; q < KEEP; ++q) keep[q] = INFINITY;
        int m = 0;
        for (int s = 0; s < S; ++s) {
            const int j = p.nn_ids[view * S + s];
            if (!(j >= 0 && j < p.n && j != view)) continue;                    // (uniform)
            const float* __restrict__ cam = p.cams + (size_t)(view * S + s) * 12;
            if (skip_on && sweep_tile_outside(cam, d, xa, ya, xb, yb, wm1, hm1)) continue;      // (uniform: the header's argument)
            const float* __restrict__ gray_j = p.gray + (size_t)j * plane;
            for (int i = tid; i < LN; i += kSweepThreads) {
                const int ly = i / LW, lx = i - ly * LW;
                const int gx = x0t + lx - R, gy = y0t + ly - R;
                float val = NAN;
                if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                    float q0, q1, q2;
                    sweep_project(cam, d, (float)gx, (float)gy, q0, q1, q2);
                    const float u = q0 / q2, v = q1 / q2;
                    if (q2 > 0.0f && u >= 0.0f && u <= wm1 && v >= 0.0f && v <= hm1) {          // (false for a NaN)
                        const float xf = fminf(floorf(u), (float)(w - 2)), yf = fminf(floorf(v), (float)(h - 2));
                        const float ax = u - xf, ay = v - yf;
                        const float* __restrict__ g = gray_j + (size_t)(int)yf * w + (int)xf;
                        const float g00 = g[0], g01 = g[1], g10 = g[w], g11 = g[w + 1];
                        const float top = g00 + ax * (g01 - g00), bot = g10 + ax * (g11 - g10);
                        val = top + ay * (bot - top);
                    }
                }
                src[i] = val;
            }
            __syncthreads();
            for (int i = tid; i < RN; i += kSweepThreads) {
                const int ly = i / TS, ox = i - ly * TS;
                const float* __restrict__ a = ref + ly * LW + ox;
                const float* __restrict__ b = src + ly * LW + ox;
                float s1 = b[0], s2 = b[0] * b[0], s3 = a[0] * b[0];
                NR_PRAGMA_UNROLL
                for (int q = 1; q <= 2 * R; ++q) { s1 = s1 + b[q]; s2 = s2 + b[q] * b[q]; s3 = s3 + a[q] * b[q]; }
                rows[i] = s1; rows[RN + i] = s2; rows[2 * RN + i] = s3;
            }
            __syncthreads();
            const float* __restrict__ c = rows + ty * TS + tx;
            float s1 = c[0], s2 = c[RN], s3 = c[2 * RN];
            NR_PRAGMA_UNROLL
            for (int q = 1; q <= 2 * R; ++q) { s1 = s1 + c[q * TS]; s2 = s2 + c[RN + q * TS]; s3 = s3 + c[2 * RN + q * TS]; }
            const float m_s = s1 * inv_n;
            const float v_s = s2 * inv_n - m_s * m_s;
            const float cov = s3 * inv_n - m_r * m_s;
            float cc = fminf(fmaxf(1.0f - cov / sqrtf(v_r * v_s), 0.0f), 2.0f);
            const bool valid = v_r >= var_min && v_s >= var_min;                    // (false for a NaN: a window with a hole)
            cc = valid ? cc : INFINITY;
            m += valid ? 1 : 0;
            NR_PRAGMA_UNROLL
            for (int q = 0; q < KEEP; ++q) {       // insertion into the ascending list of the KEEP smallest
                const bool lt = cc < keep[q];
                const float lo = lt ? cc : keep[q], hi = lt ? keep[q] : cc;
                keep[q] = lo; cc = hi;
            }
        }
        const int kk = (m + 1) / 2;
        float acc = keep[0];
        NR_PRAGMA_UNROLL
        for (int q = 1; q < KEEP; ++q) acc = q < kk ? acc + keep[q] : acc;
        const float agg = (m >= need && m > 0) ? acc / (float)kk : NAN;
        if (best_k == k - 1 && best_k >= 0) c_next = agg;
        if (agg < best) { best = agg; best_k = k; c_prev = c_last; c_next = NAN; }
        c_last = agg;
    }
    if (!inside) return;
    const size_t o = (size_t)(view - p.v0) * plane + (size_t)y * w + x;
    float depth = 0.0f, cost = kSweepCostNone;
    if (best_k >= 0) {
        const float curv = (c_prev - best) + (c_next - best);
        float off = 0.0f;
        if (curv > kSweepCurvMin) off = fminf(fmaxf(0.5f * (c_prev - c_next) / curv, -0.5f), 0.5f);    // (false for a NaN: a missing neighbour)
        depth = sweep_plane_depth(((float)best_k + off) / (float)(D - 1), inv_near, inv_far);
        cost = best;
    }
    p.depth[o] = depth; p.cost[o] = cost; p.plane[o] = best_k;
}

}  // namespace nr
