// Depth-noise and ray-sampling augmentation of the procedural stream (neuray_amd/procedural.py augment_numpy): the
// data-dependent steps of the reference's GeneralRendererDataset.__getitem__ for a `gso` scene, on depth maps and masks that never leave
// the device.  Three entries (include/neuray_hip.h): neuray_augment_stats, neuray_augment_depth, neuray_sample_coords.
//
// Everything that is reduced is an integer: counts are sums, the bounding box and the depth extrema are min / max (a valid depth is a
// positive float, whose bit pattern orders like the value), the ray selection is a radix select on integer keys.  No float atomics, no
// atomicMin / atomicMax: block reductions go through shuffles and LDS, the digit histograms through integer atomicAdd.  The float
// arithmetic is augment_numpy's, operation by operation, in fp32 without contraction (no fmaf anywhere in this file).
//
// Random numbers: Philox4x32-10, key = (stream seed, batch index), counter = (pixel y * w + x, view, purpose, 0); purposes 0 / 1: the
// local noise of the large / small offset region, 2: the global noise, 3: the ray selection (words 0 and 1: the keys of its two stages).
#pragma once
#include "nr_platform.h"

#include <math.h>
#include <stdint.h>

namespace nr {

constexpr int kAugBlock = 256;                 // every kernel here but the plan kernel: 4 waves
constexpr int kAugHost = 16;                   // floats of the host array's head, and of every working view after it
constexpr int kAugStats = 8;                   // ints per view: count, xmin, xmax, ymin, ymax, bits of min depth, bits of max depth, 0
constexpr int kAugPlan = 8;                    // floats per region: on, cx, cy, lx, ly, global offset, local amplitude, depth length
constexpr int kSampleBins = 2048;              // digits of 11, 11 and 10 bits of the 32-bit key
constexpr int kSamplePasses = 3;
constexpr int kSampleMaxBlocks = 1024;
constexpr int kSampleState = 16;
// the workspace in 64-bit words: histograms [2][3][2048], state [2][16], per-block counts [2][1024][2]
constexpr int kSampleHistWords = 2 * kSamplePasses * kSampleBins;
constexpr int kSampleStateAt = kSampleHistWords;
constexpr int kSampleBlocksAt = kSampleStateAt + 2 * kSampleState;
constexpr int kSampleWorkWords = kSampleBlocksAt + 2 * kSampleMaxBlocks * 2;

struct Philox4 { unsigned x, y, z, w; };

__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}

__device__ __forceinline__ float aug_unit(unsigned word) { return (float)(word >> 8) * 5.9604644775390625e-08f; }       // [0, 1), 24 bits
__device__ __forceinline__ float aug_symmetric(unsigned word, float a, float L) { return ((2.0f * aug_unit(word) - 1.0f) * a) * L; }
__device__ __forceinline__ float aug_uniform(float lo, float hi, float u) { return lo + (hi - lo) * u; }
__device__ __forceinline__ int aug_imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int aug_imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int aug_popc(unsigned long long b) { return __builtin_popcountll(b); }
__device__ __forceinline__ unsigned long long aug_below(int lane) { return (1ull << lane) - 1ull; }

enum { AUG_SUM = 0, AUG_MIN = 1, AUG_MAX = 2 };
template <int OP> __device__ __forceinline__ int aug_combine(int a, int b) { return OP == AUG_SUM ? a + b : (OP == AUG_MIN ? aug_imin(a, b) : aug_imax(a, b)); }

// reduction over the 256 threads of a workgroup, the result in every thread (red: 4 ints of LDS)
template <int OP> __device__ __forceinline__ int aug_block_reduce(int v, int* red, int tid) {
    for (int m = 32; m >= 1; m >>= 1) v = aug_combine<OP>(v, __shfl_xor(v, m));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return aug_combine<OP>(aug_combine<OP>(red[0], red[1]), aug_combine<OP>(red[2], red[3]));
}

// ---- 1. statistics of every view over mask > 0 ------------------------------------------------------------------------------------
struct AugStatsParams {
    const unsigned char* mask;     // [n][h][w]
    const float* depth;            // [n][h][w]
    int* row_counts;               // [n][h] foreground pixels of every row
    int* row_part;                 // [n][h][4] workspace: xmin, xmax, bits of min / max valid depth of the row
    int* stats;                    // [n][kAugStats]
    int n, h, w;
};

constexpr int kAugNoMin = 0x7f800000, kAugNoMax = -1;       // bits of +inf; below every bit pattern of a valid depth

// one workgroup per (row, view)
__global__ void __launch_bounds__(kAugBlock) augment_row_stats_kernel(AugStatsParams p) {
    __shared__ int red[4];
    const int y = (int)blockIdx.x, v = (int)blockIdx.y, tid = (int)threadIdx.x, w = p.w;
    const size_t row = ((size_t)v * p.h + y) * w;
    int cnt = 0, xmin = w, xmax = -1, dmin = kAugNoMin, dmax = kAugNoMax;
    for (int x = tid; x < w; x += kAugBlock) {
        if (p.mask[row + x] > 0) {
            cnt = cnt + 1; xmin = aug_imin(xmin, x); xmax = aug_imax(xmax, x);
            const float d = p.depth[row + x];
            if (d > 1e-3f && d < 1e4f) { const int b = __float_as_int(d); dmin = aug_imin(dmin, b); dmax = aug_imax(dmax, b); }
        }
    }
    cnt = aug_block_reduce<AUG_SUM>(cnt, red, tid);
    xmin = aug_block_reduce<AUG_MIN>(xmin, red, tid);
    xmax = aug_block_reduce<AUG_MAX>(xmax, red, tid);
    dmin = aug_block_reduce<AUG_MIN>(dmin, red, tid);
    dmax = aug_block_reduce<AUG_MAX>(dmax, red, tid);
    if (tid == 0) {
        const size_t r = (size_t)v * p.h + y;
        p.row_counts[r] = cnt;
        p.row_part[r * 4] = xmin; p.row_part[r * 4 + 1] = xmax; p.row_part[r * 4 + 2] = dmin; p.row_part[r * 4 + 3] = dmax;
    }
}

// one workgroup per view: the rows' partial results -> stats.  An empty mask: count 0, xmin = w, xmax = -1, ymin = h, ymax = -1; no valid
// depth: min = +inf, max = -inf.
__global__ void __launch_bounds__(kAugBlock) augment_view_stats_kernel(AugStatsParams p) {
    __shared__ int red[4];
    const int v = (int)blockIdx.x, tid = (int)threadIdx.x, h = p.h;
    int cnt = 0, xmin = p.w, xmax = -1, ymin = h, ymax = -1, dmin = kAugNoMin, dmax = kAugNoMax;
    for (int y = tid; y < h; y += kAugBlock) {
        const size_t r = (size_t)v * h + y;
        const int c = p.row_counts[r];
        if (c > 0) {
            cnt = cnt + c; ymin = aug_imin(ymin, y); ymax = aug_imax(ymax, y);
            xmin = aug_imin(xmin, p.row_part[r * 4]); xmax = aug_imax(xmax, p.row_part[r * 4 + 1]);
            dmin = aug_imin(dmin, p.row_part[r * 4 + 2]); dmax = aug_imax(dmax, p.row_part[r * 4 + 3]);
        }
    }
    cnt = aug_block_reduce<AUG_SUM>(cnt, red, tid);
    xmin = aug_block_reduce<AUG_MIN>(xmin, red, tid);
    xmax = aug_block_reduce<AUG_MAX>(xmax, red, tid);
    ymin = aug_block_reduce<AUG_MIN>(ymin, red, tid);
    ymax = aug_block_reduce<AUG_MAX>(ymax, red, tid);
    dmin = aug_block_reduce<AUG_MIN>(dmin, red, tid);
    dmax = aug_block_reduce<AUG_MAX>(dmax, red, tid);
    if (tid == 0) {
        int* s = p.stats + (size_t)v * kAugStats;
        s[0] = cnt; s[1] = xmin; s[2] = xmax; s[3] = ymin; s[4] = ymax;
        s[5] = dmin; s[6] = dmax == kAugNoMax ? (int)0xff800000u : dmax; s[7] = 0;
    }
}

// ---- 2. depth ranges, the plan of the offset regions, the noisy depth maps ------------------------------------------------------------
// host [kAugHost + rfn * kAugHost] floats, numbers that do not depend on device data:
//   head: 0 shrink on | 1 u far | 2 u near | 3 widen on | 4 u ratio0 | 5 u ratio1 | 6 consistent range on | 7 zero
//         8..12 the large region: region min, region max, offset min, offset max, local amplitude | 13..15 zero
//   working view r: 0..5 the large region: on, u centre, u lx, u ly, u offset, negative | 6..11 the small region | 12 global noise on | 13..15 zero
struct AugDepthParams {
    const float* depth;            // [n][h][w] the exact maps
    const unsigned char* mask;     // [n][h][w]
    const float* range_in;         // [n][2] near, far
    const int* stats;              // [n][kAugStats]
    const int* row_counts;         // [n][h]
    const float* host;
    float* range_aug;              // [n][2] after the range augmentation
    float* range_out;              // [n][2] after consistent_depth_range
    float* plan;                   // [rfn][2][kAugPlan]
    float* depth_aug;              // [rfn][h][w]
    int n, h, w, view0, rfn;       // the working views are [view0, view0 + rfn) of the n views
    unsigned key0, key1;
};

struct AugRangeOps { bool far_on, near_on, widen; float far_f, near_f, r0, r1; };

__device__ __forceinline__ void aug_range_of(const AugRangeOps& o, const float* __restrict__ range_in, int v, float& near, float& far) {
    near = range_in[2 * v]; far = range_in[2 * v + 1];
    if (o.far_on) far = far * o.far_f;
    if (o.near_on) near = near / o.near_f;
    if (o.widen) { near = near * (1.0f - o.r0); far = far * (1.0f + o.r1); }
}

// the pixel of row-major rank `rank` among the foreground pixels of a view, by one wave: the row through the row counts (a scan per 64
// rows), the column through one scan of that row.  The trip counts are the same in every lane.
__device__ __forceinline__ void aug_pixel_of_rank(const int* __restrict__ rows, const unsigned char* __restrict__ mask, int h, int w, int rank,
                                                  int lane, int& cx, int& cy) {
    int rem = rank, fy = -1;
    cx = 0; cy = 0;
    for (int base = 0; base < h; base += 64) {
        const int y = base + lane;
        const int c = y < h ? rows[y] : 0;
        int s = c;
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(s, d); if (lane >= d) s = s + t; }
        const int total = __shfl(s, 63);
        if (rem < total) {
            const int first = __builtin_ctzll(__ballot(s > rem));
            rem = rem - __shfl(s - c, first);
            fy = base + first;
            break;
        }
        rem = rem - total;
    }
    if (fy < 0) return;                                      // (a rank beyond the counts: they do not belong to this mask)
    cy = fy;
    for (int base = 0; base < w; base += 64) {
        const int x = base + lane;
        const bool on = x < w && mask[(size_t)fy * w + x] > 0;
        const unsigned long long b = __ballot(on);
        const int total = aug_popc(b);
        if (rem < total) {
            const unsigned long long hit = __ballot(on && aug_popc(b & aug_below(lane)) == rem);
            cx = base + __builtin_ctzll(hit);
            break;
        }
        rem = rem - total;
    }
}

// One wave per working view (at least one workgroup: it also writes the ranges).  Every lane evaluates the range arithmetic - a loop over
// the views at uniform addresses -, so there is nothing to reduce.
__global__ void __launch_bounds__(64) augment_plan_kernel(AugDepthParams p) {
    const int r = (int)blockIdx.x, lane = (int)threadIdx.x, n = p.n;
    const float* __restrict__ H = p.host;
    AugRangeOps o;
    o.far_on = false; o.near_on = false; o.far_f = 1.0f; o.near_f = 1.0f;
    if (H[0] != 0.0f) {
        bool any = false;
        float far_ratio = 0.0f, near_ratio = 0.0f;
        for (int v = 0; v < n; ++v) {
            const float dmin = __int_as_float(p.stats[v * kAugStats + 5]), dmax = __int_as_float(p.stats[v * kAugStats + 6]);
            if (!(dmin < INFINITY)) continue;                // an empty mask, or no valid depth in it: the view takes no part
            const float fr = (dmax * 1.1f) / p.range_in[2 * v + 1], nr_ = p.range_in[2 * v] / (dmin * 0.9f);
            far_ratio = any ? fmaxf(far_ratio, fr) : fr;
            near_ratio = any ? fmaxf(near_ratio, nr_) : nr_;
            any = true;
        }
        if (any && far_ratio < 1.0f) { o.far_on = true; o.far_f = aug_uniform(far_ratio, 1.0f, H[1]); }
        if (any && near_ratio < 1.0f) { o.near_on = true; o.near_f = aug_uniform(near_ratio, 1.0f, H[2]); }
    }
    o.widen = H[3] != 0.0f;
    o.r0 = aug_uniform(0.025f, 0.1f, H[4]); o.r1 = aug_uniform(0.025f, 0.1f, H[5]);
    if (r == 0) {
        float max_len = 0.0f;
        for (int v = 0; v < n; ++v) {
            float near, far;
            aug_range_of(o, p.range_in, v, near, far);
            max_len = v == 0 ? far - near : fmaxf(max_len, far - near);
        }
        for (int v = lane; v < n; v += 64) {
            float near, far;
            aug_range_of(o, p.range_in, v, near, far);
            p.range_aug[2 * v] = near; p.range_aug[2 * v + 1] = far;
            if (H[6] != 0.0f) {
                const float margin = (max_len - (far - near)) / 2.0f;
                const float ref_near = fmaxf(near - margin, near * 0.5f);
                near = ref_near; far = ref_near + max_len;
            }
            p.range_out[2 * v] = near; p.range_out[2 * v + 1] = far;
        }
    }
    if (r >= p.rfn) return;
    const int v = p.view0 + r;
    float near, far;
    aug_range_of(o, p.range_in, v, near, far);
    const float L = far - near;
    const int* __restrict__ S = p.stats + (size_t)v * kAugStats;
    const int count = S[0];
    const float* __restrict__ Hr = H + kAugHost + r * kAugHost;
    for (int k = 0; k < 2; ++k) {
        const float* __restrict__ R = Hr + 6 * k;
        float* __restrict__ P = p.plan + ((size_t)r * 2 + k) * kAugPlan;
        const bool on = R[0] != 0.0f && count > 0;          // (uniform)
        int cx = 0, cy = 0;
        float lx = 0.0f, ly = 0.0f, off = 0.0f, amp = 0.0f;
        if (on) {
            const int rank = aug_imin((int)(R[1] * (float)count), count - 1);
            aug_pixel_of_rank(p.row_counts + (size_t)v * p.h, p.mask + (size_t)v * p.h * p.w, p.h, p.w, rank, lane, cx, cy);
            const float rmin = k == 0 ? H[8] : 0.1f, rmax = k == 0 ? H[9] : 0.2f, omin = k == 0 ? H[10] : 0.01f, omax = k == 0 ? H[11] : 0.05f;
            amp = k == 0 ? H[12] : 0.005f;
            lx = aug_uniform(rmin, rmax, R[2]) * (float)(S[2] - S[1]);
            ly = aug_uniform(rmin, rmax, R[3]) * (float)(S[4] - S[3]);
            off = aug_uniform(omin, omax, R[4]) * L;
            if (R[5] != 0.0f) off = -off;
        }
        if (lane == 0) {
            P[0] = on ? 1.0f : 0.0f; P[1] = (float)cx; P[2] = (float)cy; P[3] = lx; P[4] = ly; P[5] = off; P[6] = amp; P[7] = L;
        }
    }
}

// one thread per pixel of a working view: depth + the offsets of the regions it lies in + the global noise
__global__ void __launch_bounds__(kAugBlock) augment_apply_kernel(AugDepthParams p) {
    const int r = (int)blockIdx.y, v = p.view0 + r, w = p.w;
    const long long plane = (long long)p.h * w;
    const long long pix = (long long)blockIdx.x * kAugBlock + (int)threadIdx.x;
    if (pix >= plane) return;
    const int y = (int)(pix / w), x = (int)(pix - (long long)y * w);
    const float* __restrict__ P = p.plan + (size_t)r * 2 * kAugPlan;
    const float L = P[7];
    float d = p.depth[(size_t)v * plane + pix];
    const bool fg = p.mask[(size_t)v * plane + pix] > 0;
    for (int k = 0; k < 2; ++k) {
        const float* __restrict__ Q = P + k * kAugPlan;
        if (Q[0] != 0.0f && fg && fabsf((float)x - Q[1]) < Q[3] && fabsf((float)y - Q[2]) < Q[4]) {
            const Philox4 z = philox4x32_10((unsigned)pix, (unsigned)v, (unsigned)k, 0u, p.key0, p.key1);
            d = d + (aug_symmetric(z.x, Q[6], L) + Q[5]);
        }
    }
    if (p.host[kAugHost + r * kAugHost + 12] != 0.0f) {
        const Philox4 z = philox4x32_10((unsigned)pix, (unsigned)v, 2u, 0u, p.key0, p.key1);
        d = d + aug_symmetric(z.x, 0.005f, L);
    }
    p.depth_aug[(size_t)r * plane + pix] = d;
}

// ---- 3. ray coordinates: the k smallest of independent random keys, twice ---------------------------------------------------------------
// Pixel p carries the composites (word0 << 32) | p and (word1 << 32) | p of its purpose-3 Philox block: unique, so "the k smallest" is a
// set.  Stage 0 takes k = min(want_fg, foreground) foreground pixels by word0, stage 1 the ray_num - k smallest by word1 among every pixel
// stage 0 left.  A stage is a radix select on the word: three histogram passes (11, 11, 10 bits; per-workgroup LDS histograms flushed
// with integer atomicAdd, only the elements that match the digits found so far take part) give the word T of the k-th element and how
// many elements with that word belong to the k smallest - those with the lowest pixel index, the composite's low half.  The ordered
// compaction then walks the pixels in row-major order: selected = word < T, or word == T and fewer than `need` such pixels before it.
// A launch reads only what earlier launches wrote; every workgroup re-derives the digit from the finished histogram.
//   state [stage][16]: 0 k | 1, 2 digits found and k left after pass 0 | 3, 4 after pass 1 | 5 T | 6 need
struct SampleParams {
    const unsigned char* mask;     // [N] the query view's mask
    unsigned* keys;                // [2][N] word0, word1
    unsigned char* taken;          // [N] picked by stage 0
    unsigned long long* work;      // [kSampleWorkWords]
    float* coords;                 // [ray_num][2] x, y
    int N, w, chunk, nblocks, ray_num, want_fg, view, stage, pass;
    unsigned key0, key1;
};

__global__ void __launch_bounds__(kAugBlock) sample_keys_kernel(SampleParams p) {
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    for (int i = b * kAugBlock + tid; i < kSampleWorkWords; i += p.nblocks * kAugBlock) p.work[i] = 0ull;
    const int start = b * p.chunk, end = aug_imin(p.N - start, p.chunk) + start;
    for (int q = start + tid; q < end; q += kAugBlock) {
        const Philox4 z = philox4x32_10((unsigned)q, (unsigned)p.view, 3u, 0u, p.key0, p.key1);
        p.keys[q] = z.x; p.keys[(size_t)p.N + q] = z.y;
    }
}

// The bin in which the cumulative count of a finished histogram reaches k (1 <= k <= total) -> digit, before = the count of the bins
// below it.  k < 0: k = min(want, total) first.  All 256 threads call it; lds: 8 ints.
__device__ __forceinline__ void sample_find(const unsigned long long* __restrict__ hist, int k_in, int want, int tid, int* lds, int& k,
                                            int& digit, int& before) {
    int c[8], s = 0;
    NR_PRAGMA_UNROLL
    for (int j = 0; j < 8; ++j) { c[j] = (int)hist[8 * tid + j]; s = s + c[j]; }
    const int lane = tid & 63, wv = tid >> 6;
    int inc = s;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc = inc + t; }
    __syncthreads();
    if (lane == 63) lds[wv] = inc;
    if (tid == 0) { lds[4] = 0; lds[5] = 0; }
    __syncthreads();
    int wbase = 0;
    for (int i = 0; i < 4; ++i) wbase = wbase + (i < wv ? lds[i] : 0);
    const int total = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    k = k_in < 0 ? aug_imin(want, total) : k_in;
    int run = wbase + inc - s;
    if (k >= 1 && run < k && k <= run + s) {
        bool found = false;
        NR_PRAGMA_UNROLL
        for (int j = 0; j < 8; ++j) {
            if (!found && k <= run + c[j]) { lds[4] = 8 * tid + j; lds[5] = run; found = true; }
            run = run + c[j];
        }
    }
    __syncthreads();
    digit = lds[4]; before = lds[5];
}

__device__ __forceinline__ bool sample_eligible(const SampleParams& p, int q) { return p.stage == 0 ? p.mask[q] > 0 : p.taken[q] == 0; }
__device__ __forceinline__ int sample_want(const SampleParams& p, const unsigned long long* state0) {
    return p.stage == 0 ? p.want_fg : p.ray_num - (int)state0[0];
}

// histogram pass `pass` of stage `stage` (after the digit of the pass before it)
__global__ void __launch_bounds__(kAugBlock) sample_hist_kernel(SampleParams p) {
    __shared__ unsigned long long bins[kSampleBins];
    __shared__ int lds[8];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x, pass = p.pass;
    unsigned long long* state = p.work + kSampleStateAt + p.stage * kSampleState;
    unsigned long long* hist = p.work + ((size_t)p.stage * kSamplePasses + pass) * kSampleBins;
    unsigned prefix = 0u;
    int k = 1;
    if (pass > 0) {
        int digit, before;
        const int k_in = pass == 1 ? -1 : (int)state[2];
        sample_find(hist - kSampleBins, k_in, sample_want(p, p.work + kSampleStateAt), tid, lds, k, digit, before);
        prefix = pass == 1 ? (unsigned)digit << 21 : ((unsigned)state[1] | ((unsigned)digit << 10));
        if (b == 0 && tid == 0) {
            if (pass == 1) state[0] = (unsigned long long)k;
            state[2 * pass - 1] = prefix; state[2 * pass] = (unsigned long long)(pass == 1 ? k - before : (int)state[2] - before);
        }
    }
    for (int i = tid; i < kSampleBins; i += kAugBlock) bins[i] = 0ull;
    __syncthreads();
    const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0), above = pass == 0 ? 32 : (pass == 1 ? 21 : 10);
    const unsigned dmask = pass == 2 ? 0x3ffu : 0x7ffu;
    const unsigned* __restrict__ keys = p.keys + (size_t)p.stage * p.N;
    const int start = b * p.chunk, end = aug_imin(p.N - start, p.chunk) + start;
    for (int q = start + tid; q < end; q += kAugBlock) {
        if (!sample_eligible(p, q)) continue;
        const unsigned word = keys[q];
        if (above < 32 && (word >> above) != (prefix >> above)) continue;
        atomicAdd(&bins[(word >> shift) & dmask], 1ull);
    }
    __syncthreads();
    for (int i = tid; i < kSampleBins; i += kAugBlock) { const unsigned long long c = bins[i]; if (c != 0ull) atomicAdd(&hist[i], c); }
}

// the last digit -> T and need (state 5, 6), and per workgroup the number of eligible pixels with word < T and with word == T
__global__ void __launch_bounds__(kAugBlock) sample_count_kernel(SampleParams p) {
    __shared__ int lds[8];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    unsigned long long* state = p.work + kSampleStateAt + p.stage * kSampleState;
    int k, digit, before;
    sample_find(p.work + ((size_t)p.stage * kSamplePasses + 2) * kSampleBins, (int)state[4], 0, tid, lds, k, digit, before);
    const unsigned T = (unsigned)state[3] | (unsigned)digit;
    const bool some = (int)state[0] > 0;
    if (b == 0 && tid == 0) { state[5] = T; state[6] = (unsigned long long)(some ? k - before : 0); }
    const unsigned* __restrict__ keys = p.keys + (size_t)p.stage * p.N;
    const int start = b * p.chunk, end = aug_imin(p.N - start, p.chunk) + start;
    int less = 0, eq = 0;
    for (int q = start + tid; q < end; q += kAugBlock) {
        if (!some || !sample_eligible(p, q)) continue;
        const unsigned word = keys[q];
        less = less + (word < T ? 1 : 0); eq = eq + (word == T ? 1 : 0);
    }
    less = aug_block_reduce<AUG_SUM>(less, lds, tid);
    eq = aug_block_reduce<AUG_SUM>(eq, lds, tid);
    if (tid == 0) {
        unsigned long long* bc = p.work + kSampleBlocksAt + ((size_t)p.stage * kSampleMaxBlocks + b) * 2;
        bc[0] = (unsigned long long)less; bc[1] = (unsigned long long)eq;
    }
}

// ordered compaction: the picks of the stage in row-major order, stage 1 behind stage 0's; stage 0 also marks every pixel taken or not
__global__ void __launch_bounds__(kAugBlock) sample_emit_kernel(SampleParams p) {
    __shared__ int lds[8];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long* state = p.work + kSampleStateAt + p.stage * kSampleState;
    const bool some = (int)state[0] > 0;
    const unsigned T = (unsigned)state[5];
    const int need = (int)state[6];
    const int out_base = p.stage == 0 ? 0 : (int)p.work[kSampleStateAt];
    const unsigned long long* bc = p.work + kSampleBlocksAt + (size_t)p.stage * kSampleMaxBlocks * 2;
    int base_less = 0, base_eq = 0;
    for (int i = tid; i < b; i += kAugBlock) { base_less = base_less + (int)bc[2 * i]; base_eq = base_eq + (int)bc[2 * i + 1]; }
    base_less = aug_block_reduce<AUG_SUM>(base_less, lds, tid);
    base_eq = aug_block_reduce<AUG_SUM>(base_eq, lds, tid);
    const unsigned* __restrict__ keys = p.keys + (size_t)p.stage * p.N;
    const int start = b * p.chunk, end = aug_imin(p.N - start, p.chunk) + start;
    for (int t0 = start; t0 < end; t0 += kAugBlock) {
        const int q = t0 + tid;
        const bool in = q < end;
        const bool el = in && some && sample_eligible(p, q);
        const unsigned word = in ? keys[q] : 0u;
        const bool less = el && word < T, eq = el && word == T;
        const unsigned long long bl = __ballot(less), be = __ballot(eq);
        __syncthreads();
        if (lane == 0) { lds[wv] = aug_popc(bl); lds[4 + wv] = aug_popc(be); }
        __syncthreads();
        int nl = base_less + aug_popc(bl & aug_below(lane)), ne = base_eq + aug_popc(be & aug_below(lane));
        for (int i = 0; i < 4; ++i) { nl = nl + (i < wv ? lds[i] : 0); ne = ne + (i < wv ? lds[4 + i] : 0); }
        const bool sel = less || (eq && ne < need);
        if (in) {
            if (p.stage == 0) p.taken[q] = sel ? 1 : 0;
            const int pos = out_base + nl + aug_imin(ne, need);
            if (sel && pos < p.ray_num) {
                const int y = q / p.w;
                p.coords[2 * (size_t)pos] = (float)(q - y * p.w); p.coords[2 * (size_t)pos + 1] = (float)y;
            }
        }
        base_less = base_less + (lds[0] + lds[1]) + (lds[2] + lds[3]);
        base_eq = base_eq + (lds[4] + lds[5]) + (lds[6] + lds[7]);
    }
}

}  // namespace nr
