// Training losses of the reference (network/loss.py: RenderLoss, ConsistencyLoss, DepthLoss), one *loss call* - every term one
// loss object produces in one __call__ - per launch.  A term reduces `rows` rows of `n` elements each to one fp32 value per row:
//   RENDER   loss.py:57-77   element = ray: l = sum_c (pr - gt)^2;  with a mask  sum(l * m) / (sum(m) + 1e-3), else  sum(l) / n.
//            A masked-out ray is multiplied by 0 as in the reference: a non-finite prediction under a zero mask still gives NaN.
//   CONSIST  loss.py:29-44   element = (ray, sample): ce = -p0 log(p1 + 1e-5) - (1 - p0) log(1 - p1 + 1e-5), mean over dn, then rn
//            (p0 is detached; the reference's use_ray_mask never reaches the value, so there is no mask here)
//   DEPTH    loss.py:91-132  element = point: depth_gt = bilinear read of the [rows][h][w] true_depth map at the point's coordinate as
//            interpolate_feats(padding_mode='border', align_corners=True) does it (x / (w - 1) * 2 - 1, grid_sample's un-normalisation,
//            clip to [0, w - 1], four taps), process() = clamp at 1e-5, -1 / d, (d - near) / (far - near), clamp to [0, 1];
//            l = (gt - pr)^2 or SmoothL1(beta);  gso scenes: the same read of the noisy map, m = |aug - gt| < thresh,
//            sum(l * m) / (sum(m) + 1e-4); else sum(l) / n.  Coordinates are fp32 or int64 pairs used as (x, y).
// Per-element arithmetic is fp32 in the reference's operation order (the library is built with -ffp-contract=off; logf is the
// accurate one).  Sums are fp64 in a fixed order, as in nr_kernels_metrics.h: a workgroup owns one chunk of kLossChunk elements of
// one (term, row), every thread adds its elements in index order, a fixed tree joins the threads, and the partial (numerator,
// mask count) goes to the slot of the block index.  loss_finish_kernel adds a row's slots in slot order.  No float atomics: a term's
// value is bitwise the same alone or next to other terms, and from run to run.
// loss_backward_kernel recomputes the element-wise derivative from the inputs; between the passes only the row denominators are kept.
#pragma once
#include "nr_platform.h"
#include "nr_device.h"

namespace nr {

constexpr int kLossMaxTerms = 4;                      // RenderLoss: nr, dr, dr_fine, nr_fine
constexpr int kLossThreads = 256;
constexpr int kLossChunk = 2048;                      // elements of one row per workgroup (8 per thread)
enum { LOSS_RENDER = 0, LOSS_CONSIST = 1, LOSS_DEPTH = 2 };

struct LossTerm {
    const float* pred;             // RENDER [rows][n][3]; CONSIST p1 [rows][n]; DEPTH depth_mean, element (row, i) at (row * n + i) * stride
    const float* ref;              // RENDER ground truth [rows][n][3]; CONSIST p0 [rows][n]; DEPTH true_depth [rows][h][w]
    const void* mask;              // RENDER ray mask [rows][n] (fp32, or bytes with mask_u8) or null; DEPTH noisy map [rows][h][w] or null
    const void* coords;            // DEPTH [rows][n][2], fp32 or int64
    const float* range;            // DEPTH [rows][2]: near, far depth
    const float* g_up;             // backward: upstream gradient [rows]
    float* d_pred;                 // backward: [rows][n][3] / [rows][n], contiguous
    int kind, rows, n, inner;      // inner: CONSIST dn (n = rn * dn)
    int stride, h, w, coords_i64, mask_u8, smooth_l1;
    float beta, thresh;
    int chunks, block0, row0;      // chunks per row; the term's first workgroup; its first row in the value / denominator arrays
};

struct LossParams {
    LossTerm t[kLossMaxTerms];
    int nterms, total_rows;
    double* ws;                    // [blocks][2]: numerator, mask count
    float* value;                  // [total_rows]
    double* den;                   // [total_rows]: the denominator num was divided by
};

// torch.clamp: NaN goes through
__device__ __forceinline__ float loss_clamp_min(float x, float lo) { return x < lo ? lo : x; }
__device__ __forceinline__ float loss_clamp_max(float x, float hi) { return x > hi ? hi : x; }

// loss.py:104-109 process()
__device__ __forceinline__ float loss_inv_depth(float d, float near, float far) {
    d = loss_clamp_min(d, 1e-5f);
    d = -1.0f / d;
    d = (d - near) / (far - near);
    return loss_clamp_max(loss_clamp_min(d, 0.0f), 1.0f);
}

__device__ __forceinline__ float loss_mask_at(const LossTerm& t, size_t i) {
    if (!t.mask) return 1.0f;
    return t.mask_u8 ? (static_cast<const unsigned char*>(t.mask)[i] ? 1.0f : 0.0f) : static_cast<const float*>(t.mask)[i];
}

struct DepthElem { float gt, m; };

// the gathered, processed ground truth of point i of `row` and its gso mask (1 without a noisy map)
__device__ __forceinline__ DepthElem loss_depth_elem(const LossTerm& t, int row, int i) {
    const size_t e = (size_t)row * t.n + i;
    float u, v;
    if (t.coords_i64) {
        const long long* c = static_cast<const long long*>(t.coords) + 2 * e;
        u = (float)c[0]; v = (float)c[1];
    } else {
        const float* c = static_cast<const float*>(t.coords) + 2 * e;
        u = c[0]; v = c[1];
    }
    const Taps tp = make_taps(u, v, t.w, t.h, t.w, t.h);           // (offsets are clamped into the map for every u, v, NaN included)
    const size_t plane = (size_t)row * t.h * t.w;
    const float near = -1.0f / t.range[2 * row], far = -1.0f / t.range[2 * row + 1];
    const float* pl = t.ref + plane;
    DepthElem o;
    o.gt = loss_inv_depth(blend4(pl[tp.o00], pl[tp.o10], pl[tp.o01], pl[tp.o11], tp), near, far);
    o.m = 1.0f;
    if (t.mask) {
        const float* pn = static_cast<const float*>(t.mask) + plane;
        const float aug = loss_inv_depth(blend4(pn[tp.o00], pn[tp.o10], pn[tp.o01], pn[tp.o11], tp), near, far);
        o.m = fabsf(aug - o.gt) < t.thresh ? 1.0f : 0.0f;
    }
    return o;
}

// workgroup -> (term, row, chunk); the table is workgroup-uniform
__device__ __forceinline__ int loss_locate(const LossParams& p, int block, int& row, int& chunk) {
    int k = 0;
    for (int j = 1; j < p.nterms; ++j) if (block >= p.t[j].block0) k = j;
    const int local = block - p.t[k].block0;
    row = local / p.t[k].chunks;
    chunk = local - row * p.t[k].chunks;
    return k;
}

__global__ void __launch_bounds__(kLossThreads) loss_partials_kernel(LossParams p) {
    NR_DYNAMIC_SMEM(double, red);                      // [2][kLossThreads]
    const int tid = (int)threadIdx.x;
    int row, chunk;
    const LossTerm& t = p.t[loss_locate(p, (int)blockIdx.x, row, chunk)];
    const int i1 = (chunk + 1) * kLossChunk < t.n ? (chunk + 1) * kLossChunk : t.n;
    double num = 0.0, cnt = 0.0;
    for (int i = chunk * kLossChunk + tid; i < i1; i += kLossThreads) {
        const size_t e = (size_t)row * t.n + i;
        if (t.kind == LOSS_RENDER) {
            const float* a = t.pred + 3 * e;
            const float* b = t.ref + 3 * e;
            const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
            const float l = d0 * d0 + d1 * d1 + d2 * d2;
            const float m = loss_mask_at(t, e);
            num += (double)(t.mask ? l * m : l);
            cnt += (double)m;
        } else if (t.kind == LOSS_CONSIST) {
            const float p0 = t.ref[e], p1 = t.pred[e];
            const float ce = -p0 * logf(p1 + 1e-5f) - (1.0f - p0) * logf(1.0f - p1 + 1e-5f);
            num += (double)ce;
        } else {
            const DepthElem g = loss_depth_elem(t, row, i);
            const float x = g.gt - t.pred[e * t.stride];
            float l;
            if (t.smooth_l1) {
                const float z = fabsf(x);
                l = z < t.beta ? 0.5f * z * z / t.beta : z - 0.5f * t.beta;
            } else {
                l = x * x;
            }
            num += (double)(t.mask ? l * g.m : l);
            cnt += (double)g.m;
        }
    }
    red[tid] = num; red[kLossThreads + tid] = cnt;
    for (int s = kLossThreads / 2; s > 0; s >>= 1) {      // fixed-order tree over the workgroup
        __syncthreads();
        if (tid < s) { red[tid] += red[tid + s]; red[kLossThreads + tid] += red[kLossThreads + tid + s]; }
    }
    if (tid == 0) { p.ws[2 * (size_t)blockIdx.x] = red[0]; p.ws[2 * (size_t)blockIdx.x + 1] = red[kLossThreads]; }
}

// one workgroup of 64 per (term, row): the row's slots in slot order (thread k: slots k, k + 64, ...), a fixed tree, num / den
__global__ void __launch_bounds__(64) loss_finish_kernel(LossParams p) {
    NR_DYNAMIC_SMEM(double, red);                      // [2][64]
    const int tid = (int)threadIdx.x;
    int k = 0;
    for (int j = 1; j < p.nterms; ++j) if ((int)blockIdx.x >= p.t[j].row0) k = j;
    const LossTerm& t = p.t[k];
    const int row = (int)blockIdx.x - t.row0;
    const double* w = p.ws + 2 * ((size_t)t.block0 + (size_t)row * t.chunks);
    double num = 0.0, cnt = 0.0;
    for (int c = tid; c < t.chunks; c += 64) { num += w[2 * c]; cnt += w[2 * c + 1]; }
    red[tid] = num; red[64 + tid] = cnt;
    for (int s = 32; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) { red[tid] += red[tid + s]; red[64 + tid] += red[64 + tid + s]; }
    }
    if (tid == 0) {
        // the reference's mask is float32 and so is its denominator, sum(mask) + eps (the count itself is exact in both)
        double den = (double)t.n;
        if (t.mask && t.kind == LOSS_RENDER) den = (double)((float)red[64] + 1e-3f);
        if (t.mask && t.kind == LOSS_DEPTH) den = (double)((float)red[64] + 1e-4f);
        p.value[blockIdx.x] = (float)(red[0] / den);
        p.den[blockIdx.x] = den;
    }
}

__global__ void __launch_bounds__(kLossThreads) loss_backward_kernel(LossParams p) {
    const int tid = (int)threadIdx.x;
    int row, chunk;
    const LossTerm& t = p.t[loss_locate(p, (int)blockIdx.x, row, chunk)];
    if (!t.d_pred) return;                             // (a term whose prediction needs no gradient)
    const int i1 = (chunk + 1) * kLossChunk < t.n ? (chunk + 1) * kLossChunk : t.n;
    const float g = t.g_up[row];
    // the row's scale as autograd forms it: g / (sum(mask) + eps) for the masked sums, g / n for torch.mean, (g / rn) / dn for the two means
    float s;
    if (t.kind == LOSS_CONSIST) s = g / (float)(t.n / t.inner) / (float)t.inner;
    else s = g / (float)p.den[t.row0 + row];
    for (int i = chunk * kLossChunk + tid; i < i1; i += kLossThreads) {
        const size_t e = (size_t)row * t.n + i;
        if (t.kind == LOSS_RENDER) {
            const float* a = t.pred + 3 * e;
            const float* b = t.ref + 3 * e;
            const float dl = t.mask ? s * loss_mask_at(t, e) : s;
            float* o = t.d_pred + 3 * e;
            o[0] = dl * (2.0f * (a[0] - b[0]));
            o[1] = dl * (2.0f * (a[1] - b[1]));
            o[2] = dl * (2.0f * (a[2] - b[2]));
        } else if (t.kind == LOSS_CONSIST) {
            const float p0 = t.ref[e], p1 = t.pred[e];
            t.d_pred[e] = (s * -p0) / (p1 + 1e-5f) + (s * (1.0f - p0)) / (1.0f - p1 + 1e-5f);
        } else {
            const DepthElem ge = loss_depth_elem(t, row, i);
            const float x = ge.gt - t.pred[e * t.stride];
            const float dl = t.mask ? s * ge.m : s;
            float dx;                                  // d l / d (gt - pr), times dl
            if (t.smooth_l1) {
                if (t.beta > 0.0f && fabsf(x) < t.beta) dx = x * dl / t.beta;
                else dx = x > 0.0f ? dl : (x < 0.0f ? -dl : x * dl);       // (NaN stays NaN)
            } else {
                dx = dl * (2.0f * x);
            }
            t.d_pred[e] = -dx;
        }
    }
}

}  // namespace nr
