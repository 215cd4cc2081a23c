// Direct rendering (cfg['use_dr_prediction'], network/renderer.py:85-125 + network/sph_solver.py:1-59): the second,
// network-free estimate of a ray's colour that the reference can emit next to the aggregation network's -
//   alpha_dr(point)  = sum_v vis_v alpha_v / (sum_v vis_v + 1e-5)           (alpha_v: the dist decoder's logit, -15 where masked)
//   colors_dr(point) = SH_16(que_dir) . theta,   theta = (A^T W A + diag(regs))^-1 A^T W C   (weighted degree-3 spherical
//                      harmonics fit of the views' colours C over their viewing directions, W = hit_v / (sum hit + 1e-3))
//   hit_prob_dr      = alpha_values2hit_prob(sigmoid(alpha_dr)),  pixel_colors_dr = sum_i hit_i colors_i.
// Off in every shipped config, so this is built for exactness, not for the roofline: one thread per sample point, the
// 16 x 16 normal matrix packed symmetric in registers (136 + 48 right-hand sides), an unrolled LDL^T elimination (the
// matrix is symmetric positive definite: sum w > 0 on the constant column, regs > 0 elsewhere) where the reference calls
// torch.inverse.  The per-(point, view) hit / vis come from the point kernel's per-view record (NeurayPointsArgs.dbg_dev,
// fields 4 / 5), geometry and colours are recomputed with the exact (reference-order) device functions.
#pragma once
#include "nr_device.h"
#ifndef NR_INFERENCE_ONLY
#include "nr_kernels_bwd2.h"         // b2_prob_bwd (the backward below)
#endif

namespace nr {

// real spherical-harmonics polynomials of sph_solver.py:14-31 up to degree 3, in the reference's operation order
__device__ __forceinline__ void sh16(float x, float y, float z, float (&a)[16]) {
    const float xx = rn_mul(x, x), yy = rn_mul(y, y), zz = rn_mul(z, z);
    a[0] = 1.0f;
    a[1] = x; a[2] = y; a[3] = z;
    a[4] = rn_mul(x, y);
    a[5] = rn_mul(y, z);
    a[6] = rn_add(rn_sub(-xx, yy), rn_mul(2.0f, zz));
    a[7] = rn_mul(z, x);
    a[8] = rn_sub(xx, yy);
    a[9] = rn_mul(rn_sub(rn_mul(3.0f, xx), yy), y);
    a[10] = rn_mul(rn_mul(x, y), z);
    a[11] = rn_mul(y, rn_sub(rn_sub(rn_mul(4.0f, zz), xx), yy));
    a[12] = rn_mul(z, rn_sub(rn_sub(rn_mul(2.0f, zz), rn_mul(3.0f, xx)), rn_mul(3.0f, yy)));
    a[13] = rn_mul(x, rn_sub(rn_sub(rn_mul(4.0f, zz), xx), yy));
    a[14] = rn_mul(rn_sub(xx, yy), z);
    a[15] = rn_mul(rn_sub(xx, rn_mul(3.0f, yy)), x);
}

__device__ __forceinline__ constexpr int sym(int i, int j) { return i <= j ? i * 16 - i * (i - 1) / 2 + (j - i) : j * 16 - j * (j - 1) / 2 + (i - j); }

// NC right-hand sides (the forward solves for the three colour columns; the backward adds the query basis as a fourth column)
template <int K, int NC>
__device__ __forceinline__ void dr_eliminate(float (&M)[136], float (&R)[16][NC]) {
    if constexpr (K < 16) {
        const float inv = 1.0f / M[sym(K, K)];
        NR_PRAGMA_UNROLL
        for (int i = K + 1; i < 16; ++i) {
            const float f = M[sym(K, i)] * inv;
            NR_PRAGMA_UNROLL
            for (int j = 0; j < 16; ++j)
                if (j >= i) M[sym(i, j)] = fmaf(-f, M[sym(K, j)], M[sym(i, j)]);
            NR_PRAGMA_UNROLL
            for (int c = 0; c < NC; ++c) R[i][c] = fmaf(-f, R[K][c], R[i][c]);
        }
        dr_eliminate<K + 1>(M, R);
    }
}
template <int K, int NC>
__device__ __forceinline__ void dr_back_substitute(const float (&M)[136], float (&R)[16][NC]) {          // on the upper triangle left in M
    if constexpr (K >= 0) {
        const float inv = 1.0f / M[sym(K, K)];
        NR_PRAGMA_UNROLL
        for (int c = 0; c < NC; ++c) {
            float s = R[K][c];
            NR_PRAGMA_UNROLL
            for (int j = K + 1; j < 16; ++j) s = fmaf(-M[sym(K, j)], R[j][c], s);
            R[K][c] = s * inv;
        }
        dr_back_substitute<K - 1>(M, R);
    }
}

// per (point): alpha logit + SH colour.  view_rec [npts][rfn][kDbgFields] (the point kernel's per-view record),
// regs [16] (SphericalHarmonicsSolver.regs), alpha_out [npts], color_out [npts][3] (null: use_nr_color_for_dr).
#ifndef NR_DR_MINW
#define NR_DR_MINW 1
#endif
__global__ void __launch_bounds__(128, NR_DR_MINW) dr_points_kernel(const float* __restrict__ qc, const float* __restrict__ view_const,
                                                        const float* __restrict__ coords, const float* __restrict__ depth,
                                                        const float* __restrict__ rgba, const float* __restrict__ view_rec,
                                                        const float* __restrict__ regs, int rfn, int rn, int dn, int h, int w,
                                                        float ground, float* __restrict__ alpha_out, float* __restrict__ color_out) {
    const long long npts = (long long)rn * dn;
    const size_t imap = (size_t)h * w * 4;
    for (long long pi = (long long)blockIdx.x * blockDim.x + threadIdx.x; pi < npts; pi += (long long)gridDim.x * blockDim.x) {
        const int ray = (int)(pi / dn);
        const Ray r = make_ray<true>(qc, coords[2 * ray], coords[2 * ray + 1]);
        const float d = depth[pi];
        const float px = rn_add(r.cx, rn_mul(r.dx, d)), py = rn_add(r.cy, rn_mul(r.dy, d)), pz = rn_add(r.cz, rn_mul(r.dz, d));
        // ---- alpha (renderer.py:85-95) and the fit's weights (:103) --------------------------------------------------
        float s_va = 0.0f, s_v = 0.0f, s_hit = 0.0f;
        int n_valid = 0;
        for (int v = 0; v < rfn; ++v) {
            const float* rec = view_rec + ((size_t)pi * rfn + v) * kDbgFields;
            const float m = rec[0], hit = rec[4], vis = rec[5];     // hit, vis already masked (renderer.py:81-82)
            // compute_prob's logit (dist_decoder.py:137-138) on the un-masked values; where the mask is 0 it is replaced anyway
            const float logit = logf(rn_add(rn_div(hit, rn_add(rn_sub(vis, hit), 1e-5f)), 1e-5f));
            const float alpha = rn_add(rn_mul(logit, m), rn_mul(rn_sub(1.0f, m), ground));
            s_va = rn_add(s_va, rn_mul(vis, m > 0.0f ? alpha : ground));
            s_v = rn_add(s_v, vis);
            s_hit = rn_add(s_hit, hit);
            n_valid += m > 0.0f ? 1 : 0;
        }
        const float a_dr = rn_div(s_va, rn_add(s_v, 1e-5f));
        alpha_out[pi] = n_valid == 0 ? ground : a_dr;
        if (!color_out) continue;
        // ---- weighted SH least squares (sph_solver.py:33-50) ------------------------------------------------------------
        const float inv_hit = rn_add(s_hit, 1e-3f);
        float s_w = 0.0f;
        for (int v = 0; v < rfn; ++v) s_w = rn_add(s_w, rn_div(view_rec[((size_t)pi * rfn + v) * kDbgFields + 4], inv_hit));
        const float w_eps = s_w < 1e-4f ? 1e-4f : 0.0f;               // "insufficient" rays get a uniform floor
        float M[136], R[16][3];
        NR_PRAGMA_UNROLL
        for (int i = 0; i < 136; ++i) M[i] = 0.0f;
        NR_PRAGMA_UNROLL
        for (int i = 0; i < 16; ++i) { R[i][0] = 0.0f; R[i][1] = 0.0f; R[i][2] = 0.0f; }
        for (int v = 0; v < rfn; ++v) {
            const float* vc = view_const + v * kViewConst;
            const Proj pr = project_point<true>(vc, px, py, pz, (float)w, (float)h);
            const float wv = rn_add(rn_div(view_rec[((size_t)pi * rfn + v) * kDbgFields + 4], inv_hit), w_eps);
            float rgb[3];
            {
                const Taps t = make_taps(pr.u, pr.v, w, h, w, h);
                const float* mp = rgba + (size_t)v * imap;
                const float4 c00 = ld4(mp + (size_t)t.o00 * 4), c10 = ld4(mp + (size_t)t.o10 * 4);
                const float4 c01 = ld4(mp + (size_t)t.o01 * 4), c11 = ld4(mp + (size_t)t.o11 * 4);
                rgb[0] = blend4(c00.x, c10.x, c01.x, c11.x, t) * pr.mask;
                rgb[1] = blend4(c00.y, c10.y, c01.y, c11.y, t) * pr.mask;
                rgb[2] = blend4(c00.z, c10.z, c01.z, c11.z, t) * pr.mask;
            }
            float a[16], aw[16];
            sh16(pr.dirx, pr.diry, pr.dirz, a);
            NR_PRAGMA_UNROLL
            for (int i = 0; i < 16; ++i) aw[i] = rn_mul(a[i], wv);
            NR_PRAGMA_UNROLL
            for (int i = 0; i < 16; ++i) {
                NR_PRAGMA_UNROLL
                for (int j = 0; j < 16; ++j)          // (constant trip count + a predicate that folds: a bound that depends on i keeps the
                    if (j >= i) M[sym(i, j)] = fmaf(aw[i], a[j], M[sym(i, j)]);      //  inner loop from being unrolled before the outer one is)
                NR_PRAGMA_UNROLL
                for (int c = 0; c < 3; ++c) R[i][c] = fmaf(aw[i], rgb[c], R[i][c]);
            }
        }
        NR_PRAGMA_UNROLL
        for (int i = 0; i < 16; ++i) M[sym(i, i)] += regs[i];
        // LDL^T elimination of the SPD system (no pivoting needed), three right-hand sides.  One function instantiation per pivot: with the
        // pivot a run-time loop variable hipcc stopped unrolling part-way, indexed M / R dynamically and put both arrays into scratch
        // memory (752 B per lane, every access a memory round trip at one wave per SIMD: 2.99 ms per launch of 1.6 M points, round 4)
        dr_eliminate<0>(M, R);
        dr_back_substitute<15>(M, R);
        float q[16];
        sh16(r.qx, r.qy, r.qz, q);
        NR_PRAGMA_UNROLL
        for (int c = 0; c < 3; ++c) {
            float s = 0.0f;
            NR_PRAGMA_UNROLL
            for (int i = 0; i < 16; ++i) s = fmaf(q[i], R[i][c], s);
            color_out[pi * 3 + c] = s;
        }
    }
}

// per ray: decode_alpha_value (sigmoid, dist_decoder.py:142-144), alpha_values2hit_prob (render_ops.py:72-80, sequential
// transmittance product as the ray kernel's), pixel colour.  colors [rn*dn][stride] starting at `first` (the SH colours:
// stride 3, first 0; use_nr_color_for_dr: the point records' blended colour, stride kPointRec, first 16).
__global__ void dr_rays_kernel(const float* __restrict__ alpha, const float* __restrict__ colors, int stride, int first, int rn, int dn,
                               float* __restrict__ hit_out, float* __restrict__ pixel_out) {
    for (int ray = blockIdx.x * blockDim.x + threadIdx.x; ray < rn; ray += gridDim.x * blockDim.x) {
        float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
        for (int i = 0; i < dn; ++i) {
            const size_t pi = (size_t)ray * dn + i;
            const float a = 1.0f / (1.0f + expf(-alpha[pi]));
            const float hit = a * T;
            T = T * ((1.0f - a) + 1e-10f);
            hit_out[pi] = hit;
            const float* c = colors + pi * stride + first;
            c0 = rn_add(c0, rn_mul(hit, c[0])); c1 = rn_add(c1, rn_mul(hit, c[1])); c2 = rn_add(c2, rn_mul(hit, c[2]));
        }
        pixel_out[ray * 3 + 0] = c0; pixel_out[ray * 3 + 1] = c1; pixel_out[ray * 3 + 2] = c2;
    }
}

// =================================================================================================================================
#ifndef NR_INFERENCE_ONLY            // (the bf16-operand build has no training path: no nr_kernels_bwd2.h)
// Backward of direct rendering (cfg['use_dr_loss'] / ['use_dr_fine_loss'], network/loss.py:70-76): the gradient of a loss on
// pixel_colors_dr / hit_prob_dr (network/renderer.py:85-125, network/sph_solver.py:33-59) with respect to the dist decoder's
// per-(point, view) outputs (mu0, mu1, s0, s1, aw, vis_dec), which the caller carries on through the decoder rows' backward.
// The view colours C_v are image samples and the directions A_v geometry: neither gets a gradient.
//   rays  (per ray, reverse of dr_rays_kernel): g_i = d hit_i + d pixel . c_i, lambda_i = dL/dT_i from the back,
//         d a_i = T_i (g_i - lambda_{i+1}), d alpha_i = d a_i a_i (1 - a_i), d c_i = d pixel hit_i.  The T_i of the forward sweep are
//         parked in d_alpha and read back by the reverse sweep (no division by 1 - a_i).
//   points (per point, reverse of dr_points_kernel): with M = sum_v w'_v A_v A_v^T + diag(regs) and theta = M^-1 sum_v w'_v A_v C_v^T,
//         colour = theta^T q, the upstream G_theta = q g^T is rank one, so Lambda = M^-1 G_theta = y g^T with y = M^-1 q: y is a fourth
//         right-hand side of the forward's LDL^T elimination.  dL/dw_v = (y . A_v) (g . (C_v - theta^T A_v)), through w_v = h_v / (sum h
//         + 1e-3) to h_v (the "insufficient" floor is a constant); the alpha logit mean sum s_v a_v / (sum s_v + 1e-5) to s_v and a_v;
//         a_v = log(h / (s - h + 1e-5) + 1e-5) to (h, s); compute_prob (dist_decoder.py:109-140) to the decoder outputs (b2_prob_bwd).
// Masked (point, view) pairs contribute nothing downstream (h, s are multiplied by the mask, a_v is replaced by `ground`): zero rows.

constexpr int kDrDecGrads = 6;     // d (mu0, mu1, s0, s1, aw, vis_dec) per (point, view)

// colour C_v (masked by the projection, as the forward) and SH basis A_v of the direction to reference view v
__device__ __forceinline__ Proj dr_view_sample(const float* __restrict__ vc, const float* __restrict__ rgba_v, float px, float py, float pz,
                                               int h, int w, float (&rgb)[3], float (&a)[16]) {
    const Proj pr = project_point<true>(vc, px, py, pz, (float)w, (float)h);
    const Taps t = make_taps(pr.u, pr.v, w, h, w, h);
    const float4 c00 = ld4(rgba_v + (size_t)t.o00 * 4), c10 = ld4(rgba_v + (size_t)t.o10 * 4);
    const float4 c01 = ld4(rgba_v + (size_t)t.o01 * 4), c11 = ld4(rgba_v + (size_t)t.o11 * 4);
    rgb[0] = blend4(c00.x, c10.x, c01.x, c11.x, t) * pr.mask;
    rgb[1] = blend4(c00.y, c10.y, c01.y, c11.y, t) * pr.mask;
    rgb[2] = blend4(c00.z, c10.z, c01.z, c11.z, t) * pr.mask;
    sh16(pr.dirx, pr.diry, pr.dirz, a);
    return pr;
}

// per point: view_rec [npts][rfn][kDbgFields] (the forward's record), d_alpha [npts], d_color [npts][3] (null: no colour gradient)
// -> d_dec [npts][rfn][kDrDecGrads].  d_dec's first field doubles as the per-view dL/dw_v between the two view sweeps.
__global__ void __launch_bounds__(128) dr_points_backward_kernel(const float* __restrict__ qc, const float* __restrict__ view_const,
                                                                 const float* __restrict__ coords, const float* __restrict__ depth,
                                                                 const float* __restrict__ rgba, const float* __restrict__ view_rec,
                                                                 const float* __restrict__ regs, const float* __restrict__ d_alpha,
                                                                 const float* __restrict__ d_color, int rfn, int rn, int dn, int h, int w,
                                                                 int use_vis, float* __restrict__ d_dec) {
    const long long npts = (long long)rn * dn;
    const size_t imap = (size_t)h * w * 4;
    const float qnearp = qc[24], qfarp = qc[25], qinv = qc[27];
    for (long long pi = (long long)blockIdx.x * blockDim.x + threadIdx.x; pi < npts; pi += (long long)gridDim.x * blockDim.x) {
        const int ray = (int)(pi / dn), smp = (int)(pi - (long long)ray * dn);
        const Ray r = make_ray<true>(qc, coords[2 * ray], coords[2 * ray + 1]);
        const float* drow = depth + (size_t)ray * dn;
        const float d = drow[smp];
        const float px = rn_add(r.cx, rn_mul(r.dx, d)), py = rn_add(r.cy, rn_mul(r.dy, d)), pz = rn_add(r.cz, rn_mul(r.dz, d));
        const float* prec = view_rec + (size_t)pi * rfn * kDbgFields;
        float* pout = d_dec + (size_t)pi * rfn * kDrDecGrads;
        // ---- forward sums of the alpha mean and of the fit's weights (as dr_points_kernel) ---------------------------------------
        float s_va = 0.0f, s_v = 0.0f, s_hit = 0.0f;
        int n_valid = 0;
        for (int v = 0; v < rfn; ++v) {
            const float* rec = prec + v * kDbgFields;
            const float m = rec[0], hit = rec[4], vis = rec[5];
            const float logit = logf(rn_add(rn_div(hit, rn_add(rn_sub(vis, hit), 1e-5f)), 1e-5f));
            s_va = rn_add(s_va, rn_mul(vis, m > 0.0f ? logit : 0.0f));
            s_v = rn_add(s_v, vis);
            s_hit = rn_add(s_hit, hit);
            n_valid += m > 0.0f ? 1 : 0;
        }
        const float inv_v = 1.0f / rn_add(s_v, 1e-5f);
        const float a_dr = rn_mul(s_va, inv_v);
        const float ga = (n_valid > 0 && d_alpha) ? d_alpha[pi] : 0.0f;        // alpha_dr = ground (a constant) where no view sees the point
        const float hit_den = rn_add(s_hit, 1e-3f), inv_hit = 1.0f / hit_den;
        const float g0 = d_color ? d_color[pi * 3 + 0] : 0.0f, g1 = d_color ? d_color[pi * 3 + 1] : 0.0f;
        const float g2 = d_color ? d_color[pi * 3 + 2] : 0.0f;
        float sum_dww = 0.0f;
        if (g0 != 0.0f || g1 != 0.0f || g2 != 0.0f) {
            float s_w = 0.0f;
            for (int v = 0; v < rfn; ++v) s_w = rn_add(s_w, rn_div(prec[v * kDbgFields + 4], hit_den));
            const float w_eps = s_w < 1e-4f ? 1e-4f : 0.0f;
            // ---- the forward's normal equations, with y = M^-1 q as a fourth right-hand side -------------------------------------
            float M[136], R[16][4];
            NR_PRAGMA_UNROLL
            for (int i = 0; i < 136; ++i) M[i] = 0.0f;
            NR_PRAGMA_UNROLL
            for (int i = 0; i < 16; ++i) { R[i][0] = 0.0f; R[i][1] = 0.0f; R[i][2] = 0.0f; }
            for (int v = 0; v < rfn; ++v) {
                float rgb[3], a[16], aw[16];
                dr_view_sample(view_const + v * kViewConst, rgba + (size_t)v * imap, px, py, pz, h, w, rgb, a);
                const float wv = rn_add(rn_div(prec[v * kDbgFields + 4], hit_den), w_eps);
                NR_PRAGMA_UNROLL
                for (int i = 0; i < 16; ++i) aw[i] = rn_mul(a[i], wv);
                NR_PRAGMA_UNROLL
                for (int i = 0; i < 16; ++i) {
                    NR_PRAGMA_UNROLL
                    for (int j = 0; j < 16; ++j)
                        if (j >= i) M[sym(i, j)] = fmaf(aw[i], a[j], M[sym(i, j)]);
                    NR_PRAGMA_UNROLL
                    for (int c = 0; c < 3; ++c) R[i][c] = fmaf(aw[i], rgb[c], R[i][c]);
                }
            }
            NR_PRAGMA_UNROLL
            for (int i = 0; i < 16; ++i) M[sym(i, i)] += regs[i];
            {
                float q[16];
                sh16(r.qx, r.qy, r.qz, q);
                NR_PRAGMA_UNROLL
                for (int i = 0; i < 16; ++i) R[i][3] = q[i];
            }
            dr_eliminate<0>(M, R);
            dr_back_substitute<15>(M, R);
            // ---- dL/dw_v for every view (parked in d_dec[.][v][0]) and sum_v dL/dw_v w_v -----------------------------------------
            for (int v = 0; v < rfn; ++v) {
                float rgb[3], a[16];
                dr_view_sample(view_const + v * kViewConst, rgba + (size_t)v * imap, px, py, pz, h, w, rgb, a);
                float ya = 0.0f, p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
                NR_PRAGMA_UNROLL
                for (int i = 0; i < 16; ++i) {
                    ya = fmaf(R[i][3], a[i], ya);
                    p0 = fmaf(R[i][0], a[i], p0); p1 = fmaf(R[i][1], a[i], p1); p2 = fmaf(R[i][2], a[i], p2);
                }
                const float dw = ya * (g0 * (rgb[0] - p0) + g1 * (rgb[1] - p1) + g2 * (rgb[2] - p2));
                pout[v * kDrDecGrads] = dw;
                sum_dww = fmaf(dw, prec[v * kDbgFields + 4] * inv_hit, sum_dww);
            }
        } else {
            for (int v = 0; v < rfn; ++v) pout[v * kDrDecGrads] = 0.0f;
        }
        // ---- per view: -> d h, d s -> compute_prob's backward -> the decoder outputs ------------------------------------------------
        const float s_c = norm_inv_depth_fast(d, qnearp, qfarp, qinv);
        const float s_n = norm_inv_depth_fast(drow[smp + 1 < dn ? smp + 1 : smp], qnearp, qfarp, qinv);
        const float s_p = norm_inv_depth_fast(drow[smp > 0 ? smp - 1 : 0], qnearp, qfarp, qinv);
        const float half_c = (smp == dn - 1) ? 500000.0f : (s_n - s_c) * 0.5f;
        const float hi = half_c, lo = (smp == 0) ? half_c : (s_c - s_p) * 0.5f;
        for (int v = 0; v < rfn; ++v) {
            const float* rec = prec + v * kDbgFields;
            float* o = pout + v * kDrDecGrads;
            if (!(rec[0] > 0.0f)) {
                NR_PRAGMA_UNROLL
                for (int k = 0; k < kDrDecGrads; ++k) o[k] = 0.0f;
                continue;
            }
            const float hit = rec[4], vis = rec[5];            // the mask is 1 here: masked = un-masked values
            float dh = (o[0] - sum_dww) * inv_hit;
            float ds = 0.0f;
            if (ga != 0.0f) {
                const float den = rn_add(rn_sub(vis, hit), 1e-5f);
                const float ratio = hit / den;
                const float logit = logf(ratio + 1e-5f);
                ds = ga * (logit - a_dr) * inv_v;
                const float dr_ = ga * vis * inv_v / (ratio + 1e-5f) / (den * den);
                dh = fmaf(dr_, vis + 1e-5f, dh);
                ds = fmaf(-dr_, hit, ds);
            }
            const float* vc = view_const + v * kViewConst;
            const float tref = norm_inv_depth_fast(fmaxf(rec[3], 1e-5f), vc[15], vc[16], vc[17]);
            const bool uv = use_vis != 0;
            float dmu0 = 0.0f, dmu1 = 0.0f, ds0 = 0.0f, ds1 = 0.0f, daw = 0.0f, dnu = 0.0f;
            b2_prob_bwd(tref - lo, tref + hi, rec[6], rec[7], rec[8], rec[9], rec[10], uv ? rec[11] : 1.0f, uv, ds, dh,
                        dmu0, dmu1, ds0, ds1, daw, dnu);
            o[0] = dmu0; o[1] = dmu1; o[2] = ds0; o[3] = ds1; o[4] = daw; o[5] = dnu;
        }
    }
}

// per ray, the reverse of dr_rays_kernel on the SH colours [rn*dn][3]: d_pixel [rn][3], d_hit [rn][dn] (null: none)
// -> d_alpha [rn*dn] (of the logits alpha_dr), d_colors [rn*dn][3]
__global__ void dr_rays_backward_kernel(const float* __restrict__ alpha, const float* __restrict__ colors, const float* __restrict__ d_pixel,
                                        const float* __restrict__ d_hit, int rn, int dn, float* __restrict__ d_alpha,
                                        float* __restrict__ d_colors) {
    for (int ray = blockIdx.x * blockDim.x + threadIdx.x; ray < rn; ray += gridDim.x * blockDim.x) {
        const float gp0 = d_pixel[ray * 3 + 0], gp1 = d_pixel[ray * 3 + 1], gp2 = d_pixel[ray * 3 + 2];
        const size_t base = (size_t)ray * dn;
        float T = 1.0f;
        for (int i = 0; i < dn; ++i) {
            const size_t pi = base + i;
            const float a = 1.0f / (1.0f + expf(-alpha[pi]));
            const float hit = a * T;
            d_alpha[pi] = T;                                          // T_i, read back by the reverse sweep
            d_colors[pi * 3 + 0] = gp0 * hit; d_colors[pi * 3 + 1] = gp1 * hit; d_colors[pi * 3 + 2] = gp2 * hit;
            T = T * ((1.0f - a) + 1e-10f);
        }
        float lam = 0.0f;                                             // dL/dT_{i+1}
        for (int i = dn - 1; i >= 0; --i) {
            const size_t pi = base + i;
            const float a = 1.0f / (1.0f + expf(-alpha[pi]));
            const float Ti = d_alpha[pi];
            const float* c = colors + pi * 3;
            const float g = (d_hit ? d_hit[pi] : 0.0f) + gp0 * c[0] + gp1 * c[1] + gp2 * c[2];
            const float da = Ti * (g - lam);
            lam = fmaf(g, a, lam * ((1.0f - a) + 1e-10f));
            d_alpha[pi] = da * a * (1.0f - a);
        }
    }
}
#endif  // NR_INFERENCE_ONLY

}  // namespace nr
