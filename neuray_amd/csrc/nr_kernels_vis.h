// Visibility-guided coarse pass (cfg['hip_coarse_pass'] = 'visibility'): the coarse hit probabilities
// that place the fine samples, from the input views' visibility alone -
//   alpha(point) = sum_v vis_v alpha_v / (sum_v vis_v + 1e-5)     (predict_alpha_values_dr, network/renderer.py:85-94)
//   hit_prob     = alpha_values2hit_prob(sigmoid(alpha))         (decode_alpha_value + render_ops.py:72-80; renderer.py:121-123)
// i.e. the hit_prob_dr of direct rendering, without the aggregation network and without a per-(point, view) record in global
// memory.  vis_points_kernel runs, per (point, view): projection, the ray_feats gather, the dist-decoder heads and compute_prob - the
// point kernel's own device functions (nr_device.h) on the pass's packed weights, in the point kernel's operation order, so that
// the per-view (mask, hit, vis) are bit for bit what its per-view record (PointParams.dbg, fields 0 / 4 / 5) holds - then the
// cross-view mean of dr_points_kernel (nr_kernels_dr.h), literally, one lane per point over the views in ascending index.
// vis_rays_kernel is dr_rays_kernel's sigmoid / transmittance sweep plus the ray mask of the ray kernel (renderer.py:195-198).
// fp32 MFMA only (the heads are a small kernel; NEURAY_ARITH_X3 stays with the network passes).
#pragma once
#include "nr_kernels.h"          // SlotCount, the point kernel's tiling

namespace nr {

struct VisParams {
    const float* que_const;    // [kQueryConst]
    const float* view_const;   // [rfn][kViewConst]
    const float* coords;       // [rn][2] pixel (x, y)
    const float* depth;        // [rn][dn]
    const float* ray_feats;    // [rfn][fh][fw][32]
    const float* weights;      // packed pass weights (folded or not: the dist heads are the same)
    float* alpha;              // [rn*dn] logits
    int* nvalid;               // [rn*dn] views that see the point
    int rfn, rn, dn, h, w, fh, fw;
    int use_vis;
    float var_bias, ground;
};

constexpr int kVisXchFloats = kMaxViews * 3 * 16;     // per-view (mask, hit, vis) of the tile's 16 points
inline size_t vis_smem_bytes() { return sizeof(float) * (kWeightLdsFloats + kVisXchFloats); }

// the point kernel's phase_enter for a kernel that runs the dist phases only: PH_DIST_M -> PH_DIST_VA (-> PH_DIST_S) -> the next
// tile's PH_DIST_M.  seq = phases entered so far (the two stage regions alternate along it).
template <int PH, int NEXT>
__device__ __forceinline__ LdsW vis_phase_enter(float* wl, nr_wbuf W, int seq, bool issue_next, int wave, int nw, int lane) {
    constexpr int RF = kStageRegionBytes / 4;
    NR_BLOCK_SYNC();
    const int r = seq & 1;
    if (issue_next) stage_issue<NEXT>(wl + (r ^ 1) * RF, W, wave, nw, lane);
    return LdsW{wl + r * RF, phase_begin(PH) * 4};
}

#ifndef NR_VIS_MINW
#define NR_VIS_MINW 2          // workgroups per CU the kernel is compiled for (8 waves each at 15 / 16 views: 128 VGPRs)
#endif

// One workgroup = ceil(rfn / 2) waves x one tile of 16 sample points (the same sample index of 16 neighbouring rays, the inference
// tiling of points_kernel); wave w takes the views 2 w, 2 w + 1.  A slot whose 16 columns are all outside its view is not
// evaluated (it hands mask = hit = vis = 0 to the cross-view step: what the masked products of renderer.py:81-82 give).
template <bool HAS_VIS>
__global__ void __launch_bounds__(64 * (kMaxViews / 2), NR_VIS_MINW) vis_points_kernel(VisParams p) {
    NR_DYNAMIC_SMEM(float, smem);
    constexpr int NS = 2, NPH = HAS_VIS ? 3 : 2;
    const int lane = threadIdx.x & 63;
    const int wave = NR_UNIFORM((int)(threadIdx.x >> 6));
    const int nw = (p.rfn + 1) / 2;
    const int g = lane >> 4, c = lane & 15;
    float* wl = smem;
    float* xv = smem + kWeightLdsFloats;               // [view][mask | hit | vis][point]
    const nr_wbuf W = nr_make_wbuf(p.weights, sizeof(float) * kPackedPassFloats);
    const float w_m1 = (float)(p.w - 1), h_m1 = (float)(p.h - 1);
    const float inv_w_m1 = 1.0f / w_m1, inv_h_m1 = 1.0f / h_m1;
    const size_t fmap = (size_t)p.fh * p.fw * 32;
    const nr_mbuf rf_map = nr_make_mbuf(p.ray_feats, sizeof(float) * fmap * p.rfn);
    const int goff = 32 * g;
    const int dn = p.dn;
    const bool use_vis = p.use_vis != 0;
    const int bid = (int)(blockIdx.x % 8) * (int)(gridDim.x / 8) + (int)(blockIdx.x / 8);      // XCD-aware tile map (points_kernel)
    const int nloop = ((p.rn + 15) / 16) * dn * 16;
    const int G = (int)gridDim.x;
    auto tile_base = [&](int it) { return (it * G + bid) * 16; };
    int seq = 0;
    if (tile_base(0) < nloop) stage_issue<PH_DIST_M>(wl, W, wave, nw, lane);
    for (int it = 0, base; (base = tile_base(it)) < nloop; ++it, seq += NPH) {
        const bool more = tile_base(it + 1) < nloop;
        // ---------------- geometry: as points_kernel (make_ray<false>, project_point<false>, half intervals, norm_inv_depth_fast) -----
        int pidx, vidx[NS]; bool pvalid;
        float mask[NS], tref[NS], pu[NS], pv[NS], lo, hi;
        float tref_sc;                                  // two active slots: lane groups s and 2 + s evaluate slot s (logistic_prob_scattered)
        int soff_f[NS];
        {
            const float* __restrict__ qc = p.que_const;
            const float qnearp = qc[24], qfarp = qc[25], qinv = qc[27];
            const int tix = base >> 4, rb = tix / dn, smp = tix - rb * dn;       // wave-uniform
            int ray = rb * 16 + c;
            pvalid = ray < p.rn;
            ray = pvalid ? ray : p.rn - 1;
            pidx = ray * dn + smp;
            const Ray r = make_ray<false>(qc, p.coords[2 * ray], p.coords[2 * ray + 1]);
            const float* drow = p.depth + (size_t)ray * dn;
            const float d = drow[smp];
            float s_c, s_n, s_p, s_x;
            {
                const int nxt = smp + 1 < dn ? smp + 1 : smp, prv = smp > 0 ? smp - 1 : 0;
                const float dg = drow[g == 0 ? smp : (g == 1 ? nxt : prv)];
                nr_group_gather4(norm_inv_depth_fast(dg, qnearp, qfarp, qinv), s_c, s_n, s_p, s_x);
            }
            const float half_c = (smp == dn - 1) ? 500000.0f : (s_n - s_c) * 0.5f;
            const float half_p = (s_c - s_p) * 0.5f;
            hi = half_c;
            lo = (smp == 0) ? half_c : half_p;
            const float px = rn_add(r.cx, rn_mul(r.dx, d));
            const float py = rn_add(r.cy, rn_mul(r.dy, d));
            const float pz = rn_add(r.cz, rn_mul(r.dz, d));
            NR_PRAGMA_UNROLL
            for (int s = 0; s < NS; ++s) {
                const int vraw = wave * NS + s;
                const bool vok = vraw < p.rfn;                  // padding view of an odd rfn: masked out
                const int view = vok ? vraw : p.rfn - 1;
                const float* __restrict__ vc = p.view_const + view * kViewConst;
                Proj pr = project_point<false>(vc, px, py, pz, (float)p.w, (float)p.h);
                if (!vok) pr.mask = 0.0f;
                mask[s] = pr.mask;
                tref[s] = norm_inv_depth_fast(fmaxf(pr.z, 1e-5f), vc[15], vc[16], vc[17]);
                pu[s] = pr.u; pv[s] = pr.v;
                soff_f[s] = view * (int)(fmap * sizeof(float));
                vidx[s] = vraw;
            }
            // (selected here, from the values themselves: indexed after the lone-slot move below, hipcc keeps tref[] in scratch memory)
            tref_sc = (g & 1) ? tref[1] : tref[0];
        }

        // ---------------- the heads of NA active slots (slots [0, NA)); every variant runs the same barriers and stage copies ---------
        auto tile = [&](auto na_tag) NR_LAMBDA_INLINE {
            constexpr int NA = decltype(na_tag)::value, NA1 = NA > 0 ? NA : 1;
            constexpr bool SC = NA == 2;               // the two slots' narrow rows as one reduce-scattered batch (points_kernel)
            float fray[NA1][8];
            if constexpr (NA > 0) {
                Taps tfs[NA];
                float4 qf[NA][8];
                NR_PRAGMA_UNROLL
                for (int s = 0; s < NA; ++s) {
                    tfs[s] = make_taps_fast(pu[s], pv[s], w_m1, h_m1, inv_w_m1, inv_h_m1, p.fw, p.fh, p.fw == p.w && p.fh == p.h);
                    issue8(rf_map, goff, soff_f[s], tfs[s], qf[s]);
                }
                NR_PIN();
                NR_PRAGMA_UNROLL
                for (int s = 0; s < NA; ++s) {
                    blend8(qf[s], tfs[s], mask[s], fray[s]);
                    NR_PRAGMA_UNROLL
                    for (int k = 0; k < 8; ++k) NR_KEEP(fray[s][k]);
                }
                NR_PIN();
            }
            float none[NA1][1];
            NR_PRAGMA_UNROLL
            for (int s = 0; s < NA1; ++s) none[s][0] = 0.0f;
            NoLayer last;
            float hit[NA1], vis[NA1];
            {
                float h1[NA1][8], h2[NA1][8], fm[NA1][2], fv[NA1][2], fa[NA1][1];
                float mu0[NA1], mu1[NA1], s0[NA1], s1[NA1], aw[NA1], nu[NA1];
                float mu_g = 0.0f, sd_g = 0.0f, aw_g = 0.0f, nu_g = 1.0f;
                LayerPre<L_DV2> p_dv2; VecPre<L_DFIN_V> p_fv;
                const LdsW W1 = vis_phase_enter<PH_DIST_M, PH_DIST_VA>(wl, W, seq, true, wave, nw, lane);
                if constexpr (NA > 0) {
                    LayerPre<L_DM1> p_dm1; LayerPre<L_DM2> p_dm2; LayerPre<L_DV1> p_dv1; VecPre<L_DFIN_M> p_fm;
                    layer_prefetch<L_DM1>(W1, lane, p_dm1);
                    layer_fwd<L_DM1, NA, ACT_ELU>(W1, lane, p_dm1, fray, none, h1, p_dm2);
                    layer_fwd<L_DM2, NA, ACT_ELU>(W1, lane, p_dm2, h1, none, h2, p_fm);
                    layer_prefetch<L_DV1>(W1, lane, p_dv1);
                    if constexpr (SC) mu_g = softplus(layer_vec_scatter_2x2<L_DFIN_M>(p_fm, h2, g));
                    else layer_vec<L_DFIN_M, NA>(p_fm, h2, fm);
                    layer_fwd<L_DV1, NA, ACT_ELU>(W1, lane, p_dv1, fray, none, h1, last);
                }
                const LdsW W2 = vis_phase_enter<PH_DIST_VA, HAS_VIS ? PH_DIST_S : PH_DIST_M>(wl, W, seq + 1, HAS_VIS || more, wave, nw, lane);
                if constexpr (NA > 0) {
                    LayerPre<L_DA1> p_da1; LayerPre<L_DA2> p_da2; VecPre<L_DFIN_A> p_fa;
                    layer_prefetch<L_DV2>(W2, lane, p_dv2);
                    layer_fwd<L_DV2, NA, ACT_ELU>(W2, lane, p_dv2, h1, none, h2, p_fv);
                    layer_prefetch<L_DA1>(W2, lane, p_da1);
                    if constexpr (SC) sd_g = softplus(layer_vec_scatter_2x2<L_DFIN_V>(p_fv, h2, g)) + p.var_bias;
                    else {
                        layer_vec<L_DFIN_V, NA>(p_fv, h2, fv);
                        NR_PRAGMA_UNROLL
                        for (int s = 0; s < NA; ++s) {
                            mu0[s] = softplus(fm[s][0]); mu1[s] = softplus(fm[s][1]);
                            s0[s] = softplus(fv[s][0]) + p.var_bias; s1[s] = softplus(fv[s][1]) + p.var_bias;
                        }
                    }
                    layer_fwd<L_DA1, NA, ACT_ELU>(W2, lane, p_da1, fray, none, h1, p_da2);
                    layer_fwd<L_DA2, NA, ACT_ELU>(W2, lane, p_da2, h1, none, h2, p_fa);
                    if constexpr (SC) aw_g = sigmoidf(layer_vec_scatter_1x2<L_DFIN_A, 0>(p_fa, h2));
                    else layer_vec<L_DFIN_A, NA>(p_fa, h2, fa);
                }
                if constexpr (HAS_VIS) {
                    const LdsW W2s = vis_phase_enter<PH_DIST_S, PH_DIST_M>(wl, W, seq + 2, more, wave, nw, lane);
                    if constexpr (NA > 0) {
                        LayerPre<L_DS1> p_ds1; LayerPre<L_DS2> p_ds2; VecPre<L_DFIN_S> p_fs;
                        float fs[NA][1];
                        layer_prefetch<L_DS1>(W2s, lane, p_ds1);
                        layer_fwd<L_DS1, NA, ACT_ELU>(W2s, lane, p_ds1, fray, none, h1, p_ds2);
                        layer_fwd<L_DS2, NA, ACT_ELU>(W2s, lane, p_ds2, h1, none, h2, p_fs);
                        if constexpr (SC) nu_g = sigmoidf(layer_vec_scatter_1x2<L_DFIN_S, 0>(p_fs, h2));
                        else {
                            layer_vec<L_DFIN_S, NA>(p_fs, h2, fs);
                            NR_PRAGMA_UNROLL
                            for (int s = 0; s < NA; ++s) { aw[s] = sigmoidf(fa[s][0]); nu[s] = sigmoidf(fs[s][0]); }
                        }
                    }
                } else if constexpr (!SC) {
                    NR_PRAGMA_UNROLL
                    for (int s = 0; s < NA; ++s) { aw[s] = sigmoidf(fa[s][0]); nu[s] = 1.0f; }
                }
                // ---------------- compute_prob (dist_decoder.py:109-140) and the mask (renderer.py:81-82) -------------------------
                float vh_[2][NA1];
                if constexpr (SC) {
                    float v_, h_;
                    logistic_prob_scattered(tref_sc, lo, hi, mu_g, sd_g, aw_g, nu_g, use_vis && HAS_VIS, v_, h_);
                    nr_group_gather2(v_, vh_[0][0], vh_[0][1]);
                    nr_group_gather2(h_, vh_[1][0], vh_[1][1]);
                } else {
                    NR_PRAGMA_UNROLL
                    for (int s = 0; s < NA; ++s)
                        logistic_prob(tref[s], lo, hi, mu0[s], mu1[s], s0[s], s1[s], aw[s], nu[s], use_vis && HAS_VIS, vh_[0][s], vh_[1][s]);
                }
                NR_PRAGMA_UNROLL
                for (int s = 0; s < NA; ++s) { vis[s] = vh_[0][s] * mask[s]; hit[s] = vh_[1][s] * mask[s]; }
            }
            // per-view (mask, hit, vis) -> LDS; an idle slot hands over zeros
            if (g == 0) {
                NR_PRAGMA_UNROLL
                for (int s = 0; s < NS; ++s) {
                    float* x = xv + vidx[s] * 48 + c;
                    x[0] = s < NA ? mask[s < NA ? s : 0] : 0.0f;
                    x[16] = s < NA ? hit[s < NA ? s : 0] : 0.0f;
                    x[32] = s < NA ? vis[s < NA ? s : 0] : 0.0f;
                }
            }
        };

        {
            const bool a0 = __ballot(mask[0] != 0.0f) != 0ull, a1 = __ballot(mask[1] != 0.0f) != 0ull;
            const int na = (a0 ? 1 : 0) + (a1 ? 1 : 0);
            if (na == 2) {
                tile(SlotCount<2>{});
            } else if (na == 1) {
                if (!a0) {              // the lone active slot becomes slot 0 (and the idle one slot 1)
                    const int v0 = vidx[0];
                    mask[0] = mask[1]; tref[0] = tref[1]; pu[0] = pu[1]; pv[0] = pv[1]; soff_f[0] = soff_f[1];
                    vidx[0] = vidx[1]; vidx[1] = v0;
                }
                tile(SlotCount<1>{});
            } else {
                tile(SlotCount<0>{});
            }
        }

        // ---------------- cross-view mean: dr_points_kernel's alpha block (nr_kernels_dr.h), views in ascending index -------------------
        // (xv is written again two or three barriers on, behind the next tile's phases: no second barrier here)
        NR_BLOCK_SYNC();
        if (wave == 0 && lane < 16 && pvalid) {
            const float ground = p.ground;
            float s_va = 0.0f, s_v = 0.0f;
            int n_valid = 0;
            for (int v = 0; v < p.rfn; ++v) {
                const float m = xv[v * 48 + c], hit = xv[v * 48 + 16 + c], vis = xv[v * 48 + 32 + c];
                const float logit = logf(rn_add(rn_div(hit, rn_add(rn_sub(vis, hit), 1e-5f)), 1e-5f));
                const float alpha = rn_add(rn_mul(logit, m), rn_mul(rn_sub(1.0f, m), ground));
                s_va = rn_add(s_va, rn_mul(vis, m > 0.0f ? alpha : ground));
                s_v = rn_add(s_v, vis);
                n_valid += m > 0.0f ? 1 : 0;
            }
            const float a_dr = rn_div(s_va, rn_add(s_v, 1e-5f));
            p.alpha[pidx] = n_valid == 0 ? ground : a_dr;
            p.nvalid[pidx] = n_valid;
        }
    }
}

// per ray: dr_rays_kernel's sigmoid + transmittance sweep (the same expressions), and the ray mask of the ray kernel from the valid-view
// counts: more than point_num samples seen by more than view_num views (renderer.py:195-198; integer logic)
__global__ void vis_rays_kernel(const float* __restrict__ alpha, const int* __restrict__ nvalid, int rn, int dn, int view_num, int point_num,
                                float* __restrict__ hit_out, unsigned char* __restrict__ ray_mask) {
    for (int ray = blockIdx.x * blockDim.x + threadIdx.x; ray < rn; ray += gridDim.x * blockDim.x) {
        float T = 1.0f;
        int cnt = 0;
        for (int i = 0; i < dn; ++i) {
            const size_t pi = (size_t)ray * dn + i;
            const float a = 1.0f / (1.0f + expf(-alpha[pi]));
            const float hit = a * T;
            T = T * ((1.0f - a) + 1e-10f);
            hit_out[pi] = hit;
            cnt += nvalid[pi] > view_num ? 1 : 0;
        }
        if (ray_mask) ray_mask[ray] = cnt > point_num ? 1 : 0;
    }
}

}  // namespace nr
