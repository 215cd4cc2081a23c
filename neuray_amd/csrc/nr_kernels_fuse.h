// Geometry export (neuray_amd/geometry.py): the cross-view depth consistency test and the fusion of per-view depth
// maps into one coloured, oriented point cloud.  The procedural ray caster's layout (nr_kernels_proc.h): one thread per pixel, one wave per 64
// neighbouring pixels of a row, four rows per workgroup, the view index from the block; the source slot loop has the same trip count in every
// lane, so every pose / K / K^-1 / nn_ids entry is read at a wave-uniform address and arrives through scalar loads.  The arithmetic is
// geometry.consistency_numpy's / fuse_numpy's, operation by operation, in fp32 without contraction (no fmaf anywhere in this file).  No LDS.
//
// Pixel centres sit at integer coordinates.  For pixel (x, y) of view i with depth d > 0 and source slot s, j = nn_ids[i][s]:
//   Xw = R_i^T (K_i^-1 [x,y,1]^T d - t_i);  Pc = R_j Xw + t_j, z = Pc.z, q = K_j Pc, (u, v) = q.xy / q.z, (un, vn) = floor((u, v) + 0.5)
//   seen        z > 0, (un, vn) inside the image, d_j = D_j[vn][un] > 0          (the nearest texel: no depth is interpolated across a silhouette)
//   Yw = R_j^T (K_j^-1 [un,vn,1]^T d_j - t_j);  Qc = R_i Yw + t_i, q' = K_i Qc
//   e_px^2 = (q'.x / q'.z - x)^2 + (q'.y / q'.z - y)^2,  e_d = |Qc.z - d| / d
//   consistent  seen, Qc.z > 0, e_px^2 < tau_px^2, e_d < tau_d
//   occluded    seen, not consistent, (z - d_j) / d_j > tau_d                     (the source sees a nearer surface)
#pragma once
#include "nr_platform.h"

#include <math.h>

namespace nr {

constexpr int kFuseTileX = 64, kFuseTileY = 4;        // a workgroup: 4 waves, one image row of 64 pixels each
constexpr int kFuseMaxSrc = 16;

struct FuseConsistencyParams {
    const float* depth;        // [n][h][w] z-depth, 0 = none
    const float* poses;        // [n][3][4] world -> camera [R|t]
    const float* Ks;           // [n][3][3]
    const float* Ks_inv;       // [n][3][3]
    const int* nn_ids;         // [n][S] source views; -1 or the view itself: an unused slot
    unsigned char* count;      // [n][h][w] consistent slots (may be null, as every output)
    float* fused_depth;        // [n][h][w]
    unsigned* consistent_bits; // [n][h][w] bit s = slot s
    unsigned* occluded_bits;   // [n][h][w]
    int* src_texel;            // [n][S][h][w] vn * w + un where seen, else -1
    int n, h, w, S;
    float tau_px, tau_d;
};

struct FuseParams {
    const float* depth;                // as above
    const float* poses;
    const float* Ks;
    const float* Ks_inv;
    const int* nn_ids;
    const unsigned char* count;        // [n][h][w]: the consistency kernel's outputs
    const float* fused_depth;
    const unsigned* consistent_bits;
    const float* rgb;                  // [n][3][h][w] (may be null with colour)
    unsigned char* taken;              // [n][h][w], zeroed once by the caller (null: no de-duplication)
    unsigned char* emit;               // [h][w]
    float* xyz;                        // [h][w][3]
    float* colour;                     // [h][w][3] (may be null)
    float* normal;                     // [h][w][3] (may be null)
    int n, h, w, S, view, min_views;
    float tau_n;
};

// world point of pixel (px, py) at z-depth d: R^T (K^-1 [px,py,1]^T d - t)
__device__ __forceinline__ void fuse_unproject(const float* __restrict__ Rt, const float* __restrict__ Ki, float px, float py, float d,
                                               float& X, float& Y, float& Z) {
    const float a0 = (Ki[0] * px + Ki[1] * py + Ki[2]) * d - Rt[3];
    const float a1 = (Ki[3] * px + Ki[4] * py + Ki[5]) * d - Rt[7];
    const float a2 = (Ki[6] * px + Ki[7] * py + Ki[8]) * d - Rt[11];
    X = Rt[0] * a0 + Rt[4] * a1 + Rt[8] * a2;
    Y = Rt[1] * a0 + Rt[5] * a1 + Rt[9] * a2;
    Z = Rt[2] * a0 + Rt[6] * a1 + Rt[10] * a2;
}

// Pc = R X + t, q = K Pc -> (u, v) = q.xy / q.z and z = Pc.z
__device__ __forceinline__ void fuse_project(const float* __restrict__ Rt, const float* __restrict__ K, float X, float Y, float Z, float& u, float& v,
                                             float& z) {
    const float c0 = Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[3];
    const float c1 = Rt[4] * X + Rt[5] * Y + Rt[6] * Z + Rt[7];
    const float c2 = Rt[8] * X + Rt[9] * Y + Rt[10] * Z + Rt[11];
    const float q0 = K[0] * c0 + K[1] * c1 + K[2] * c2, q1 = K[3] * c0 + K[4] * c1 + K[5] * c2, q2 = K[6] * c0 + K[7] * c1 + K[8] * c2;
    u = q0 / q2; v = q1 / q2; z = c2;
}

// the nearest texel of world point X in source view j -> vn * w + un, or -1 when X is behind the camera or outside the image (z: its depth there)
__device__ __forceinline__ int fuse_texel(const float* __restrict__ Rt_j, const float* __restrict__ K_j, float X, float Y, float Z, int h, int w,
                                          float& z, float& un, float& vn) {
    float u, v;
    fuse_project(Rt_j, K_j, X, Y, Z, u, v, z);
    un = floorf(u + 0.5f); vn = floorf(v + 0.5f);
    const bool in = z > 0.0f && un >= 0.0f && un < (float)w && vn >= 0.0f && vn < (float)h;       // (false for a NaN)
    return in ? (int)vn * w + (int)un : -1;
}

__device__ __forceinline__ bool fuse_slot_used(int j, int view, int n) { return j >= 0 && j != view && j < n; }

__global__ void __launch_bounds__(kFuseTileX * kFuseTileY) depth_consistency_kernel(FuseConsistencyParams p) {
    const int view = blockIdx.z;
    const int x_raw = (int)blockIdx.x * kFuseTileX + (int)(threadIdx.x % kFuseTileX);
    const int y_raw = (int)blockIdx.y * kFuseTileY + (int)(threadIdx.x / kFuseTileX);
    const bool inside = x_raw < p.w && y_raw < p.h;   // partial tiles: the lane works on the edge pixel, stores nothing
    const int x = x_raw < p.w ? x_raw : p.w - 1, y = y_raw < p.h ? y_raw : p.h - 1;
    const int h = p.h, w = p.w, S = p.S;
    const size_t plane = (size_t)h * w, pix = (size_t)y * w + x;
    const float* __restrict__ Rt_i = p.poses + view * 12;
    const float* __restrict__ K_i = p.Ks + view * 9;
    const float* __restrict__ Ki_i = p.Ks_inv + view * 9;
    const float fx = (float)x, fy = (float)y;
    const float d = p.depth[(size_t)view * plane + pix];
    const bool have = d > 0.0f;
    float X, Y, Z;
    fuse_unproject(Rt_i, Ki_i, fx, fy, d, X, Y, Z);
    const float tau_px2 = p.tau_px * p.tau_px, tau_d = p.tau_d;
    float acc = d;
    int count = 0;
    unsigned cons = 0u, occ = 0u;
    for (int s = 0; s < S; ++s) {
        const int j = p.nn_ids[view * S + s];
        int texel = -1;
        if (fuse_slot_used(j, view, p.n)) {           // (uniform: j is the same in every lane)
            const float* __restrict__ Rt_j = p.poses + j * 12;
            float z, un, vn;
            const int t = fuse_texel(Rt_j, p.Ks + j * 9, X, Y, Z, h, w, z, un, vn);
            const bool in = have && t >= 0;
            const float dj = in ? p.depth[(size_t)j * plane + (size_t)t] : 0.0f;
            const bool seen = in && dj > 0.0f;
            float Xs, Ys, Zs, u2, v2, qz;
            fuse_unproject(Rt_j, p.Ks_inv + j * 9, un, vn, dj, Xs, Ys, Zs);
            fuse_project(Rt_i, K_i, Xs, Ys, Zs, u2, v2, qz);
            const float du = u2 - fx, dv = v2 - fy;
            const float e_px2 = du * du + dv * dv;
            const float e_d = fabsf(qz - d) / d;
            const bool ok = seen && qz > 0.0f && e_px2 < tau_px2 && e_d < tau_d;
            const bool hidden = seen && !ok && (z - dj) / dj > tau_d;
            if (ok) { acc = acc + qz; count = count + 1; cons |= 1u << s; }
            if (hidden) occ |= 1u << s;
            texel = seen ? t : -1;
        }
        if (inside && p.src_texel) p.src_texel[((size_t)view * S + s) * plane + pix] = texel;
    }
    if (!inside) return;
    const size_t o = (size_t)view * plane + pix;
    if (p.count) p.count[o] = (unsigned char)count;
    if (p.fused_depth) p.fused_depth[o] = have ? acc / (float)(1 + count) : 0.0f;
    if (p.consistent_bits) p.consistent_bits[o] = cons;
    if (p.occluded_bits) p.occluded_bits[o] = occ;
}

// camera-space point of pixel (px, py) from the fused depth
__device__ __forceinline__ void fuse_cam_point(const float* __restrict__ Ki, float px, float py, float fd, float& a, float& b, float& c) {
    a = (Ki[0] * px + Ki[1] * py + Ki[2]) * fd;
    b = (Ki[3] * px + Ki[4] * py + Ki[5]) * fd;
    c = (Ki[6] * px + Ki[7] * py + Ki[8]) * fd;
}

// One view per launch, the views in ascending order on one stream.  A pixel is kept where count >= min_views and emitted where it is kept and
// its byte of `taken` is 0; an emitted pixel stores the constant 1 into taken[j][texel] of every consistent source - other views' masks only
// (a slot never names the view itself), so a launch never writes the mask it reads and the result does not depend on scheduling.
__global__ void __launch_bounds__(kFuseTileX * kFuseTileY) fuse_view_kernel(FuseParams p) {
    const int view = p.view;
    const int x_raw = (int)blockIdx.x * kFuseTileX + (int)(threadIdx.x % kFuseTileX);
    const int y_raw = (int)blockIdx.y * kFuseTileY + (int)(threadIdx.x / kFuseTileX);
    const bool inside = x_raw < p.w && y_raw < p.h;
    const int x = x_raw < p.w ? x_raw : p.w - 1, y = y_raw < p.h ? y_raw : p.h - 1;
    const int h = p.h, w = p.w, S = p.S, min_views = p.min_views;
    const size_t plane = (size_t)h * w, pix = (size_t)y * w + x;
    const float* __restrict__ Rt_i = p.poses + view * 12;
    const float* __restrict__ Ki_i = p.Ks_inv + view * 9;
    const unsigned char* __restrict__ cnt = p.count + (size_t)view * plane;
    const float* __restrict__ fdm = p.fused_depth + (size_t)view * plane;
    const float fx = (float)x, fy = (float)y;
    const int count = cnt[pix];
    const float fd = fdm[pix];
    const bool kept = count >= min_views;
    const bool emitted = kept && (p.taken == nullptr || p.taken[(size_t)view * plane + pix] == 0);
    const unsigned cons = p.consistent_bits[(size_t)view * plane + pix];
    const float d = p.depth[(size_t)view * plane + pix];
    float X, Y, Z;
    fuse_unproject(Rt_i, Ki_i, fx, fy, d, X, Y, Z);
    float cr = 0.0f, cg = 0.0f, cb = 0.0f;
    if (p.colour) {
        const float* __restrict__ c = p.rgb + (size_t)view * 3 * plane + pix;
        cr = c[0]; cg = c[plane]; cb = c[2 * plane];
    }
    int used = 0;
    for (int s = 0; s < S; ++s) {
        const int j = p.nn_ids[view * S + s];
        if (!fuse_slot_used(j, view, p.n)) continue;  // (uniform)
        float z, un, vn;
        const int t = fuse_texel(p.poses + j * 12, p.Ks + j * 9, X, Y, Z, h, w, z, un, vn);
        const bool on = emitted && inside && ((cons >> s) & 1u) != 0u && t >= 0;
        if (on) {
            if (p.taken) p.taken[(size_t)j * plane + (size_t)t] = 1;
            if (p.colour) {
                const float* __restrict__ c = p.rgb + (size_t)j * 3 * plane + (size_t)t;
                cr = cr + c[0]; cg = cg + c[plane]; cb = cb + c[2 * plane];
            }
            used = used + 1;
        }
    }
    // the normal: differences of camera-space points along x and y over the neighbours that are kept and close in depth
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    float a0, a1, a2;
    fuse_cam_point(Ki_i, fx, fy, fd, a0, a1, a2);
    if (p.normal) {
        const float lim = p.tau_n * fd;
        float dxv[3], dyv[3];
        bool okx, oky;
        {
            const bool hl = x > 0, hr = x + 1 < w;
            const size_t il = hl ? pix - 1 : pix, ir = hr ? pix + 1 : pix;
            const float fl = fdm[il], fr = fdm[ir];
            const bool ql = hl && cnt[il] >= min_views && fabsf(fl - fd) < lim, qr = hr && cnt[ir] >= min_views && fabsf(fr - fd) < lim;
            float l0, l1, l2, r0, r1, r2;
            fuse_cam_point(Ki_i, fx - 1.0f, fy, fl, l0, l1, l2);
            fuse_cam_point(Ki_i, fx + 1.0f, fy, fr, r0, r1, r2);
            if (!ql) { l0 = a0; l1 = a1; l2 = a2; }
            if (!qr) { r0 = a0; r1 = a1; r2 = a2; }
            dxv[0] = r0 - l0; dxv[1] = r1 - l1; dxv[2] = r2 - l2;
            okx = ql || qr;
        }
        {
            const bool hu = y > 0, hd = y + 1 < h;
            const size_t iu = hu ? pix - w : pix, id = hd ? pix + w : pix;
            const float fu = fdm[iu], fw = fdm[id];
            const bool qu = hu && cnt[iu] >= min_views && fabsf(fu - fd) < lim, qd = hd && cnt[id] >= min_views && fabsf(fw - fd) < lim;
            float u0, u1, u2, b0, b1, b2;
            fuse_cam_point(Ki_i, fx, fy - 1.0f, fu, u0, u1, u2);
            fuse_cam_point(Ki_i, fx, fy + 1.0f, fw, b0, b1, b2);
            if (!qu) { u0 = a0; u1 = a1; u2 = a2; }
            if (!qd) { b0 = a0; b1 = a1; b2 = a2; }
            dyv[0] = b0 - u0; dyv[1] = b1 - u1; dyv[2] = b2 - u2;
            oky = qu || qd;
        }
        float c0 = dxv[1] * dyv[2] - dxv[2] * dyv[1], c1 = dxv[2] * dyv[0] - dxv[0] * dyv[2], c2 = dxv[0] * dyv[1] - dxv[1] * dyv[0];
        const float len2 = c0 * c0 + c1 * c1 + c2 * c2;
        if (okx && oky && len2 > 0.0f) {
            const float len = sqrtf(len2);
            if (c0 * a0 + c1 * a1 + c2 * a2 > 0.0f) { c0 = -c0; c1 = -c1; c2 = -c2; }        // towards the camera
            c0 = c0 / len; c1 = c1 / len; c2 = c2 / len;
            nx = Rt_i[0] * c0 + Rt_i[4] * c1 + Rt_i[8] * c2;
            ny = Rt_i[1] * c0 + Rt_i[5] * c1 + Rt_i[9] * c2;
            nz = Rt_i[2] * c0 + Rt_i[6] * c1 + Rt_i[10] * c2;
        }
    }
    if (!inside) return;
    p.emit[pix] = emitted ? 1 : 0;
    // what is not emitted is stored as zeros: the outputs of two runs are the same bytes everywhere
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (emitted) fuse_unproject(Rt_i, Ki_i, fx, fy, fd, px, py, pz);
    p.xyz[pix * 3] = px; p.xyz[pix * 3 + 1] = py; p.xyz[pix * 3 + 2] = pz;
    if (p.colour) {
        const float m = (float)(1 + used);
        p.colour[pix * 3] = emitted ? cr / m : 0.0f; p.colour[pix * 3 + 1] = emitted ? cg / m : 0.0f; p.colour[pix * 3 + 2] = emitted ? cb / m : 0.0f;
    }
    if (p.normal) { p.normal[pix * 3] = emitted ? nx : 0.0f; p.normal[pix * 3 + 1] = emitted ? ny : 0.0f; p.normal[pix * 3 + 2] = emitted ? nz : 0.0f; }
}

}  // namespace nr
