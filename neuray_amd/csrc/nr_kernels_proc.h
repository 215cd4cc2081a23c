// Procedural 3-D scenes (neuray_amd/procedural.py): a ray caster for spheres and axis-aligned boxes that renders
// posed ground truth - colour, exact z-depth, mask, primitive id - for the kernels next to it to train on.  One thread per pixel, one
// wave per 64 neighbouring pixels of a row (coalesced stores along x); the scene array is read at wave-uniform addresses only (the
// primitive loop and the shading loop both run over the primitive index, the same in every lane), so it arrives through scalar loads.
// The arithmetic is procedural.render_numpy's, operation by operation, in fp32 without contraction (no fmaf anywhere in this file):
// what differs from numpy's float32 evaluation is the device library's sinf / powf.
//
// scene [kProcHeader + n_prims * kProcPrim] floats:
//   header: 0 n_prims | 1..3 light direction L (unit) | 4 ambient | 5..7 background colour | 8..15 zero
//   primitive: 0 kind (0 sphere, 1 box) | 1..3 centre p | 4..6 half-extents e (sphere: e[0] = radius) | 7..9 base colour b | 10 specular
//              strength s | 11 exponent m | 12 + 7 w .. : wave w = (k[3] in cycles per unit, phase, a[3]), w = 0..3 | 40..47 zero
#pragma once
#include "nr_platform.h"

#include <math.h>

namespace nr {

constexpr int kProcHeader = 16, kProcPrim = 48, kProcMaxPrims = 32, kProcWaves = 4;
constexpr int kProcTileX = 64, kProcTileY = 4;        // a workgroup: 4 waves, one image row of 64 pixels each

struct ProcParams {
    const float* scene;        // see above
    const float* poses;        // [n][3][4] world -> camera [R|t]
    const float* Ks_inv;       // [n][3][3]
    float* rgb;                // [n][3][h][w]
    float* depth;              // [n][h][w] z-depth of the centre ray, 0 on a miss (may be null)
    unsigned char* mask;       // [n][h][w] (may be null)
    signed char* prim;         // [n][h][w] primitive index, -1 on a miss (may be null)
    int n_prims, n, h, w, ss;
};

struct ProcRay { float cx, cy, cz, dx, dy, dz; };

// one axis of the slab method.  d == 0 is its own branch: inside the slab the axis does not bound the ray, outside there is no hit
__device__ __forceinline__ void proc_slab(float o, float d, float e, int ax, float& t_in, float& t_out, int& axis, bool& ok) {
    if (d == 0.0f) {
        if (fabsf(o) > e) ok = false;
    } else {
        const float t1 = (-e - o) / d, t2 = (e - o) / d;
        const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
        if (lo > t_in) { t_in = lo; axis = ax; }
        t_out = fminf(t_out, hi);
    }
}

// nearest hit along the ray over all primitives (uniform trip count; the lower index wins a tie) -> primitive index or -1
__device__ __forceinline__ int proc_cast(const float* __restrict__ sc, int n_prims, const ProcRay& r, float& t_hit, int& axis_hit) {
    float best = INFINITY;
    int bi = -1, bax = 0;
    const float A = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    for (int i = 0; i < n_prims; ++i) {
        const float* __restrict__ P = sc + kProcHeader + i * kProcPrim;
        const float ox = r.cx - P[1], oy = r.cy - P[2], oz = r.cz - P[3];
        float t;
        int ax = 0;
        bool hit;
        if (P[0] == 0.0f) {                           // sphere: the smaller root of |c + t d - p|^2 = r^2
            const float rad = P[4];
            const float B = ox * r.dx + oy * r.dy + oz * r.dz;
            const float Cc = (ox * ox + oy * oy + oz * oz) - rad * rad;
            const float disc = B * B - A * Cc;
            t = (-B - sqrtf(fmaxf(disc, 0.0f))) / A;
            hit = disc >= 0.0f && t > 0.0f;
        } else {                                      // box: the entry of the slab method
            float t_in = -INFINITY, t_out = INFINITY;
            bool ok = true;
            proc_slab(ox, r.dx, P[4], 0, t_in, t_out, ax, ok);
            proc_slab(oy, r.dy, P[5], 1, t_in, t_out, ax, ok);
            proc_slab(oz, r.dz, P[6], 2, t_in, t_out, ax, ok);
            t = t_in;
            hit = ok && t_in > 0.0f && t_in <= t_out;
        }
        if (hit && t < best) { best = t; bi = i; bax = ax; }
    }
    t_hit = best;
    axis_hit = bax;
    return bi;
}

__device__ __forceinline__ float proc_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// colour of the hit on primitive P at ray parameter t (axis: the box face's axis)
__device__ __forceinline__ void proc_shade(const float* __restrict__ sc, const float* __restrict__ P, const ProcRay& r, float t, int axis,
                                           float& cr, float& cg, float& cb) {
    const float Lx = sc[1], Ly = sc[2], Lz = sc[3], amb = sc[4];
    const float qx = (r.cx + t * r.dx) - P[1], qy = (r.cy + t * r.dy) - P[2], qz = (r.cz + t * r.dz) - P[3];
    float nx, ny, nz;
    if (P[0] == 0.0f) {
        const float rad = P[4];
        nx = qx / rad; ny = qy / rad; nz = qz / rad;
    } else {                                          // the face the ray entered through, against the ray
        const float da = axis == 0 ? r.dx : (axis == 1 ? r.dy : r.dz);
        const float s = da > 0.0f ? -1.0f : 1.0f;
        nx = axis == 0 ? s : 0.0f; ny = axis == 1 ? s : 0.0f; nz = axis == 2 ? s : 0.0f;
    }
    float ar = P[7], ag = P[8], ab = P[9];            // albedo: object space, the same from every view
    NR_PRAGMA_UNROLL
    for (int w = 0; w < kProcWaves; ++w) {
        const float* __restrict__ W = P + 12 + 7 * w;
        const float ph = 6.28318530717958647692f * (W[0] * qx + W[1] * qy + W[2] * qz) + W[3];
        const float s = sinf(ph);
        ar = ar + W[4] * s; ag = ag + W[5] * s; ab = ab + W[6] * s;
    }
    ar = proc_clamp01(ar); ag = proc_clamp01(ag); ab = proc_clamp01(ab);
    const float dn = sqrtf(r.dx * r.dx + r.dy * r.dy + r.dz * r.dz);
    const float hx = Lx + (-r.dx) / dn, hy = Ly + (-r.dy) / dn, hz = Lz + (-r.dz) / dn;      // L + v, v = -d / |d|
    const float hn = sqrtf(hx * hx + hy * hy + hz * hz);
    const float ndl = fmaxf(0.0f, nx * Lx + ny * Ly + nz * Lz);
    const float ndh = hn > 0.0f ? fmaxf(0.0f, (nx * hx + ny * hy + nz * hz) / hn) : 0.0f;
    const float shade = amb + (1.0f - amb) * ndl;
    const float spec = P[10] * powf(ndh, P[11]);      // the view-dependent part
    cr = proc_clamp01(ar * shade + spec); cg = proc_clamp01(ag * shade + spec); cb = proc_clamp01(ab * shade + spec);
}

__global__ void __launch_bounds__(kProcTileX * kProcTileY) procedural_render_kernel(ProcParams p) {
    const float* __restrict__ sc = p.scene;
    const int view = blockIdx.z;
    const int x_raw = (int)blockIdx.x * kProcTileX + (int)(threadIdx.x % kProcTileX);
    const int y_raw = (int)blockIdx.y * kProcTileY + (int)(threadIdx.x / kProcTileX);
    const bool inside = x_raw < p.w && y_raw < p.h;   // partial tiles at the right / bottom edge: the lane works on the edge pixel, stores nothing
    const int x = x_raw < p.w ? x_raw : p.w - 1, y = y_raw < p.h ? y_raw : p.h - 1;
    const float* __restrict__ Rt = p.poses + view * 12;
    const float* __restrict__ Ki = p.Ks_inv + view * 9;
    ProcRay r;
    r.cx = -(Rt[0] * Rt[3] + Rt[4] * Rt[7] + Rt[8] * Rt[11]);        // c = -R^T t
    r.cy = -(Rt[1] * Rt[3] + Rt[5] * Rt[7] + Rt[9] * Rt[11]);
    r.cz = -(Rt[2] * Rt[3] + Rt[6] * Rt[7] + Rt[10] * Rt[11]);
    auto aim = [&](float px, float py) {                              // d = R^T K^-1 [px, py, 1]^T, un-normalised: t is the z-depth
        const float c0 = Ki[0] * px + Ki[1] * py + Ki[2], c1 = Ki[3] * px + Ki[4] * py + Ki[5], c2 = Ki[6] * px + Ki[7] * py + Ki[8];
        r.dx = Rt[0] * c0 + Rt[4] * c1 + Rt[8] * c2;
        r.dy = Rt[1] * c0 + Rt[5] * c1 + Rt[9] * c2;
        r.dz = Rt[2] * c0 + Rt[6] * c1 + Rt[10] * c2;
    };
    const int ss = p.ss, n_prims = p.n_prims;
    const bool want_centre = p.depth != nullptr || p.mask != nullptr || p.prim != nullptr;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, t_c = 0.0f;
    int prim_c = -1;
    bool have_centre = false;
    for (int j = 0; j < ss; ++j) {
        for (int i = 0; i < ss; ++i) {
            const float offx = ((float)i + 0.5f) / (float)ss - 0.5f, offy = ((float)j + 0.5f) / (float)ss - 0.5f;
            aim((float)x + offx, (float)y + offy);
            float t;
            int axis;
            const int hit = proc_cast(sc, n_prims, r, t, axis);
            float cr = sc[5], cg = sc[6], cb = sc[7];                 // a miss: the background
            for (int k = 0; k < n_prims; ++k)                          // (uniform index: the primitive's floats are the same address in every lane)
                if (hit == k) proc_shade(sc, sc + kProcHeader + k * kProcPrim, r, t, axis, cr, cg, cb);
            acc_r = acc_r + cr; acc_g = acc_g + cg; acc_b = acc_b + cb;
            if (2 * i + 1 == ss && 2 * j + 1 == ss) { prim_c = hit; t_c = t; have_centre = true; }        // odd ss: the middle sub-ray is the centre ray
        }
    }
    if (want_centre && !have_centre) {
        int axis;
        aim((float)x, (float)y);
        prim_c = proc_cast(sc, n_prims, r, t_c, axis);
    }
    if (!inside) return;
    const float cnt = (float)(ss * ss);
    const size_t plane = (size_t)p.h * p.w, pix = (size_t)y * p.w + x;
    float* rgb = p.rgb + (size_t)view * 3 * plane + pix;
    rgb[0] = acc_r / cnt; rgb[plane] = acc_g / cnt; rgb[2 * plane] = acc_b / cnt;
    if (p.depth) p.depth[(size_t)view * plane + pix] = prim_c >= 0 ? t_c : 0.0f;
    if (p.mask) p.mask[(size_t)view * plane + pix] = prim_c >= 0 ? 1 : 0;
    if (p.prim) p.prim[(size_t)view * plane + pix] = (signed char)prim_c;
}

}  // namespace nr
