// Mesh export (neuray_amd/mesh.py): the volumetric fusion of posed depth maps into a truncated signed distance
// field and the extraction of its zero surface by naive surface nets.  The layout of nr_kernels_fuse.h with a lattice in place of an image:
// one thread per lattice point (or cell), one wave per 64 consecutive x, four y per workgroup, (y tile, z) from a linear block index; every
// state array is read and written coalesced.  The loop over the views has the same trip count in every lane, so every pose / K entry is read
// at a wave-uniform address and arrives through scalar loads.  The arithmetic is mesh.integrate_numpy's / surface_nets_numpy's, operation by
// operation, in fp32 without contraction (no fmaf anywhere in this file).  No LDS, no atomics: every thread owns its words of the outputs.
//
// Lattice point (ix, iy, iz) sits at origin + (ix, iy, iz) * vs; arrays are [nz][ny][nx], colour planar [3][nz][ny][nx].  The state is sums:
// Tsum, W, Csum[3], Cw.  For lattice point p and view i, the views in ascending order:
//   Pc = R_i p + t_i, z = Pc.z, q = K_i Pc, (u, v) = q.xy / q.z, (un, vn) = floor((u, v) + 0.5)          (fuse_texel: the NEAREST texel)
//   skip unless z > 0, the texel inside the image, d = D_i[vn][un] > 0;  sdf = d - z;  skip if sdf < -trunc
//   Tsum += min(sdf / trunc, 1), W += 1;  if sdf <= trunc: Csum[c] += rgb_i[c][vn][un], Cw += 1
// Surface nets: f = Tsum / W, a lattice point is inside where f < 0, a cell (its 8 corners (c + d), d in {0,1}^3) is valid where every corner
// has W >= min_weight and active where it is valid and its corners are not all on one side.
#pragma once
#include "nr_kernels_fuse.h"

namespace nr {

constexpr int kTsdfTileX = kFuseTileX, kTsdfTileY = kFuseTileY;

struct TsdfIntegrateParams {
    const float* depth;        // [n][h][w] z-depth, 0 = none
    const float* rgb;          // [n][3][h][w] (null: no colour)
    const float* poses;        // [n][3][4] world -> camera [R|t]
    const float* Ks;           // [n][3][3]
    float* tsum;               // [nz][ny][nx]
    float* wsum;               // [nz][ny][nx]
    float* csum;               // [3][nz][ny][nx] (null: no colour)
    float* cw;                 // [nz][ny][nx]
    float ox, oy, oz, vs, trunc;
    int nx, ny, nz, h, w, v0, v1, bx, by;
};

struct SurfaceCellsParams {
    const float* tsum;
    const float* wsum;
    unsigned char* cells;      // [nz-1][ny-1][nx-1]
    int nx, ny, nz, bx, by;
    float min_weight;
};

struct SurfaceEmitParams {
    const float* tsum;
    const float* wsum;
    const float* csum;         // (null: grey)
    const float* cw;
    const unsigned char* cells;
    const long long* vert_offset;      // [cells] exclusive prefix sum of bit 0
    const long long* quad_offset;      // [cells] exclusive prefix sum of the number of quad bits
    float* vertices;           // [m][3]
    float* normals;            // [m][3]
    float* colours;            // [m][3]
    int* faces;                // [2 quads][3]
    size_t n_vertices, n_quads;        // the sizes of the outputs: a slot past them is not written
    float ox, oy, oz, vs;
    int nx, ny, nz, bx, by;
};

// the lattice (or cell) coordinates of this thread in a box of (ex, ey, ez) elements: partial tiles work on the edge element and store nothing
__device__ __forceinline__ bool tsdf_coords(int bx, int by, int ex, int ey, int& x, int& y, int& z) {
    const int b = (int)blockIdx.x;
    const int bxi = b % bx, t = b / bx;
    const int byi = t % by;
    z = t / by;
    const int x_raw = bxi * kTsdfTileX + (int)(threadIdx.x % kTsdfTileX), y_raw = byi * kTsdfTileY + (int)(threadIdx.x / kTsdfTileX);
    x = x_raw < ex ? x_raw : ex - 1;
    y = y_raw < ey ? y_raw : ey - 1;
    return x_raw < ex && y_raw < ey;
}

__global__ void __launch_bounds__(kTsdfTileX * kTsdfTileY) tsdf_integrate_kernel(TsdfIntegrateParams p) {
    int x, y, z;
    const bool inside = tsdf_coords(p.bx, p.by, p.nx, p.ny, x, y, z);
    const int h = p.h, w = p.w;
    const size_t plane = (size_t)h * w, vol = (size_t)p.nx * p.ny * p.nz, idx = ((size_t)z * p.ny + y) * p.nx + x;
    const float X = p.ox + (float)x * p.vs, Y = p.oy + (float)y * p.vs, Z = p.oz + (float)z * p.vs;
    const float trunc = p.trunc;
    const bool colour = p.csum != nullptr;
    float ts = p.tsum[idx], ws = p.wsum[idx];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, cw = 0.0f;
    if (colour) { c0 = p.csum[idx]; c1 = p.csum[vol + idx]; c2 = p.csum[2 * vol + idx]; cw = p.cw[idx]; }
    for (int i = p.v0; i < p.v1; ++i) {               // (uniform: the camera of view i is the same address in every lane)
        float zc, un, vn;
        const int t = fuse_texel(p.poses + (size_t)i * 12, p.Ks + (size_t)i * 9, X, Y, Z, h, w, zc, un, vn);
        if (t < 0) continue;                          // (a wave none of whose lanes projects into the view skips the gather altogether)
        const float d = p.depth[(size_t)i * plane + (size_t)t];
        const float sdf = d - zc;
        if (!(d > 0.0f) || sdf < -trunc) continue;
        ts = ts + fminf(sdf / trunc, 1.0f);
        ws = ws + 1.0f;
        if (colour && sdf <= trunc) {
            const float* __restrict__ c = p.rgb + (size_t)i * 3 * plane + (size_t)t;
            c0 = c0 + c[0]; c1 = c1 + c[plane]; c2 = c2 + c[2 * plane];
            cw = cw + 1.0f;
        }
    }
    if (!inside) return;
    p.tsum[idx] = ts; p.wsum[idx] = ws;
    if (colour) { p.csum[idx] = c0; p.csum[vol + idx] = c1; p.csum[2 * vol + idx] = c2; p.cw[idx] = cw; }
}

// bit (dz * 9 + dy * 3 + dx) of the 27-point neighbourhood mask, d in {0, 1, 2} for the offsets {-1, 0, +1}
constexpr unsigned tsdf_cell_mask(int a, int b, int c) {       // the 8 corners of the cell at offset (a, b, c) in {-1, 0}^3
    unsigned m = 0u;
    for (int dz = 0; dz < 2; ++dz)
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) m |= 1u << ((c + 1 + dz) * 9 + (b + 1 + dy) * 3 + (a + 1 + dx));
    return m;
}

// One byte per cell: bit 0 active; bits 1..3: the cell emits the quad of the lattice edge from its corner (cx, cy, cz) towards +x / +y / +z -
// the edge's ends differ in `inside` and the four cells around it exist and are valid (for the edge along axis a, (a, b, c) cyclic: the cells
// at offsets (b - 1, c - 1), (b, c - 1), (b, c), (b - 1, c)).  A cell that does not exist has a corner outside the lattice: never `ok`.
__global__ void __launch_bounds__(kTsdfTileX * kTsdfTileY) surface_cells_kernel(SurfaceCellsParams p) {
    int cx, cy, cz;
    const bool inside = tsdf_coords(p.bx, p.by, p.nx - 1, p.ny - 1, cx, cy, cz);
    const int nx = p.nx, ny = p.ny;
    unsigned ok = 0u;
    NR_PRAGMA_UNROLL
    for (int dz = -1; dz < 2; ++dz)
        NR_PRAGMA_UNROLL
        for (int dy = -1; dy < 2; ++dy)
            NR_PRAGMA_UNROLL
            for (int dx = -1; dx < 2; ++dx) {
                const int ix = cx + dx, iy = cy + dy, iz = cz + dz;          // (never past the upper end: cx + 1 <= nx - 1)
                if (ix >= 0 && iy >= 0 && iz >= 0 && p.wsum[((size_t)iz * ny + iy) * nx + ix] >= p.min_weight)
                    ok |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
            }
    unsigned in = 0u;                                 // bit (dz * 4 + dy * 2 + dx): the corner is inside
    NR_PRAGMA_UNROLL
    for (int k = 0; k < 8; ++k) {
        const size_t i = ((size_t)(cz + (k >> 2)) * ny + (cy + ((k >> 1) & 1))) * nx + (cx + (k & 1));
        if (p.tsum[i] / p.wsum[i] < 0.0f) in |= 1u << k;
    }
    auto valid = [&](unsigned m) { return (ok & m) == m; };
    const bool own = valid(tsdf_cell_mask(0, 0, 0));
    unsigned bits = own && in != 0u && in != 0xffu ? 1u : 0u;
    const bool lo = (in & 1u) != 0u;
    if (own) {
        if (lo != ((in & 2u) != 0u) && valid(tsdf_cell_mask(0, -1, -1)) && valid(tsdf_cell_mask(0, 0, -1)) && valid(tsdf_cell_mask(0, -1, 0))) bits |= 2u;
        if (lo != ((in & 4u) != 0u) && valid(tsdf_cell_mask(-1, 0, -1)) && valid(tsdf_cell_mask(0, 0, -1)) && valid(tsdf_cell_mask(-1, 0, 0))) bits |= 4u;
        if (lo != ((in & 16u) != 0u) && valid(tsdf_cell_mask(-1, -1, 0)) && valid(tsdf_cell_mask(0, -1, 0)) && valid(tsdf_cell_mask(-1, 0, 0))) bits |= 8u;
    }
    if (!inside) return;
    p.cells[((size_t)cz * (ny - 1) + cy) * (nx - 1) + cx] = (unsigned char)bits;
}

// Per active cell, into its slot vert_offset[cell]: the vertex origin + (cell + m) * vs, m the mean of the crossing points t = f_lo / (f_lo -
// f_hi) of the cell's edges whose ends differ in `inside` (the four x-edges, then y, then z, each with the other two offsets - in ascending
// axis order - running 00, 10, 01, 11); the normal: the normalised sums of the forward differences of f over the four edges per axis (towards
// free space, zero where the vector is zero); the colour: sum of Csum / sum of Cw over the 8 corners in corner order, 0.5 where that is 0 / 0 or
// there is no colour state.  Per quad bit, into slot quad_offset[cell] + (the number of lower quad bits): the triangles (v0, v1, v2) and (v0,
// v2, v3) of the quad of the four cells around the edge, in the order above where the edge's low end is inside, reversed otherwise.
__global__ void __launch_bounds__(kTsdfTileX * kTsdfTileY) surface_emit_kernel(SurfaceEmitParams p) {
    int cx, cy, cz;
    if (!tsdf_coords(p.bx, p.by, p.nx - 1, p.ny - 1, cx, cy, cz)) return;
    const int nx = p.nx, ny = p.ny, mx = nx - 1, my = ny - 1;
    const size_t cell = ((size_t)cz * my + cy) * mx + cx;
    const unsigned bits = p.cells[cell];
    if ((bits & 1u) == 0u) return;
    const size_t vol = (size_t)nx * ny * p.nz;
    float f[8];
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
    NR_PRAGMA_UNROLL
    for (int k = 0; k < 8; ++k) {
        const size_t i = ((size_t)(cz + (k >> 2)) * ny + (cy + ((k >> 1) & 1))) * nx + (cx + (k & 1));
        f[k] = p.tsum[i] / p.wsum[i];
        if (p.csum) { s0 = s0 + p.csum[i]; s1 = s1 + p.csum[vol + i]; s2 = s2 + p.csum[2 * vol + i]; sw = sw + p.cw[i]; }
    }
    float ax = 0.0f, ay = 0.0f, az = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    int crossings = 0;
    NR_PRAGMA_UNROLL
    for (int axis = 0; axis < 3; ++axis)
        NR_PRAGMA_UNROLL
        for (int e = 0; e < 4; ++e) {
            const int o1 = e & 1, o2 = e >> 1;          // the other two axes, ascending
            const int dx = axis == 0 ? 0 : o1, dy = axis == 1 ? 0 : (axis == 0 ? o1 : o2), dz = axis == 2 ? 0 : o2;
            const int klo = dz * 4 + dy * 2 + dx, khi = klo + (1 << axis);
            const float flo = f[klo], fhi = f[khi];
            const float diff = fhi - flo;
            if (axis == 0) gx = gx + diff; else if (axis == 1) gy = gy + diff; else gz = gz + diff;
            if ((flo < 0.0f) != (fhi < 0.0f)) {
                const float t = flo / (flo - fhi);
                ax = ax + (axis == 0 ? t : (float)dx); ay = ay + (axis == 1 ? t : (float)dy); az = az + (axis == 2 ? t : (float)dz);
                crossings = crossings + 1;
            }
        }
    const float cnt = (float)crossings;
    const size_t v = (size_t)p.vert_offset[cell];
    if (v >= p.n_vertices) return;
    p.vertices[v * 3] = p.ox + ((float)cx + ax / cnt) * p.vs;
    p.vertices[v * 3 + 1] = p.oy + ((float)cy + ay / cnt) * p.vs;
    p.vertices[v * 3 + 2] = p.oz + ((float)cz + az / cnt) * p.vs;
    const float len2 = gx * gx + gy * gy + gz * gz;
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    if (len2 > 0.0f) { const float len = sqrtf(len2); n0 = gx / len; n1 = gy / len; n2 = gz / len; }
    p.normals[v * 3] = n0; p.normals[v * 3 + 1] = n1; p.normals[v * 3 + 2] = n2;
    const bool grey = !(sw > 0.0f);
    p.colours[v * 3] = grey ? 0.5f : s0 / sw; p.colours[v * 3 + 1] = grey ? 0.5f : s1 / sw; p.colours[v * 3 + 2] = grey ? 0.5f : s2 / sw;
    if ((bits & 14u) == 0u) return;
    size_t q = (size_t)p.quad_offset[cell];
    const bool lo = f[0] < 0.0f;
    const long long sx = 1, sy = mx, sz = (long long)mx * my;          // cell strides
    NR_PRAGMA_UNROLL
    for (int axis = 0; axis < 3; ++axis) {
        if ((bits & (2u << axis)) == 0u || q >= p.n_quads) continue;
        const long long sb = axis == 0 ? sy : (axis == 1 ? sz : sx), sc = axis == 0 ? sz : (axis == 1 ? sx : sy);
        const long long cA = (long long)cell - sb - sc, cB = (long long)cell - sc, cC = (long long)cell, cD = (long long)cell - sb;
        const int v0 = (int)p.vert_offset[lo ? cA : cD], v1 = (int)p.vert_offset[lo ? cB : cC];
        const int v2 = (int)p.vert_offset[lo ? cC : cB], v3 = (int)p.vert_offset[lo ? cD : cA];
        int* __restrict__ o = p.faces + q * 6;
        o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v0; o[4] = v2; o[5] = v3;
        q = q + 1;
    }
}

}  // namespace nr
