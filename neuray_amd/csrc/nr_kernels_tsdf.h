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
//
// Ray casting (mesh.raycast_numpy): per view and pixel the first zero crossing of the field along the pixel's ray.
//   field: f = Tsum / W in float32, NaN ("unknown") where W < min_weight - one elementwise pass of the caller, not of these kernels.  NaN
//     is exact here: the library is built without any fast-math flag, so x == x is false exactly for NaN and NaN propagates through + - *.
//   ray of pixel (x, y) of view i (pixel centres at integers): the 12 floats M = R^T K^-1 (row-major), c = -R^T t, made in float64 and
//     rounded; d[a] = (M[a][0] * x + M[a][1] * y) + M[a][2]; the point at z-depth s is c + s d; in lattice units g[a](s) = g0[a] + s * gd[a]
//     with g0[a] = (c[a] - origin[a]) / vs and gd[a] = d[a] / vs.
//   interval: [s_in, s_out] starts as [near, far] (depth_range, default [0, inf)); per axis a with hi = n[a] - 1: if gd[a] == 0 the ray is
//     empty where g0[a] < 0 or g0[a] > hi, else t1 = (0 - g0[a]) / gd[a], t2 = (hi - g0[a]) / gd[a], s_in = max(s_in, min(t1, t2)), s_out =
//     min(s_out, max(t1, t2)).  Empty unless s_in <= s_out: status 0.
//   samples: ds = (step * vs) / sqrt((d0 d0 + d1 d1) + d2 d2) (a ray without 0 < ds < inf is empty); s_k = s_in + (float)k * ds for k = 0 ..
//     floor(min((s_out - s_in) / ds, 2^22)).
//   value at s: cell[a] = clamp(floor(g[a]), 0, n[a] - 2), t[a] = g[a] - cell[a]; with the corners c_j, j = dz * 4 + dy * 2 + dx, and
//     lerp(p, q, t) = p + t * (q - p): x first, a_0..3 = lerp(c_0, c_1), lerp(c_2, c_3), lerp(c_4, c_5), lerp(c_6, c_7) at t[0]; then y,
//     b_0 = lerp(a_0, a_1), b_1 = lerp(a_2, a_3) at t[1]; then z, lerp(b_0, b_1) at t[2].  NaN (unknown) if any corner is.
//   first crossing: the first k whose samples k - 1 and k are both known (and both evaluated) with (f_{k-1} < 0) != (f_k < 0).  f_k < 0:
//     status 1, depth = s_{k-1} + ds * (f_{k-1} / (f_{k-1} - f_k)); otherwise status 2 (the surface from behind), depth 0.  The ray ends
//     there.  No crossing: status 0, depth 0.
//   at a hit: the cell and t of g(depth) where all 8 of its corners are known, else those of sample k.  Normal: the gradient of the
//     trilinear interpolant there - per axis the four corner differences along it (the other two offsets, in ascending axis order, running
//     00, 10, 01, 11), lerped over the lower then the higher of the other two axes - divided by its length (zero where that is zero).
//     Colour: the same trilinear combination of Csum[c] over that of Cw; 0.5 where that is not positive or there is no colour state.
//   block skipping: `blocks` holds one byte per block of 8 x 8 x 8 cells, non-zero where a cell of the block or within one cell of it is
//     active (surface_blocks_kernel).  A sample whose cell lies in an unflagged block is not evaluated and counts as unknown; k then moves
//     to kn = max(k + 1, floor(clamp((s_exit - s_in) / ds, 0, kmax)) + 1), s_exit the smallest over the axes with gd[a] != 0 of ((gd[a] > 0 ?
//     8 (b[a] + 1) : 8 b[a]) - g0[a]) / gd[a], provided the cell of sample kn - 1 lies in the same block b; if not, kn - 1 is tried the same
//     way, and k + 1 is taken if that fails too.  The cell coordinates are monotone in k (every operation from k to the cell is monotone
//     under rounding), so with samples k and kn - 1 in block b every sample between them is: only samples of unflagged blocks are skipped,
//     whatever the rounding of s_exit.  Two samples that bracket a crossing lie in cells that share a corner (step < 1), one of those cells is
//     active and the other within one cell of it: both blocks are flagged, both samples evaluated - no output bit depends on `blocks`.
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

// ---- ray casting (the contract is at the head of this file) ----
constexpr int kTsdfBlock = 8;                         // cells per block and axis
constexpr int kRaycastMaxK = 1 << 22;
constexpr int kRaycastWaveX = 8, kRaycastWaveY = 8, kRaycastWavesX = 2, kRaycastWavesY = 2;      // a wave covers 8 x 8 pixels, a workgroup 2 x 2 of them
constexpr int kRaycastTileX = kRaycastWaveX * kRaycastWavesX, kRaycastTileY = kRaycastWaveY * kRaycastWavesY;

struct SurfaceBlocksParams {
    const unsigned char* cells;        // [nz-1][ny-1][nx-1]
    unsigned char* blocks;             // [bz][by][bx], b = ceil((n - 1) / 8)
    int mx, my, mz, bx, by;            // cells per axis; blocks per row and per slice
};

struct TsdfRaycastParams {
    const float* field;        // [nz][ny][nx] f, NaN = unknown
    const float* csum;         // [3][nz][ny][nx] (null: grey)
    const float* cw;
    const float* rays;         // [n][12]: M row-major, c
    const float* range;        // [n][2] near, far (null: [0, inf))
    const unsigned char* blocks;       // (null: every sample is evaluated)
    float* depth;              // [n][h][w]
    float* normal;             // [n][3][h][w] (may be null)
    float* colours;            // [n][3][h][w] (may be null)
    unsigned char* status;     // [n][h][w]
    int* evaluated;            // [n][h][w] (may be null)
    float ox, oy, oz, vs, step;
    int nx, ny, nz, h, w, bx, by;
};

// One wave per block of 8 x 8 x 8 cells: the 64 lanes read the block's 10 x 10 x 10 neighbourhood of cell bytes clipped to the cell grid
// (at most 1000 bytes, 16 rounds), a ballot combines them and lane 0 stores the byte.
__global__ void __launch_bounds__(64) surface_blocks_kernel(SurfaceBlocksParams p) {
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int bxi = b % p.bx, t = b / p.bx;
    const int byi = t % p.by, bzi = t / p.by;
    const int x0 = bxi * kTsdfBlock - 1, y0 = byi * kTsdfBlock - 1, z0 = bzi * kTsdfBlock - 1;
    constexpr int kSide = kTsdfBlock + 2;
    bool any = false;
    for (int i = lane; i < kSide * kSide * kSide; i += 64) {
        const int cx = x0 + i % kSide, cy = y0 + (i / kSide) % kSide, cz = z0 + i / (kSide * kSide);
        if (cx >= 0 && cy >= 0 && cz >= 0 && cx < p.mx && cy < p.my && cz < p.mz)
            any = any || (p.cells[((size_t)cz * p.my + cy) * p.mx + cx] & 1u) != 0u;
    }
    const bool flagged = __ballot(any) != 0ull;
    if (lane == 0) p.blocks[b] = flagged ? 1 : 0;
}

struct TsdfRay { float g0x, g0y, g0z, gdx, gdy, gdz, s_in, ds; };

__device__ __forceinline__ float tsdf_lerp(float a, float b, float t) { return a + t * (b - a); }

__device__ __forceinline__ int tsdf_cell_of(float g, int cells, float& t) {
    int c = (int)floorf(g);
    c = c < 0 ? 0 : (c > cells - 1 ? cells - 1 : c);
    t = g - (float)c;
    return c;
}

// the (clamped) cell of the point at z-depth s and the point's offsets in it -> the index of the cell's corner 0
__device__ __forceinline__ int tsdf_ray_cell(const TsdfRay& r, float s, int nx, int ny, int nz, int& cx, int& cy, int& cz, float& tx, float& ty,
                                             float& tz) {
    cx = tsdf_cell_of(r.g0x + s * r.gdx, nx - 1, tx);
    cy = tsdf_cell_of(r.g0y + s * r.gdy, ny - 1, ty);
    cz = tsdf_cell_of(r.g0z + s * r.gdz, nz - 1, tz);
    return (cz * ny + cy) * nx + cx;
}

__device__ __forceinline__ void tsdf_corners(const float* __restrict__ a, int base, int nx, int ny, float (&c)[8]) {
    NR_PRAGMA_UNROLL
    for (int j = 0; j < 8; ++j) c[j] = a[(size_t)base + (size_t)((j >> 2) * ny + ((j >> 1) & 1)) * nx + (j & 1)];
}

__device__ __forceinline__ float tsdf_trilinear(const float (&c)[8], float tx, float ty, float tz) {
    const float a0 = tsdf_lerp(c[0], c[1], tx), a1 = tsdf_lerp(c[2], c[3], tx), a2 = tsdf_lerp(c[4], c[5], tx), a3 = tsdf_lerp(c[6], c[7], tx);
    return tsdf_lerp(tsdf_lerp(a0, a1, ty), tsdf_lerp(a2, a3, ty), tz);
}

__device__ __forceinline__ bool tsdf_same_block(const TsdfRay& r, int k, int nx, int ny, int nz, int bx, int by, int bz) {
    int cx, cy, cz;
    float tx, ty, tz;
    tsdf_ray_cell(r, r.s_in + (float)k * r.ds, nx, ny, nz, cx, cy, cz, tx, ty, tz);
    return (cx >> 3) == bx && (cy >> 3) == by && (cz >> 3) == bz;
}

// the z-depth at which the ray leaves the slab of block coordinate b along one axis (inf where it never does)
__device__ __forceinline__ float tsdf_block_exit(float g0, float gd, int b) {
    if (gd == 0.0f) return INFINITY;
    return ((float)((gd > 0.0f ? b + 1 : b) * kTsdfBlock) - g0) / gd;
}

__global__ void __launch_bounds__(kRaycastTileX * kRaycastTileY) tsdf_raycast_kernel(TsdfRaycastParams p) {
    const int view = (int)blockIdx.z;
    const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
    const int x = (int)blockIdx.x * kRaycastTileX + (wave % kRaycastWavesX) * kRaycastWaveX + lane % kRaycastWaveX;
    const int y = (int)blockIdx.y * kRaycastTileY + (wave / kRaycastWavesX) * kRaycastWaveY + lane / kRaycastWaveX;
    if (x >= p.w || y >= p.h) return;                 // (nothing below needs the whole wave)
    const int nx = p.nx, ny = p.ny, nz = p.nz;
    const float* __restrict__ f = p.field;
    const float* __restrict__ cam = p.rays + (size_t)view * 12;        // (wave-uniform: scalar loads)
    const float px = (float)x, py = (float)y;
    const float dx = (cam[0] * px + cam[1] * py) + cam[2], dy = (cam[3] * px + cam[4] * py) + cam[5], dz = (cam[6] * px + cam[7] * py) + cam[8];
    TsdfRay r;
    r.g0x = (cam[9] - p.ox) / p.vs; r.g0y = (cam[10] - p.oy) / p.vs; r.g0z = (cam[11] - p.oz) / p.vs;
    r.gdx = dx / p.vs; r.gdy = dy / p.vs; r.gdz = dz / p.vs;
    float s_in = 0.0f, s_out = INFINITY;
    if (p.range) { s_in = p.range[(size_t)view * 2]; s_out = p.range[(size_t)view * 2 + 1]; }
    bool ok = true;
    NR_PRAGMA_UNROLL
    for (int a = 0; a < 3; ++a) {
        const float g0 = a == 0 ? r.g0x : (a == 1 ? r.g0y : r.g0z), gd = a == 0 ? r.gdx : (a == 1 ? r.gdy : r.gdz);
        const float hi = (float)((a == 0 ? nx : (a == 1 ? ny : nz)) - 1);
        if (gd == 0.0f) {
            if (g0 < 0.0f || g0 > hi) ok = false;
        } else {
            const float t1 = (0.0f - g0) / gd, t2 = (hi - g0) / gd;
            s_in = fmaxf(s_in, fminf(t1, t2));
            s_out = fminf(s_out, fmaxf(t1, t2));
        }
    }
    r.s_in = s_in;
    r.ds = (p.step * p.vs) / sqrtf((dx * dx + dy * dy) + dz * dz);
    ok = ok && s_in <= s_out && r.ds > 0.0f && r.ds < INFINITY;
    const int kmax = ok ? (int)floorf(fminf((s_out - s_in) / r.ds, (float)kRaycastMaxK)) : -1;
    const unsigned char* __restrict__ blocks = p.blocks;
    int k = 0, evaluated = 0, base = 0;
    unsigned status = 0u;
    float prev = NAN, cur = NAN, tx = 0.0f, ty = 0.0f, tz = 0.0f;
    while (k <= kmax) {                               // (divergent by nature: rays end at different k)
        int cx, cy, cz;
        base = tsdf_ray_cell(r, s_in + (float)k * r.ds, nx, ny, nz, cx, cy, cz, tx, ty, tz);
        if (blocks) {
            const int bx = cx >> 3, by = cy >> 3, bz = cz >> 3;          // (kTsdfBlock = 8)
            if (blocks[((size_t)bz * p.by + by) * p.bx + bx] == 0) {
                const float s_exit = fminf(fminf(tsdf_block_exit(r.g0x, r.gdx, bx), tsdf_block_exit(r.g0y, r.gdy, by)), tsdf_block_exit(r.g0z, r.gdz, bz));
                int kn = (int)floorf(fmaxf(fminf((s_exit - s_in) / r.ds, (float)kmax), 0.0f)) + 1;
                kn = kn > k + 1 ? kn : k + 1;
                if (kn > k + 1 && !tsdf_same_block(r, kn - 1, nx, ny, nz, bx, by, bz)) {
                    kn = kn - 1;
                    if (kn > k + 1 && !tsdf_same_block(r, kn - 1, nx, ny, nz, bx, by, bz)) kn = k + 1;
                }
                prev = NAN;
                k = kn;
                continue;
            }
        }
        float c[8];
        tsdf_corners(f, base, nx, ny, c);
        cur = tsdf_trilinear(c, tx, ty, tz);
        evaluated = evaluated + 1;
        if (prev == prev && cur == cur && (prev < 0.0f) != (cur < 0.0f)) {
            status = cur < 0.0f ? 1u : 2u;
            break;
        }
        prev = cur;
        k = k + 1;
    }
    const size_t plane = (size_t)p.h * p.w, pix = (size_t)view * plane + (size_t)y * p.w + x, pix3 = (size_t)view * 3 * plane + (size_t)y * p.w + x;
    float depth = 0.0f, n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (status == 1u) {
        depth = (s_in + (float)(k - 1) * r.ds) + r.ds * (prev / (prev - cur));
        float c[8];
        if (p.normal || p.colours) {                  // (base, tx, ty, tz: sample k's, from the loop)
            int cx, cy, cz;
            float hx, hy, hz;
            const int hit = tsdf_ray_cell(r, depth, nx, ny, nz, cx, cy, cz, hx, hy, hz);
            tsdf_corners(f, hit, nx, ny, c);
            bool known = true;
            NR_PRAGMA_UNROLL
            for (int j = 0; j < 8; ++j) known = known && c[j] == c[j];
            if (known) { base = hit; tx = hx; ty = hy; tz = hz; }
            else tsdf_corners(f, base, nx, ny, c);
        }
        if (p.normal) {
            const float gx = tsdf_lerp(tsdf_lerp(c[1] - c[0], c[3] - c[2], ty), tsdf_lerp(c[5] - c[4], c[7] - c[6], ty), tz);
            const float gy = tsdf_lerp(tsdf_lerp(c[2] - c[0], c[3] - c[1], tx), tsdf_lerp(c[6] - c[4], c[7] - c[5], tx), tz);
            const float gz = tsdf_lerp(tsdf_lerp(c[4] - c[0], c[5] - c[1], tx), tsdf_lerp(c[6] - c[2], c[7] - c[3], tx), ty);
            const float len2 = (gx * gx + gy * gy) + gz * gz;
            if (len2 > 0.0f) { const float len = sqrtf(len2); n0 = gx / len; n1 = gy / len; n2 = gz / len; }
        }
        if (p.colours) {
            c0 = c1 = c2 = 0.5f;
            if (p.csum) {
                const size_t vol = (size_t)nx * ny * nz;
                tsdf_corners(p.cw, base, nx, ny, c);
                const float den = tsdf_trilinear(c, tx, ty, tz);
                if (den > 0.0f) {
                    tsdf_corners(p.csum, base, nx, ny, c);
                    c0 = tsdf_trilinear(c, tx, ty, tz) / den;
                    tsdf_corners(p.csum + vol, base, nx, ny, c);
                    c1 = tsdf_trilinear(c, tx, ty, tz) / den;
                    tsdf_corners(p.csum + 2 * vol, base, nx, ny, c);
                    c2 = tsdf_trilinear(c, tx, ty, tz) / den;
                }
            }
        }
    }
    p.depth[pix] = depth;
    p.status[pix] = (unsigned char)status;
    if (p.normal) { p.normal[pix3] = n0; p.normal[pix3 + plane] = n1; p.normal[pix3 + 2 * plane] = n2; }
    if (p.colours) { p.colours[pix3] = c0; p.colours[pix3 + plane] = c1; p.colours[pix3 + 2 * plane] = c2; }
    if (p.evaluated) p.evaluated[pix] = evaluated;
}

}  // namespace nr
