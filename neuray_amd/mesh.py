"""Mesh export: TSDF fusion of posed depth maps and surface-nets extraction.

Per-view depth maps - a database's, or `render_depth_fine` of a renderer, optionally through geometry.filter_depth - are integrated into a
truncated signed distance field on a regular lattice, and its zero surface is extracted as a watertight triangle mesh by naive surface nets
(one vertex per cell the surface crosses, one quad per lattice edge it crosses: no case table).  `integrate_numpy` / `surface_nets_numpy` restate
the formulas vectorised in float64 or float32 (the reference of the tests and the path of a machine without a GPU, like
geometry.consistency_numpy); csrc/nr_kernels_tsdf.h through `RenderEngine.tsdf_integrate` / `surface_cells` / `surface_emit` evaluates the
same operations in fp32 on the device.

Lattice point (ix, iy, iz), 0 <= i < (nx, ny, nz), sits at origin + (ix, iy, iz) * vs.  Arrays are [nz][ny][nx], x fastest; colour is planar
[3][nz][ny][nx].  Pixel centres sit at integer coordinates, depth is z-depth, 0 = none, read at the nearest texel.  The state of a volume is
sums, float32, zero-initialised: Tsum, W, Csum[3], Cw.  For lattice point p and view i, the views in ascending order:
  Pc = R_i p + t_i, z = Pc.z;  q = K_i Pc, u = q.x / q.z, v = q.y / q.z, un = floor(u + 0.5), vn = floor(v + 0.5)
  skip unless z > 0, 0 <= un < w, 0 <= vn < h, d = D_i[vn,un] > 0;   sdf = d - z;   skip if sdf < -trunc
  Tsum += min(sdf / trunc, 1), W += 1;   if sdf <= trunc: Csum[c] += rgb_i[c][vn,un], Cw += 1
Extraction: f = Tsum / W; a lattice point is inside where f < 0; cell (cx, cy, cz), 0 <= c < n - 1, with the corners (c + d), d in {0,1}^3, is
valid where all 8 corners have W >= min_weight, active where it is valid and its corners are not all on one side.  The cell byte: bit 0 active;
bits 1..3: the cell emits the quad of the lattice edge from its corner (cx, cy, cz) towards +x / +y / +z - the edge's ends differ in `inside`
and the four cells around it exist and are valid (for axis a, (a, b, c) cyclic, the cells at offsets (b-1, c-1), (b, c-1), (b, c), (b-1, c)).
An active cell's vertex is origin + (cell + m) * vs, m the mean of the crossing points t = f_lo / (f_lo - f_hi) of its edges whose ends differ
in `inside` (the four x-edges, then y, then z, each with the other two offsets - in ascending axis order - running 00, 10, 01, 11); its normal
the normalised sums of the forward differences of f over the four edges per axis (towards free space); its colour sum Csum / sum Cw over the
corners in corner order (x fastest), 0.5 grey where that is 0 / 0.  A quad is the four cells' vertices in the order above where the edge's low
end is inside, reversed otherwise; its triangles are (v0, v1, v2) and (v0, v2, v3); faces are ordered by owner cell, then axis.

Ray casting of a volume: per view and pixel the first zero crossing of the field along the pixel's ray (DESIGN.md 4.22;
csrc/nr_kernels_tsdf.h evaluates the same operations in fp32, `raycast_numpy` restates them in float64 or float32).

  field: f = Tsum / W in float32, NaN ("unknown") where W < min_weight (`field_numpy`).  A cell is valid where none of its 8 corners is unknown.
  ray of pixel (x, y) of view i (pixel centres at integers): the 12 floats M = R^T K^-1 (row-major) and c = -R^T t, made in float64 and
    rounded to float32 (`ray_table`); d[a] = (M[a][0] x + M[a][1] y) + M[a][2]; the point at z-depth s is c + s d, so s is z-depth; in
    lattice units g[a](s) = g0[a] + s gd[a] with g0[a] = (c[a] - origin[a]) / vs and gd[a] = d[a] / vs.
  interval: [s_in, s_out] starts as [near, far] (depth_range [n,2], default [0, inf)); per axis a with hi = n[a] - 1: if gd[a] == 0 the ray
    is empty where g0[a] < 0 or g0[a] > hi, else t1 = (0 - g0[a]) / gd[a], t2 = (hi - g0[a]) / gd[a], s_in = max(s_in, min(t1, t2)), s_out =
    min(s_out, max(t1, t2)).  Empty unless s_in <= s_out: status 0.
  samples: ds = (step vs) / sqrt((d0 d0 + d1 d1) + d2 d2), step in voxels, 0 < step <= 0.95 (a ray without 0 < ds < inf is empty); s_k = s_in +
    k ds for k = 0 .. floor(min((s_out - s_in) / ds, 2^22)).
  value at s: cell[a] = clamp(floor(g[a]), 0, n[a] - 2), t[a] = g[a] - cell[a]; with the corners c_j, j = dz 4 + dy 2 + dx, and lerp(p, q,
    t) = p + t (q - p): along x first, a_0..3 = lerp(c_0, c_1), lerp(c_2, c_3), lerp(c_4, c_5), lerp(c_6, c_7) at t[0]; then y, b_0 =
    lerp(a_0, a_1), b_1 = lerp(a_2, a_3) at t[1]; then z, lerp(b_0, b_1) at t[2].  Unknown (NaN) if any corner is.
  first crossing: the first k whose samples k - 1 and k are both known (and both evaluated) with (f_{k-1} < 0) != (f_k < 0) - inside is f <
    0, the extraction's definition.  f_k < 0: status 1 (hit), depth = s_{k-1} + ds (f_{k-1} / (f_{k-1} - f_k)); otherwise status 2 (the
    surface seen from behind), depth 0.  The ray ends there.  No crossing: status 0, depth 0.
  at a hit: the cell and t of g(depth) where that cell is valid, else those of sample k.  Normal: the gradient of the trilinear interpolant
    there - per axis the four corner differences along it (the other two offsets, in ascending axis order, running 00, 10, 01, 11), lerped
    over the lower, then the higher of the other two axes - divided by its length (towards free space, surface_emit's sign; zero where the
    length is zero).  Colour: the trilinear combination of Csum[c] over that of Cw; 0.5 grey where that denominator is not positive or the
    volume has no colour.  Pixels without a hit have zero normals and colours.
  block skipping: `blocks` (`blocks_numpy`) holds one byte per block of 8 x 8 x 8 cells, non-zero where a cell of the block or within one
    cell of it is active.  A sample whose cell lies in an unflagged block is not evaluated and counts as unknown; k then moves to kn = max(k
    + 1, floor(clamp((s_exit - s_in) / ds, 0, kmax)) + 1), s_exit the smallest over the axes with gd[a] != 0 of ((gd[a] > 0 ? 8 (b[a] + 1) :
    8 b[a]) - g0[a]) / gd[a], provided the cell of sample kn - 1 lies in the same block b; if it does not, kn - 1 is tried the same way, and k
    + 1 is taken if that fails too.  No output but `evaluated` (the number of field samples evaluated) depends on `blocks`."""
import numpy as np
import torch

from . import geometry as _geo

MAX_POINTS = 1 << 30
_CYCLIC = ((1, 2), (2, 0), (0, 1))          # (b, c) of axis a, as axes 0 = x, 1 = y, 2 = z


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _check_volume(dims, voxel_size, trunc):
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 2:
        raise ValueError("neuray_amd.mesh: dims %r (three dimensions of at least 2)" % (dims,))
    if dims[0] * dims[1] * dims[2] > MAX_POINTS:
        raise ValueError("neuray_amd.mesh: %d lattice points (at most 2^30)" % (dims[0] * dims[1] * dims[2]))
    if not voxel_size > 0 or not trunc > 0:
        raise ValueError("neuray_amd.mesh: voxel_size and trunc must be positive")
    return dims


def zero_state(dims, colour=True):
    nx, ny, nz = dims
    state = {'tsum': np.zeros((nz, ny, nx), np.float32), 'w': np.zeros((nz, ny, nx), np.float32)}
    if colour:
        state.update(csum=np.zeros((3, nz, ny, nx), np.float32), cw=np.zeros((nz, ny, nx), np.float32))
    return state


def integrate_numpy(depth, imgs, poses, Ks, origin, voxel_size, dims, trunc, views=None, state=None, colour=True, dtype=np.float64,
                    details=False):
    """Adds the views [v0, v1) (None: all) to `state` (None: zeros) -> a new state dict(tsum, w [nz,ny,nx], csum [3,nz,ny,nx], cw) of
    `dtype` (the sums are carried in dtype: float32 gives the kernel's bits up to the rounding of its operations) and, with details, per
    (view of the range, lattice point) [v1-v0,nz,ny,nx] float64 u, v, z, sdf and bool 'seen' (z > 0, texel inside, d > 0), 'kept' (seen and not
    sdf < -trunc), 'coloured' (kept and sdf <= trunc)."""
    nx, ny, nz = _check_volume(dims, voxel_size, trunc)
    T = np.dtype(dtype).type
    depth = np.asarray(depth, np.float32)
    n, h, w = depth.shape
    D = depth.astype(T)
    P, K, _ = _geo._cameras(poses, Ks, T)
    if P.shape[0] != n or K.shape[0] != n:
        raise ValueError("neuray_amd.mesh: %d depth maps, %d poses, %d Ks" % (n, P.shape[0], K.shape[0]))
    rgb = None
    if colour:
        rgb = np.asarray(imgs, np.float32)
        if rgb.shape != (n, 3, h, w):
            raise ValueError("neuray_amd.mesh: imgs %r for depth %r" % (rgb.shape, depth.shape))
        rgb = rgb.reshape(n, 3, h * w).astype(T)
    v0, v1 = (0, n) if views is None else (int(views[0]), int(views[1]))
    if not 0 <= v0 <= v1 <= n:
        raise ValueError("neuray_amd.mesh: views [%d,%d) outside [0,%d)" % (v0, v1, n))
    state = zero_state((nx, ny, nz), colour) if state is None else state
    out = {k: np.array(state[k], dtype=T) for k in (('tsum', 'w', 'csum', 'cw') if colour else ('tsum', 'w'))}
    o, vs, tr = [T(np.float32(c)) for c in origin], T(np.float32(voxel_size)), T(np.float32(trunc))
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    X = [o[0] + ix.astype(T) * vs, o[1] + iy.astype(T) * vs, o[2] + iz.astype(T) * vs]
    det = None
    if details:
        det = {k: np.zeros((v1 - v0, nz, ny, nx), np.float64) for k in ('u', 'v', 'z', 'sdf')}
        det.update({k: np.zeros((v1 - v0, nz, ny, nx), bool) for k in ('seen', 'kept', 'coloured')})
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i in range(v0, v1):
            u, v, z = _geo._project(P[i], K[i], X)
            un, vn = np.floor(u + T(0.5)), np.floor(v + T(0.5))
            inb = (z > 0) & (un >= 0) & (un < w) & (vn >= 0) & (vn < h)
            t = np.where(inb, vn, 0).astype(np.int64) * w + np.where(inb, un, 0).astype(np.int64)
            d = np.where(inb, D[i].reshape(-1)[t], T(0))
            seen = inb & (d > 0)
            sdf = d - z
            kept = seen & ~(sdf < -tr)
            out['tsum'] = np.where(kept, out['tsum'] + np.minimum(sdf / tr, T(1)), out['tsum'])
            out['w'] = np.where(kept, out['w'] + T(1), out['w'])
            coloured = kept & (sdf <= tr)
            if colour:
                for c in range(3):
                    out['csum'][c] = np.where(coloured, out['csum'][c] + rgb[i, c][t], out['csum'][c])
                out['cw'] = np.where(coloured, out['cw'] + T(1), out['cw'])
            if details:
                for k, a in (('u', u), ('v', v), ('z', z), ('sdf', sdf), ('seen', seen), ('kept', kept), ('coloured', coloured)):
                    det[k][i - v0] = a
    if details:
        out.update(det)
    return out


def _corner(a, dx, dy, dz):
    """a[z + dz, y + dy, x + dx] over the cells"""
    nz, ny, nx = a.shape
    return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def _cell_shift(a, sx, sy, sz):
    """a[cz - sz, cy - sy, cx - sx] over the cells (s in {0, 1}), False where that cell does not exist"""
    o = np.zeros_like(a)
    mz, my, mx = a.shape
    o[sz:, sy:, sx:] = a[:mz - sz, :my - sy, :mx - sx]
    return o


def cells_numpy(tsum, w, min_weight=1.0, dtype=np.float64):
    """-> (cells uint8 [nz-1,ny-1,nx-1], f [nz,ny,nx] dtype): the cell bytes and f = Tsum / W (NaN or inf where W = 0)"""
    if not min_weight > 0:
        raise ValueError("neuray_amd.mesh: min_weight must be positive")
    T = np.dtype(dtype).type
    tsum, w = np.asarray(tsum).astype(T), np.asarray(w).astype(T)
    if tsum.ndim != 3 or tsum.shape != w.shape or min(tsum.shape) < 2:
        raise ValueError("neuray_amd.mesh: tsum %r and w %r ([nz,ny,nx], each at least 2)" % (tsum.shape, w.shape))
    with np.errstate(divide='ignore', invalid='ignore'):
        f = tsum / w
        inside = f < 0
    ok = w >= T(np.float32(min_weight))
    valid = np.ones(tuple(s - 1 for s in tsum.shape), bool)
    any_in, all_in = np.zeros_like(valid), np.ones_like(valid)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
        valid &= _corner(ok, dx, dy, dz)
        any_in |= _corner(inside, dx, dy, dz)
        all_in &= _corner(inside, dx, dy, dz)
    cells = (valid & any_in & ~all_in).astype(np.uint8)
    lo = _corner(inside, 0, 0, 0)
    for a in range(3):
        hi = _corner(inside, *[1 if k == a else 0 for k in range(3)])
        b, c = _CYCLIC[a]
        sb, sc = [1 if k == b else 0 for k in range(3)], [1 if k == c else 0 for k in range(3)]
        around = valid & _cell_shift(valid, *sb) & _cell_shift(valid, *sc) & _cell_shift(valid, *[p + q for p, q in zip(sb, sc)])
        cells |= ((lo != hi) & around).astype(np.uint8) << (a + 1)
    return cells, f


def surface_nets_numpy(tsum, w, csum, cw, origin, voxel_size, min_weight=1.0, dtype=np.float64):
    """The mesh of a volume's state -> dict(cells uint8 [nz-1,ny-1,nx-1], vertices / normals / colors [m,3] dtype, faces [k,3] int32).
    csum / cw None: grey."""
    T = np.dtype(dtype).type
    if not voxel_size > 0:
        raise ValueError("neuray_amd.mesh: voxel_size must be positive")
    cells, f = cells_numpy(tsum, w, min_weight, dtype)
    mz, my, mx = cells.shape
    active = (cells & 1) > 0
    cz, cy, cx = [a[active] for a in np.meshgrid(np.arange(mz), np.arange(my), np.arange(mx), indexing='ij')]
    m = cx.shape[0]
    fc = [_corner(f, k & 1, (k >> 1) & 1, k >> 2)[active] for k in range(8)]
    acc = [np.zeros(m, T) for _ in range(3)]
    grad = [np.zeros(m, T) for _ in range(3)]
    crossings = np.zeros(m, np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):
        for axis in range(3):
            for e in range(4):
                o1, o2 = e & 1, e >> 1
                d = [0, 0, 0]
                d[[k for k in range(3) if k != axis][0]], d[[k for k in range(3) if k != axis][1]] = o1, o2
                klo = d[2] * 4 + d[1] * 2 + d[0]
                flo, fhi = fc[klo], fc[klo + (1 << axis)]
                grad[axis] = grad[axis] + (fhi - flo)
                cross = (flo < 0) != (fhi < 0)
                t = flo / (flo - fhi)
                for k in range(3):
                    acc[k] = np.where(cross, acc[k] + (t if k == axis else T(d[k])), acc[k])
                crossings += cross
        cnt = crossings.astype(T)
        o, vs = [T(np.float32(c)) for c in origin], T(np.float32(voxel_size))
        vertices = np.stack([o[k] + ((cx, cy, cz)[k].astype(T) + acc[k] / cnt) * vs for k in range(3)], -1) if m else np.zeros((0, 3), T)
        len2 = grad[0] * grad[0] + grad[1] * grad[1] + grad[2] * grad[2]
        ln = np.sqrt(len2)
        normals = np.stack([np.where(len2 > 0, grad[k] / ln, T(0)) for k in range(3)], -1) if m else np.zeros((0, 3), T)
        if csum is not None:
            csum, cw = np.asarray(csum).astype(T), np.asarray(cw).astype(T)
            s, sw = [np.zeros(m, T) for _ in range(3)], np.zeros(m, T)
            for k in range(8):
                for c in range(3):
                    s[c] = s[c] + _corner(csum[c], k & 1, (k >> 1) & 1, k >> 2)[active]
                sw = sw + _corner(cw, k & 1, (k >> 1) & 1, k >> 2)[active]
            colors = np.stack([np.where(sw > 0, s[c] / sw, T(0.5)) for c in range(3)], -1) if m else np.zeros((0, 3), T)
        else:
            colors = np.full((m, 3), T(0.5))
    vid = (np.cumsum(active.reshape(-1)) - active.reshape(-1)).reshape(cells.shape)
    lo_inside = _corner(f < 0, 0, 0, 0) if m else np.zeros(cells.shape, bool)
    strides = (1, mx, mx * my)
    owners, axes, quads = [], [], []
    for a in range(3):
        own = np.flatnonzero(((cells >> (a + 1)) & 1).reshape(-1))
        b, c = _CYCLIC[a]
        ring = np.stack([own - strides[b] - strides[c], own - strides[c], own, own - strides[b]], -1)
        rev = ~lo_inside.reshape(-1)[own]
        ring[rev] = ring[rev][:, ::-1]
        owners.append(own)
        axes.append(np.full(own.shape[0], a, np.int64))
        quads.append(vid.reshape(-1)[ring].reshape(-1, 4))
    owners, axes, quads = np.concatenate(owners), np.concatenate(axes), np.concatenate(quads)
    order = np.argsort(owners * 3 + axes, kind='stable')
    q = quads[order]
    faces = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    return {'cells': cells, 'vertices': vertices, 'normals': normals, 'colors': colors, 'faces': faces}


def boundary_edges(faces):
    """the number of undirected edges of a triangle list that belong to exactly one face (0: the mesh is closed)"""
    faces = np.asarray(_geo._host(faces)).astype(np.int64).reshape(-1, 3)
    if faces.shape[0] == 0:
        return 0
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    _, counts = np.unique(e[:, 0] * (faces.max() + 1) + e[:, 1], return_counts=True)
    return int((counts == 1).sum())


# ---- ray casting --------------------------------------------------------------------------------------------------------
BLOCK = 8
RAYCAST_MAX_K = 1 << 22
MAX_STEP = 0.95


def field_numpy(tsum, w, min_weight=1.0):
    """f = Tsum / W as float32 [nz,ny,nx], NaN where W < min_weight"""
    if not min_weight > 0:
        raise ValueError("neuray_amd.mesh: min_weight must be positive")
    tsum, w = np.asarray(tsum, np.float32), np.asarray(w, np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(w >= np.float32(min_weight), tsum / w, np.float32('nan')).astype(np.float32)


def ray_table(poses, Ks):
    """[n,12] float32: M = R^T K^-1 row-major, then c = -R^T t; float64 arithmetic on the float32 cameras, rounded once"""
    P = np.asarray(_geo._host(poses), np.float32).reshape(-1, 3, 4).astype(np.float64)
    K = np.asarray(_geo._host(Ks), np.float32).reshape(-1, 3, 3).astype(np.float64)
    if P.shape[0] != K.shape[0]:
        raise ValueError("neuray_amd.mesh: %d poses, %d Ks" % (P.shape[0], K.shape[0]))
    Rt = P[:, :, :3].transpose(0, 2, 1)
    return np.concatenate([(Rt @ np.linalg.inv(K)).reshape(-1, 9), -(Rt @ P[:, :, 3:])[:, :, 0]], 1).astype(np.float32)


def blocks_numpy(cells):
    """cell bytes [nz-1,ny-1,nx-1] -> uint8 [bz,by,bx], b = ceil((n - 1) / 8): 1 where a cell of the block or within one cell of it is active"""
    active = (np.asarray(cells) & 1) > 0
    if active.ndim != 3 or min(active.shape) < 1:
        raise ValueError("neuray_amd.mesh: cells %r ([nz-1,ny-1,nx-1])" % (active.shape,))
    grown = np.zeros(tuple(s + 2 for s in active.shape), bool)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                grown[dz:dz + active.shape[0], dy:dy + active.shape[1], dx:dx + active.shape[2]] |= active
    grown = grown[1:-1, 1:-1, 1:-1]
    nb = tuple(-(-s // BLOCK) for s in active.shape)
    padded = np.zeros(tuple(b * BLOCK for b in nb), bool)
    padded[:active.shape[0], :active.shape[1], :active.shape[2]] = grown
    return padded.reshape(nb[0], BLOCK, nb[1], BLOCK, nb[2], BLOCK).any((1, 3, 5)).astype(np.uint8)


def _check_raycast(shape, voxel_size, h, w, step, n, depth_range, blocks):
    nz, ny, nx = shape
    _check_volume((nx, ny, nz), voxel_size, 1.0)
    if h < 1 or w < 1:
        raise ValueError("neuray_amd.mesh: image size h=%d w=%d must be positive" % (h, w))
    if not 0 < step <= MAX_STEP:
        raise ValueError("neuray_amd.mesh: step=%r outside (0, %g] voxels" % (step, MAX_STEP))
    if depth_range is not None:
        depth_range = np.asarray(_geo._host(depth_range), np.float32)
        if depth_range.shape != (n, 2) or not np.all((depth_range[:, 0] >= 0) & (depth_range[:, 0] <= depth_range[:, 1])):
            raise ValueError("neuray_amd.mesh: depth_range [%d,2] with 0 <= near <= far" % n)
    if blocks is not None:
        blocks = np.asarray(blocks)
        want = tuple(-(-(s - 1) // BLOCK) for s in shape)
        if blocks.shape != want:
            raise ValueError("neuray_amd.mesh: blocks %r for a volume of %r cells (%r)" % (blocks.shape, tuple(s - 1 for s in shape), want))
    return depth_range, blocks


def _lerp(a, b, t):
    return a + t * (b - a)


def _trilinear(c, t):
    a = [_lerp(c[2 * j], c[2 * j + 1], t[0]) for j in range(4)]
    return _lerp(_lerp(a[0], a[1], t[1]), _lerp(a[2], a[3], t[1]), t[2])


def raycast_numpy(field, csum, cw, origin, voxel_size, poses, Ks, h, w, step=0.5, depth_range=None, dtype=np.float64, blocks=None,
                  details=False):
    """The reference of the ray caster (the module docstring states the operations), vectorised over the pixels.  field [nz,ny,nx] float32 (`field_numpy`), csum
    [3,nz,ny,nx] / cw [nz,ny,nx] or None -> dict(depth [n,h,w] dtype, normal [n,3,h,w], colors [n,3,h,w], status [n,h,w] uint8, evaluated
    [n,h,w] int32) and, with details, per pixel float64: 'min_abs_f' (the smallest |f| of a known evaluated sample), 'end' (the distance of
    (s_out - s_in) / ds to an integer), 'block_face' (the smallest distance, in voxels, of a visited sample to a face between two blocks), 'cell_face'
    (that of the hit point to a cell face); inf where there is none."""
    T = np.dtype(dtype).type
    field = np.asarray(field, np.float32)
    if field.ndim != 3:
        raise ValueError("neuray_amd.mesh: field %r ([nz,ny,nx])" % (field.shape,))
    nz, ny, nx = field.shape
    rays = ray_table(poses, Ks).astype(T)
    n = rays.shape[0]
    h, w = int(h), int(w)
    depth_range, blocks = _check_raycast(field.shape, voxel_size, h, w, step, n, depth_range, blocks)
    dims = (nx, ny, nz)
    F = field.astype(T).reshape(-1)
    o, vs, st = [T(np.float32(c)) for c in origin], T(np.float32(voxel_size)), T(np.float32(step))
    view, py, px = [a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing='ij')]
    R = view.shape[0]
    x, y = px.astype(T), py.astype(T)
    cam = rays[view]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        d = [(cam[:, 3 * a] * x + cam[:, 3 * a + 1] * y) + cam[:, 3 * a + 2] for a in range(3)]
        g0 = [(cam[:, 9 + a] - o[a]) / vs for a in range(3)]
        gd = [d[a] / vs for a in range(3)]
        if depth_range is None:
            s_in, s_out = np.zeros(R, T), np.full(R, T(np.inf))
        else:
            s_in, s_out = depth_range.astype(T)[view, 0], depth_range.astype(T)[view, 1]
        ok = np.ones(R, bool)
        for a in range(3):
            hi = T(dims[a] - 1)
            zero = gd[a] == 0
            t1, t2 = (T(0) - g0[a]) / gd[a], (hi - g0[a]) / gd[a]
            s_in = np.where(zero, s_in, np.maximum(s_in, np.minimum(t1, t2)))
            s_out = np.where(zero, s_out, np.minimum(s_out, np.maximum(t1, t2)))
            ok &= ~(zero & ((g0[a] < 0) | (g0[a] > hi)))
        ds = (st * vs) / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        ok &= (s_in <= s_out) & (ds > 0) & (ds < np.inf)
        q_end = (s_out - s_in) / ds
        kmax = np.where(ok, np.floor(np.minimum(np.where(ok, q_end, 0), T(RAYCAST_MAX_K))), -1).astype(np.int64)

        def cell_of(idx, s):
            """(cell [3] int64, t [3], g [3]) of the points at z-depth s of the rays idx"""
            g = [g0[a][idx] + s * gd[a][idx] for a in range(3)]
            cell = [np.clip(np.floor(g[a]), 0, dims[a] - 2).astype(np.int64) for a in range(3)]
            return cell, [g[a] - cell[a].astype(T) for a in range(3)], g

        def corners(arr, cell):
            base = (cell[2] * ny + cell[1]) * nx + cell[0]
            return [arr[base + ((j >> 2) * ny + ((j >> 1) & 1)) * nx + (j & 1)] for j in range(8)]

        def block_of(cell):
            return [cell[a] >> 3 for a in range(3)]

        nb = tuple(-(-(dims[a] - 1) // BLOCK) for a in range(3))
        flags = None if blocks is None else (blocks.reshape(-1) != 0)
        k = np.zeros(R, np.int64)
        prev = np.full(R, T(np.nan))
        status = np.zeros(R, np.uint8)
        evaluated = np.zeros(R, np.int32)
        f_lo, f_hi = np.zeros(R, T), np.zeros(R, T)
        det = {key: np.full(R, np.inf) for key in ('min_abs_f', 'block_face', 'cell_face')} if details else None
        live = np.flatnonzero(k <= kmax)
        while live.size:
            s = s_in[live] + k[live].astype(T) * ds[live]
            cell, t, g = cell_of(live, s)
            if details:
                for a in range(3):                           # the faces between two blocks: 8 j for 1 <= j <= (n - 2) // 8
                    ga = g[a].astype(np.float64)
                    j = np.round(ga / BLOCK)
                    face = np.where((j >= 1) & (j <= (dims[a] - 2) // BLOCK), np.abs(ga - j * BLOCK), np.inf)
                    det['block_face'][live] = np.minimum(det['block_face'][live], face)
            skip = np.zeros(live.size, bool)
            if flags is not None:
                b = block_of(cell)
                skip = ~flags[(b[2] * nb[1] + b[1]) * nb[0] + b[0]]
                if skip.any():
                    idx = live[skip]
                    bs, kk = [b[a][skip] for a in range(3)], k[idx]
                    s_exit = None
                    for a in range(3):
                        face = np.where(gd[a][idx] > 0, (bs[a] + 1) * BLOCK, bs[a] * BLOCK).astype(T)
                        e = np.where(gd[a][idx] == 0, T(np.inf), (face - g0[a][idx]) / gd[a][idx])
                        s_exit = e if s_exit is None else np.minimum(s_exit, e)
                    kn = np.floor(np.maximum(np.minimum((s_exit - s_in[idx]) / ds[idx], kmax[idx].astype(T)), T(0))).astype(np.int64) + 1
                    kn = np.maximum(kn, kk + 1)

                    def same(kq):
                        bq = block_of(cell_of(idx, s_in[idx] + kq.astype(T) * ds[idx])[0])
                        return (bq[0] == bs[0]) & (bq[1] == bs[1]) & (bq[2] == bs[2])
                    bad = (kn > kk + 1) & ~same(kn - 1)
                    kn = np.where(bad, kn - 1, kn)
                    bad = bad & (kn > kk + 1) & ~same(kn - 1)
                    kn = np.where(bad, kk + 1, kn)
                    prev[idx] = T(np.nan)
                    k[idx] = kn
            ev = live[~skip]
            cur = _trilinear(corners(F, [c[~skip] for c in cell]), [a[~skip] for a in t])
            evaluated[ev] += 1
            if details:
                det['min_abs_f'][ev] = np.fmin(det['min_abs_f'][ev], np.abs(cur).astype(np.float64))
            cross = (prev[ev] == prev[ev]) & (cur == cur) & ((prev[ev] < 0) != (cur < 0))
            hit = ev[cross]
            status[hit] = np.where(cur[cross] < 0, 1, 2)
            f_lo[hit], f_hi[hit] = prev[hit], cur[cross]
            kmax[hit] = -1                                   # the ray ends there (k stays at the crossing's)
            go = ev[~cross]
            prev[go] = cur[~cross]
            k[go] += 1
            live = live[k[live] <= kmax[live]]
        hit = np.flatnonzero(status == 1)
        depth = np.zeros(R, T)
        depth[hit] = (s_in[hit] + (k[hit] - 1).astype(T) * ds[hit]) + ds[hit] * (f_lo[hit] / (f_lo[hit] - f_hi[hit]))
        cell, t, g = cell_of(hit, depth[hit])
        c = corners(F, cell)
        known = np.ones(hit.size, bool)
        for j in range(8):
            known &= c[j] == c[j]
        cell_k, t_k, _ = cell_of(hit, s_in[hit] + k[hit].astype(T) * ds[hit])
        cell = [np.where(known, cell[a], cell_k[a]) for a in range(3)]
        t = [np.where(known, t[a], t_k[a]) for a in range(3)]
        c = corners(F, cell)
        if details:
            det['cell_face'][hit] = np.min([np.abs(g[a].astype(np.float64) - np.round(g[a].astype(np.float64))) for a in range(3)], 0)
        grad = [_lerp(_lerp(c[1] - c[0], c[3] - c[2], t[1]), _lerp(c[5] - c[4], c[7] - c[6], t[1]), t[2]),
                _lerp(_lerp(c[2] - c[0], c[3] - c[1], t[0]), _lerp(c[6] - c[4], c[7] - c[5], t[0]), t[2]),
                _lerp(_lerp(c[4] - c[0], c[5] - c[1], t[0]), _lerp(c[6] - c[2], c[7] - c[3], t[0]), t[1])]
        len2 = (grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]
        ln = np.sqrt(len2)
        normal, colors = np.zeros((R, 3), T), np.zeros((R, 3), T)
        colors[hit] = T(0.5)
        for a in range(3):
            normal[hit, a] = np.where(len2 > 0, grad[a] / ln, T(0))
        if csum is not None:
            den = _trilinear(corners(np.asarray(cw, np.float32).astype(T).reshape(-1), cell), t)
            for a in range(3):
                num = _trilinear(corners(np.asarray(csum[a], np.float32).astype(T).reshape(-1), cell), t)
                colors[hit, a] = np.where(den > 0, num / den, T(0.5))
    out = {'depth': depth.reshape(n, h, w), 'normal': normal.reshape(n, h, w, 3).transpose(0, 3, 1, 2).copy(),
           'colors': colors.reshape(n, h, w, 3).transpose(0, 3, 1, 2).copy(), 'status': status.reshape(n, h, w),
           'evaluated': evaluated.reshape(n, h, w)}
    if details:
        with np.errstate(invalid='ignore'):
            det['end'] = np.where(ok, np.abs(q_end.astype(np.float64) - np.round(q_end.astype(np.float64))), np.inf)
        out.update({key: v.reshape(n, h, w) for key, v in det.items()})
    return out


# ---- the public surface --------------------------------------------------------------------------------------------------------------
class TSDFVolume:
    """A truncated signed distance field on a regular lattice: origin (3,), voxel_size, dims (nx, ny, nz); trunc defaults to 3 voxels.
    On the device when there is one (or `engine` is given): the state lives in device tensors and the three kernels run; on NumPy (the
    float32 reference) otherwise."""

    def __init__(self, origin, voxel_size, dims, trunc=None, colour=True, engine=None):
        self.origin = tuple(float(c) for c in origin)
        self.voxel_size = float(voxel_size)
        self.trunc = 3.0 * self.voxel_size if trunc is None else float(trunc)
        self.dims = _check_volume(dims, self.voxel_size, self.trunc)
        if len(self.origin) != 3:
            raise ValueError("neuray_amd.mesh: origin %r" % (origin,))
        self.colour = bool(colour)
        self.engine = _geo._engine(engine)
        if self.engine is not None and self.engine.variant != 'fp32':
            raise NotImplementedError("neuray_amd: the mesh export lives in the fp32 library (variant=%r)" % (self.engine.variant,))
        if self.engine is not None:
            nx, ny, nz = self.dims
            shapes = {'tsum': (nz, ny, nx), 'w': (nz, ny, nx), 'csum': (3, nz, ny, nx), 'cw': (nz, ny, nx)}
            self._state = {k: torch.zeros(shapes[k], dtype=torch.float32, device=self.engine.device)
                           for k in (('tsum', 'w', 'csum', 'cw') if self.colour else ('tsum', 'w'))}
        else:
            self._state = zero_state(self.dims, self.colour)

    def integrate(self, depth, imgs, poses, Ks, views=None):
        """adds the views [v0, v1) (None: all) of depth [n,h,w], imgs [n,3,h,w] in [0,1], poses [n,3,4], Ks [n,3,3]; returns self"""
        if self.engine is not None:
            self.engine.tsdf_integrate(self._state, self.origin, self.voxel_size, self.trunc, self.dims, _geo._depth3(torch.as_tensor(depth)),
                                       imgs, poses, Ks, views)
        else:
            new = integrate_numpy(_geo._depth3(_geo._host(depth)), _geo._host(imgs) if self.colour else None, _geo._host(poses), _geo._host(Ks),
                                  self.origin, self.voxel_size, self.dims, self.trunc, views, self._state, self.colour, np.float32)
            self._state = {k: new[k] for k in self._state}
        return self

    def state(self):
        """dict(tsum, w [nz,ny,nx] and, with colour, csum [3,nz,ny,nx], cw): the sums themselves (device tensors or numpy arrays), not copies"""
        return self._state

    def tsdf(self):
        """f = Tsum / W [nz,ny,nx], NaN where no view has reached the lattice point"""
        s = self._state
        if self.engine is not None:
            return torch.where(s['w'] > 0, s['tsum'] / s['w'], torch.full_like(s['w'], float('nan')))
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(s['w'] > 0, s['tsum'] / s['w'], np.float32('nan'))

    def extract(self, min_weight=1):
        """-> dict(vertices [m,3] float32, faces [k,3] int32, colors [m,3] in [0,1], normals [m,3]); one read-back (the two totals)"""
        if not min_weight > 0:
            raise ValueError("neuray_amd.mesh: min_weight must be positive")
        s = self._state
        if self.engine is not None:
            cells = self.engine.surface_cells(s, self.dims, min_weight)
            return self.engine.surface_emit(s, self.origin, self.voxel_size, self.dims, cells)
        ref = surface_nets_numpy(s['tsum'], s['w'], s.get('csum'), s.get('cw'), self.origin, self.voxel_size, min_weight, np.float32)
        return {k: ref[k] for k in ('vertices', 'faces', 'colors', 'normals')}

    def field(self, min_weight=1):
        """f = Tsum / W [nz,ny,nx] float32, NaN where W < min_weight: the ray caster's field (one elementwise pass)"""
        if not min_weight > 0:
            raise ValueError("neuray_amd.mesh: min_weight must be positive")
        s = self._state
        if self.engine is not None:
            return torch.where(s['w'] >= float(min_weight), s['tsum'] / s['w'], torch.full_like(s['w'], float('nan')))
        return field_numpy(s['tsum'], s['w'], min_weight)

    def raycast(self, poses, Ks, h, w, min_weight=1, step=0.5, depth_range=None, skip=True):
        """The volume seen from the cameras poses [n,3,4], Ks [n,3,3] at h x w pixels -> dict(depth [n,h,w] float32 z-depth, 0 = none;
        normal [n,3,h,w] unit, towards free space; colors [n,3,h,w] in [0,1]; status [n,h,w] uint8: 0 nothing, 1 hit, 2 the surface seen
        from behind; evaluated [n,h,w] int32).  step: the sample spacing in voxels, 0 < step <= 0.95; depth_range [n,2]: near, far per view
        (default [0, inf)); skip: skip the blocks of 8 x 8 x 8 cells away from the surface (changes no bit of the other outputs).  Device
        tensors where the volume lives on the device (no host synchronisation with host cameras), the float32 reference otherwise."""
        f = self.field(min_weight)
        s = self._state
        nx, ny, nz = self.dims
        n = int(np.asarray(poses).reshape(-1, 3, 4).shape[0]) if not torch.is_tensor(poses) else int(poses.reshape(-1, 3, 4).shape[0])
        _check_raycast((nz, ny, nx), self.voxel_size, int(h), int(w), step, n, None if torch.is_tensor(depth_range) else depth_range, None)
        if self.engine is not None:
            blocks = self.engine.surface_blocks(self.engine.surface_cells(s, self.dims, min_weight), self.dims) if skip else None
            state = {'f': f, 'csum': s.get('csum'), 'cw': s.get('cw')}
            return self.engine.tsdf_raycast(state, self.origin, self.voxel_size, self.dims, poses, Ks, h, w, step, depth_range, blocks,
                                            ('depth', 'normal', 'colors', 'status', 'evaluated'))
        blocks = blocks_numpy(cells_numpy(s['tsum'], s['w'], min_weight, np.float32)[0]) if skip else None
        return raycast_numpy(f, s.get('csum'), s.get('cw'), self.origin, self.voxel_size, poses, Ks, h, w, step, depth_range, np.float32, blocks)


def raycast_views(volume, database, ids, min_weight=1, step=0.5):
    """The volume seen from the database's views `ids` -> geometry.database_depth_maps' dictionary with
    the ray-cast depth as an imgs_info has it: dict(depth [n,1,h,w], imgs [n,3,h,w] (the ray-cast colours), poses [n,3,4], Ks [n,3,3]) as
    float32 numpy arrays, and normal [n,3,h,w], status [n,h,w]: what filter_depth, fuse_points, a DepthInitNet or a comparison with
    database_depth_maps take."""
    maps = _geo.database_depth_maps(database, ids)
    n, h, w = maps['depth'].shape
    out = volume.raycast(maps['poses'], maps['Ks'], h, w, min_weight, step)
    out = {k: _geo._host(v) for k, v in out.items()}
    return {'depth': np.ascontiguousarray(out['depth'][:, None], np.float32), 'imgs': np.ascontiguousarray(out['colors'], np.float32),
            'poses': maps['poses'], 'Ks': maps['Ks'], 'normal': np.ascontiguousarray(out['normal'], np.float32), 'status': out['status']}


def depth_bounds(depth, poses, Ks):
    """the box (lo [3], hi [3]) of the unprojected valid depths, or None where no pixel has depth"""
    depth = torch.as_tensor(depth).detach()
    depth = _geo._depth3(depth).float()
    n, h, w = depth.shape
    dev = depth.device
    P, _, Ki = _geo._host_cameras(poses, Ks)
    P, Ki = P.to(dev), Ki.to(dev)
    ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1).float()
    lo, hi = None, None
    for i in range(n):
        have = depth[i] > 0
        if not bool(have.any()):
            continue
        cam = (pix[have] @ Ki[i].T) * depth[i][have][:, None]
        world = (cam - P[i, :, 3]) @ P[i, :, :3]              # R^T (K^-1 [x,y,1] d - t)
        a, b = world.min(0).values.cpu(), world.max(0).values.cpu()
        lo, hi = (a, b) if lo is None else (torch.minimum(lo, a), torch.maximum(hi, b))
    return None if lo is None else (lo.numpy().astype(np.float64), hi.numpy().astype(np.float64))


def fuse_mesh(depth, imgs, poses, Ks, voxel_size=None, bounds=None, trunc=None, filter=True, src=8, tau_px=1.0, tau_d=0.01, min_views=2,
              min_weight=1, engine=None):
    """Depth maps [n,h,w] and images [n,3,h,w] (in [0,1]) of posed views -> dict(vertices, faces, colors, normals, volume: the TSDFVolume).
    filter: geometry.filter_depth first (src, tau_px, tau_d, min_views).  bounds (lo [3], hi [3]): default the box of the unprojected valid
    depths padded by trunc; voxel_size: default 256 lattice points on the longest side of the box."""
    if filter:
        depth = _geo.filter_depth(depth, poses, Ks, src=src, tau_px=tau_px, tau_d=tau_d, min_views=min_views, engine=engine)['depth']
    pad = bounds is None
    if bounds is None:
        bounds = depth_bounds(depth, poses, Ks)
        if bounds is None:
            raise ValueError("neuray_amd.mesh: no pixel has depth%s: nothing to bound the volume with" % (' after the filter' if filter else ''))
    lo, hi = np.asarray(bounds[0], np.float64).reshape(3), np.asarray(bounds[1], np.float64).reshape(3)
    if not np.all(hi > lo):
        raise ValueError("neuray_amd.mesh: empty bounds %r .. %r" % (lo, hi))
    if voxel_size is None:
        side = float((hi - lo).max())
        if pad:                                            # the padded box has 256 points on its longest side
            voxel_size = side / (255 - 2 * 3) if trunc is None else (side + 2 * float(trunc)) / 255
        else:
            voxel_size = side / 255
    voxel_size = float(voxel_size)
    trunc = 3.0 * voxel_size if trunc is None else float(trunc)
    if pad:
        lo, hi = lo - trunc, hi + trunc
    dims = tuple(max(2, int(np.ceil((hi[k] - lo[k]) / voxel_size - 1e-9)) + 1) for k in range(3))
    vol = TSDFVolume(lo, voxel_size, dims, trunc, colour=imgs is not None, engine=engine)
    vol.integrate(depth, imgs, poses, Ks)
    out = vol.extract(min_weight)
    out['volume'] = vol
    return out


# ---- files -----------------------------------------------------------------------------------------------------------------------------
_FACE_DTYPE = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])


def write_mesh_ply(path, vertices, faces, colors=None, normals=None):
    """binary little-endian PLY: geometry.write_ply's vertex record (x y z nx ny nz float, red green blue uchar) plus `element face` with
    `property list uchar int vertex_indices`"""
    faces = np.asarray(_geo._host(faces)).astype('<i4').reshape(-1, 3)
    m = _geo._host(vertices).reshape(-1, 3).shape[0]
    if faces.size and (faces.min() < 0 or faces.max() >= m):
        raise ValueError("neuray_amd.mesh: a face names vertex %d of %d" % (int(faces.max() if faces.max() >= m else faces.min()), m))
    _geo.write_ply(path, vertices, colors, normals)
    with open(path, 'rb') as f:
        data = f.read()
    mark = b'end_header\n'
    head, body = data[:data.index(mark)], data[data.index(mark) + len(mark):]
    rec = np.zeros(faces.shape[0], _FACE_DTYPE)
    rec['n'], rec['v'] = 3, faces
    with open(path, 'wb') as f:
        f.write(head + ('element face %d\nproperty list uchar int vertex_indices\n' % faces.shape[0]).encode('ascii') + mark + body)
        f.write(rec.tobytes())


def read_mesh_ply(path):
    """what write_mesh_ply wrote -> dict(vertices [m,3] float32, normals [m,3] float32, colors [m,3] uint8, faces [k,3] int32)"""
    with open(path, 'rb') as f:
        lines = []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("neuray_amd.mesh: %s: no end_header" % path)
            lines.append(line.decode('ascii').strip())
            if lines[-1] == 'end_header':
                break
        if lines[0] != 'ply' or lines[1] != 'format binary_little_endian 1.0':
            raise ValueError("neuray_amd.mesh: %s is not a binary little-endian PLY" % path)
        elements = [ln.split()[1:] for ln in lines if ln.startswith('element')]
        if [e[0] for e in elements] != ['vertex', 'face']:
            raise ValueError("neuray_amd.mesh: %s: elements %r (vertex, face)" % (path, elements))
        props = [tuple(ln.split()[1:]) for ln in lines if ln.startswith('property')]
        want = [('float', f_) for f_ in _geo._PLY_FIELDS] + [('uchar', c) for c in ('red', 'green', 'blue')] + [('list', 'uchar', 'int', 'vertex_indices')]
        if props != want:
            raise ValueError("neuray_amd.mesh: %s: unexpected properties %r" % (path, props))
        m, k = int(elements[0][1]), int(elements[1][1])
        vdata, fdata = f.read(m * _geo._PLY_DTYPE.itemsize), f.read(k * _FACE_DTYPE.itemsize)
        if len(vdata) != m * _geo._PLY_DTYPE.itemsize or len(fdata) != k * _FACE_DTYPE.itemsize:
            raise ValueError("neuray_amd.mesh: %s: truncated" % path)
    rec, frec = np.frombuffer(vdata, _geo._PLY_DTYPE), np.frombuffer(fdata, _FACE_DTYPE)
    if k and not np.all(frec['n'] == 3):
        raise ValueError("neuray_amd.mesh: %s: a face is not a triangle" % path)
    return {'vertices': np.stack([rec[f_] for f_ in _geo._PLY_FIELDS[:3]], -1), 'normals': np.stack([rec[f_] for f_ in _geo._PLY_FIELDS[3:]], -1),
            'colors': np.stack([rec['red'], rec['green'], rec['blue']], -1), 'faces': frec['v'].astype(np.int32).reshape(-1, 3)}
