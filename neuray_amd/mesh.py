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
end is inside, reversed otherwise; its triangles are (v0, v1, v2) and (v0, v2, v3); faces are ordered by owner cell, then axis."""
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
