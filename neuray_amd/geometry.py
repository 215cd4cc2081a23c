"""Geometry export: depth-map consistency filter and point-cloud fusion.

Per-view depth maps - a database's, or `render_depth_fine` of a renderer - become a filtered depth map per view and one coloured, oriented
point cloud.  The cross-view test at its core is NeuRay's notion of visibility: a point seen by view i is visible, occluded or unseen in view j
according to j's depth map.  `consistency_numpy` / `fuse_numpy` restate the formulas vectorised in float64 or float32 (the reference of the
tests and the path of a machine without a GPU, like procedural.render_numpy); csrc/nr_kernels_fuse.h through
`RenderEngine.depth_consistency` / `RenderEngine.fuse_view` evaluates the same operations in fp32 on the device.

Pixel centres sit at integer coordinates (oracle.coords2rays, the procedural ray caster); depth is the z-depth of depth2points, 0 = none.
For pixel (x, y) of view i with d = D_i[y,x] > 0 and source slot s, j = nn_ids[i][s] (-1 or i itself: an unused slot):
  Xw = R_i^T (K_i^-1 [x,y,1]^T d - t_i);  Pc = R_j Xw + t_j, z = Pc.z, q = K_j Pc, u = q.x / q.z, v = q.y / q.z
  un = floor(u + 0.5), vn = floor(v + 0.5)            the NEAREST texel: a depth interpolated across a silhouette is a surface that does not exist
  seen        z > 0, 0 <= un < w, 0 <= vn < h, d_j = D_j[vn,un] > 0
  Yw = R_j^T (K_j^-1 [un,vn,1]^T d_j - t_j);  Qc = R_i Yw + t_i, q' = K_i Qc
  e_px^2 = (q'.x / q'.z - x)^2 + (q'.y / q'.z - y)^2,  e_d = |Qc.z - d| / d
  consistent  seen, Qc.z > 0, e_px^2 < tau_px^2, e_d < tau_d
  occluded    seen, not consistent, (z - d_j) / d_j > tau_d                      the source sees a nearer surface
  fused_depth = (d + sum of Qc.z over the consistent slots, in slot order) / (1 + count)
Fusion, the views in ascending order: a pixel is kept where count >= min_views and emitted where it is kept and nobody has taken it; an
emitted pixel takes the texel it was consistent with in every such source view.  Its point is the world point of fused_depth, its colour the
mean of its own and the consistent source texels' colours, its normal the cross product of the x and y differences of the camera-space
points of fused_depth (central where both neighbours are kept and within tau_n * fused_depth, one-sided where one is, zero otherwise),
facing the camera."""
import numpy as np
import torch

from . import procedural as _proc

MAX_SRC = 16
DEFAULTS = {'tau_px': 1.0, 'tau_d': 0.01, 'min_views': 2, 'tau_n': 0.05, 'src': 8}


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _unproject(Rt, Ki, px, py, d):
    """R^T (K^-1 [px,py,1]^T d - t), in the kernel's order of operations"""
    a = [(Ki[k, 0] * px + Ki[k, 1] * py + Ki[k, 2]) * d - Rt[k, 3] for k in range(3)]
    return [Rt[0, c] * a[0] + Rt[1, c] * a[1] + Rt[2, c] * a[2] for c in range(3)]


def _project(Rt, K, X):
    """-> u, v, z of K (R X + t)"""
    c = [Rt[k, 0] * X[0] + Rt[k, 1] * X[1] + Rt[k, 2] * X[2] + Rt[k, 3] for k in range(3)]
    q = [K[k, 0] * c[0] + K[k, 1] * c[1] + K[k, 2] * c[2] for k in range(3)]
    with np.errstate(divide='ignore', invalid='ignore'):
        return q[0] / q[2], q[1] / q[2], c[2]


def _cameras(poses, Ks, T):
    poses = np.asarray(poses, np.float32).reshape(-1, 3, 4)
    Ks = np.asarray(Ks, np.float32).reshape(-1, 3, 3)
    return poses.astype(T), Ks.astype(T), _proc._inverse(Ks, T).astype(T)


def _check_table(nn_ids, n):
    nn_ids = np.asarray(nn_ids).astype(np.int64).reshape(n, -1)
    if not 1 <= nn_ids.shape[1] <= MAX_SRC:
        raise ValueError("neuray_amd.geometry: %d source slots (1 .. %d)" % (nn_ids.shape[1], MAX_SRC))
    return nn_ids


def _used(j, i, n):
    return 0 <= j < n and j != i


def consistency_numpy(depth, poses, Ks, nn_ids, tau_px=1.0, tau_d=0.01, dtype=np.float64, details=False):
    """-> dict(count [n,h,w] uint8, fused_depth [n,h,w] dtype, consistent_bits / occluded_bits [n,h,w] int32, src_texel [n,S,h,w] int32) and,
    with details, per (view, slot, pixel) [n,S,h,w]: 'valid' (the slot is used and the pixel has depth), u, v, z, e_px (its root), e_d,
    occ (= (z - d_j) / d_j) - what decides whether a pair is near a threshold."""
    if not (tau_px > 0 and tau_d > 0):
        raise ValueError("neuray_amd.geometry: thresholds must be positive")
    T = np.dtype(dtype).type
    depth = np.asarray(depth, np.float32)
    n, h, w = depth.shape
    D = depth.astype(T)
    P, K, Ki = _cameras(poses, Ks, T)
    nn_ids = _check_table(nn_ids, n)
    S = nn_ids.shape[1]
    tau_px2, tau_dT = T(np.float32(tau_px)) * T(np.float32(tau_px)), T(np.float32(tau_d))
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    fx, fy = xs.astype(T), ys.astype(T)
    out = {'count': np.zeros((n, h, w), np.uint8), 'fused_depth': np.zeros((n, h, w), T), 'consistent_bits': np.zeros((n, h, w), np.int32),
           'occluded_bits': np.zeros((n, h, w), np.int32), 'src_texel': np.full((n, S, h, w), -1, np.int32)}
    det = {k: np.zeros((n, S, h, w), np.float64) for k in ('u', 'v', 'z', 'e_px', 'e_d', 'occ')} if details else None
    if details:
        det['valid'] = np.zeros((n, S, h, w), bool)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i in range(n):
            d = D[i]
            have = d > 0
            X = _unproject(P[i], Ki[i], fx, fy, d)
            acc, count = d.copy(), np.zeros((h, w), np.int64)
            for s in range(S):
                j = int(nn_ids[i, s])
                if not _used(j, i, n):
                    continue
                u, v, z = _project(P[j], K[j], X)
                un, vn = np.floor(u + T(0.5)), np.floor(v + T(0.5))
                inb = have & (z > 0) & (un >= 0) & (un < w) & (vn >= 0) & (vn < h)
                t = np.where(inb, vn, 0).astype(np.int64) * w + np.where(inb, un, 0).astype(np.int64)
                dj = np.where(inb, D[j].reshape(-1)[t], T(0))
                seen = inb & (dj > 0)
                Y = _unproject(P[j], Ki[j], un, vn, dj)
                u2, v2, qz = _project(P[i], K[i], Y)
                du, dv = u2 - fx, v2 - fy
                e_px2 = du * du + dv * dv
                e_d = np.abs(qz - d) / d
                ok = seen & (qz > 0) & (e_px2 < tau_px2) & (e_d < tau_dT)
                occ_ratio = (z - dj) / dj
                hidden = seen & ~ok & (occ_ratio > tau_dT)
                acc = np.where(ok, acc + qz, acc)
                count += ok
                out['consistent_bits'][i] |= ok.astype(np.int32) << s
                out['occluded_bits'][i] |= hidden.astype(np.int32) << s
                out['src_texel'][i, s] = np.where(seen, t, -1)
                if details:
                    det['valid'][i, s] = have
                    for k, a in (('u', u), ('v', v), ('z', z), ('e_px', np.sqrt(e_px2)), ('e_d', e_d), ('occ', occ_ratio)):
                        det[k][i, s] = a
            out['count'][i] = count
            out['fused_depth'][i] = np.where(have, acc / (count + 1).astype(T), T(0))
    if details:
        out.update(det)
    return out


def _popcount(bits, S):
    return sum(((bits >> s) & 1) for s in range(S)).astype(np.int64)


def _cam_point(Ki, px, py, fd):
    return [(Ki[k, 0] * px + Ki[k, 1] * py + Ki[k, 2]) * fd for k in range(3)]


def fuse_numpy(depth, imgs, poses, Ks, nn_ids, consistent_bits, src_texel, min_views=2, tau_n=0.05, dedup=True, dtype=np.float64,
               fused_depth=None):
    """The fusion given the consistency result (bits and texels: from there on emit / taken are integer logic) -> dict(emit [n,h,w] uint8,
    taken [n,h,w] uint8 (the masks after the last view), fused_depth [n,h,w], xyz / colour / normal [n,h,w,3] dtype (zero where not emitted),
    cross_rel [n,h,w]: |dx x dy| / (|dx| |dy|) of the normal's two differences, 0 where there is no normal).  fused_depth: taken as given,
    or recomputed here from depth, bits and texels."""
    if min_views < 1 or not tau_n > 0:
        raise ValueError("neuray_amd.geometry: min_views >= 1 and tau_n > 0")
    T = np.dtype(dtype).type
    depth = np.asarray(depth, np.float32)
    n, h, w = depth.shape
    D = depth.astype(T)
    rgb = np.asarray(imgs, np.float32).reshape(n, 3, h * w).astype(T)
    P, K, Ki = _cameras(poses, Ks, T)
    nn_ids = _check_table(nn_ids, n)
    S = nn_ids.shape[1]
    bits, texel = np.asarray(consistent_bits).astype(np.int64), np.asarray(src_texel).astype(np.int64)
    count = _popcount(bits, S)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    fx, fy = xs.astype(T), ys.astype(T)
    if fused_depth is None:
        fd_all = np.zeros((n, h, w), T)
        for i in range(n):
            acc = D[i].copy()
            for s in range(S):
                j = int(nn_ids[i, s])
                ok = ((bits[i] >> s) & 1) > 0
                if not _used(j, i, n) or not ok.any():
                    continue
                t = np.where(ok, texel[i, s], 0)
                Y = _unproject(P[j], Ki[j], (t % w).astype(T), (t // w).astype(T), np.where(ok, D[j].reshape(-1)[t], T(0)))
                acc = np.where(ok, acc + _project(P[i], K[i], Y)[2], acc)
            fd_all[i] = np.where(D[i] > 0, acc / (count[i] + 1).astype(T), T(0))
    else:
        fd_all = np.asarray(fused_depth).astype(T)
    tau_nT = T(np.float32(tau_n))
    kept_all = count >= min_views
    taken = np.zeros((n, h * w), np.uint8)
    out = {'emit': np.zeros((n, h, w), np.uint8), 'fused_depth': fd_all, 'cross_rel': np.zeros((n, h, w), np.float64)}
    for k in ('xyz', 'colour', 'normal'):
        out[k] = np.zeros((n, h, w, 3), T)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i in range(n):
            kept, fd = kept_all[i], fd_all[i]
            emit = kept & (taken[i].reshape(h, w) == 0) if dedup else kept.copy()
            col = [rgb[i, c].reshape(h, w).copy() for c in range(3)]
            for s in range(S):
                j = int(nn_ids[i, s])
                on = emit & (((bits[i] >> s) & 1) > 0) & (texel[i, s] >= 0)
                if not _used(j, i, n) or not on.any():
                    continue
                t = texel[i, s][on]
                if dedup:
                    taken[j][t] = 1
                for c in range(3):
                    col[c][on] = col[c][on] + rgb[j, c][t]
            m = (count[i] + 1).astype(T)
            out['emit'][i] = emit
            xyz = _unproject(P[i], Ki[i], fx, fy, fd)
            a = _cam_point(Ki[i], fx, fy, fd)
            lim = tau_nT * fd

            def shifted(arr, dy, dx):             # arr[y + dy, x + dx], the pixel's own value beyond the edge
                o = arr.copy()
                ys_, xs_ = slice(max(-dy, 0), h - max(dy, 0)), slice(max(-dx, 0), w - max(dx, 0))
                yd_, xd_ = slice(max(dy, 0), h - max(-dy, 0)), slice(max(dx, 0), w - max(-dx, 0))
                o[ys_, xs_] = arr[yd_, xd_]
                return o

            def side(dy, dx):                     # (qualifies, camera-space point) of the neighbour at (y + dy, x + dx)
                inside = (ys + dy >= 0) & (ys + dy < h) & (xs + dx >= 0) & (xs + dx < w)
                f = shifted(fd, dy, dx)
                q = inside & shifted(kept, dy, dx) & (np.abs(f - fd) < lim)
                pt = _cam_point(Ki[i], fx + T(dx), fy + T(dy), f)
                return q, [np.where(q, pt[k], a[k]) for k in range(3)]
            ql, pl = side(0, -1)
            qr, pr = side(0, 1)
            qu, pu = side(-1, 0)
            qd, pd = side(1, 0)
            dxv, dyv = [pr[k] - pl[k] for k in range(3)], [pd[k] - pu[k] for k in range(3)]
            c = [dxv[1] * dyv[2] - dxv[2] * dyv[1], dxv[2] * dyv[0] - dxv[0] * dyv[2], dxv[0] * dyv[1] - dxv[1] * dyv[0]]
            len2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
            has = (ql | qr) & (qu | qd) & (len2 > 0)
            ln = np.sqrt(len2)
            flip = (c[0] * a[0] + c[1] * a[1] + c[2] * a[2]) > 0
            c = [np.where(flip, -c[k], c[k]) / ln for k in range(3)]
            nw = [P[i][0, k] * c[0] + P[i][1, k] * c[1] + P[i][2, k] * c[2] for k in range(3)]
            prod = np.sqrt(sum(v * v for v in dxv).astype(np.float64)) * np.sqrt(sum(v * v for v in dyv).astype(np.float64))
            out['cross_rel'][i] = np.where(has & emit & (prod > 0), ln.astype(np.float64) / np.where(prod > 0, prod, 1.0), 0.0)
            for k in range(3):
                out['xyz'][i, ..., k] = np.where(emit, xyz[k], T(0))
                out['colour'][i, ..., k] = np.where(emit, col[k] / m, T(0))
                out['normal'][i, ..., k] = np.where(emit & has, nw[k], T(0))
    out['taken'] = taken.reshape(n, h, w)
    return out


# ---- the public surface --------------------------------------------------------------------------------------------------------------
def nearest_sources(poses, src=8):
    """the `src` nearest other cameras of every camera (pipeline.nearest_view_table, self excluded), padded with -1 -> [n,S] int32"""
    from .pipeline import nearest_view_table
    poses = np.asarray(poses, np.float32).reshape(-1, 3, 4)
    n = poses.shape[0]
    src = max(1, min(int(src), MAX_SRC))
    order = nearest_view_table(poses, poses)
    table = np.full((n, src), -1, np.int32)
    for i in range(n):
        others = [int(j) for j in order[i] if int(j) != i][:src]
        table[i, :len(others)] = others
    return table


def _engine(engine):
    return engine if engine is not None else _proc._device_engine()


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _host_cameras(poses, Ks):
    from .engine import host_inverse
    Ks = torch.as_tensor(_host(Ks), dtype=torch.float32).reshape(-1, 3, 3)
    return torch.as_tensor(_host(poses), dtype=torch.float32).reshape(-1, 3, 4), Ks, host_inverse(Ks)


def _depth3(depth):
    return depth[:, 0] if depth.ndim == 4 else depth


def filter_depth(depth, poses, Ks, nn_ids=None, src=8, tau_px=1.0, tau_d=0.01, min_views=2, engine=None):
    """Depth maps [n,h,w] of posed views -> dict of tensors: 'depth' (fused_depth where at least min_views sources agree, else 0), 'count',
    'consistent_bits', 'occluded_bits'.  nn_ids=None: the `src` nearest other cameras.  On the device when there is one (or `engine` is
    given), through consistency_numpy otherwise."""
    if min_views < 1:
        raise ValueError("neuray_amd.geometry: min_views >= 1")
    nn_ids = nearest_sources(_host(poses), src) if nn_ids is None else nn_ids
    eng = _engine(engine)
    if eng is not None:
        t_poses, t_Ks, t_Ki = _host_cameras(poses, Ks)
        res = eng.depth_consistency(_depth3(torch.as_tensor(depth)), t_poses, t_Ks, nn_ids, tau_px, tau_d, Ks_inv=t_Ki)
    else:
        ref = consistency_numpy(_depth3(_host(depth)), _host(poses), _host(Ks), _host(nn_ids), tau_px, tau_d, dtype=np.float32)
        res = {k: torch.from_numpy(ref[k]) for k in ('count', 'fused_depth', 'consistent_bits', 'occluded_bits')}
    kept = res['count'] >= min_views
    return {'depth': torch.where(kept, res['fused_depth'], torch.zeros_like(res['fused_depth'])), 'count': res['count'],
            'consistent_bits': res['consistent_bits'], 'occluded_bits': res['occluded_bits']}


def fuse_points(depth, imgs, poses, Ks, nn_ids=None, src=8, tau_px=1.0, tau_d=0.01, min_views=2, tau_n=0.05, dedup=True, engine=None):
    """Depth maps [n,h,w] and images [n,3,h,w] (in [0,1]) of posed views -> dict of tensors: points [m,3], colors [m,3], normals [m,3]
    (zero where there is none), view [m] and pixel [m] (= y * w + x) int64, ordered by (view, row, column).  One read-back (m: the
    compaction is a boolean mask)."""
    nn_ids = nearest_sources(_host(poses), src) if nn_ids is None else nn_ids
    eng = _engine(engine)
    if eng is not None:
        t_poses, t_Ks, t_Ki = _host_cameras(poses, Ks)
        dev = eng.device
        t_depth = eng._f32(_depth3(torch.as_tensor(depth)))
        t_imgs = eng._f32(torch.as_tensor(imgs))
        t_poses, t_Ks, t_Ki = t_poses.to(dev), t_Ks.to(dev), t_Ki.to(dev)
        t_nn = torch.as_tensor(nn_ids).to(device=dev, dtype=torch.int32).contiguous()
        cons = eng.depth_consistency(t_depth, t_poses, t_Ks, t_nn, tau_px, tau_d, Ks_inv=t_Ki, outputs=('count', 'fused_depth', 'consistent_bits'))
        n, h, w = t_depth.shape
        taken = torch.zeros(n, h, w, dtype=torch.uint8, device=dev) if dedup else None
        views = [eng.fuse_view(i, t_depth, t_imgs, t_poses, t_Ks, t_nn, cons, taken, min_views, tau_n, Ks_inv=t_Ki) for i in range(n)]
        emit = torch.stack([v['emit'] for v in views]) > 0
        xyz, col, nrm = (torch.stack([v[k] for v in views]) for k in ('xyz', 'colour', 'normal'))
    else:
        d, p, k, t = _depth3(_host(depth)), _host(poses), _host(Ks), _host(nn_ids)
        cons = consistency_numpy(d, p, k, t, tau_px, tau_d, dtype=np.float32)
        ref = fuse_numpy(d, _host(imgs), p, k, t, cons['consistent_bits'], cons['src_texel'], min_views, tau_n, dedup, dtype=np.float32,
                         fused_depth=cons['fused_depth'])
        emit = torch.from_numpy(ref['emit'] > 0)
        xyz, col, nrm = (torch.from_numpy(ref[k_]) for k_ in ('xyz', 'colour', 'normal'))
        n, h, w = emit.shape
    flat = emit.reshape(-1)
    index = torch.nonzero(flat)[:, 0]
    return {'points': xyz.reshape(-1, 3)[flat], 'colors': col.reshape(-1, 3)[flat], 'normals': nrm.reshape(-1, 3)[flat],
            'view': index // (h * w), 'pixel': index % (h * w)}


# ---- files -----------------------------------------------------------------------------------------------------------------------------
_PLY_FIELDS = ('x', 'y', 'z', 'nx', 'ny', 'nz')
_PLY_DTYPE = np.dtype([(f, '<f4') for f in _PLY_FIELDS] + [(c, 'u1') for c in ('red', 'green', 'blue')])


def write_ply(path, points, colors=None, normals=None):
    """binary little-endian PLY with x y z nx ny nz (float) red green blue (uchar); colors in [0,1] (floats) or uint8"""
    pts = _host(points).reshape(-1, 3)
    m = pts.shape[0]
    rec = np.zeros(m, _PLY_DTYPE)
    nrm = np.zeros((m, 3), np.float32) if normals is None else _host(normals).reshape(m, 3)
    for k in range(3):
        rec[_PLY_FIELDS[k]], rec[_PLY_FIELDS[3 + k]] = pts[:, k], nrm[:, k]
    if colors is not None:
        c = _host(colors).reshape(m, 3)
        if c.dtype != np.uint8:
            c = np.clip(c * 255, 0, 255).astype(np.uint8)              # (color_map_backward)
        rec['red'], rec['green'], rec['blue'] = c[:, 0], c[:, 1], c[:, 2]
    else:
        rec['red'] = rec['green'] = rec['blue'] = 255
    header = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % m] + ['property float %s' % f for f in _PLY_FIELDS] + \
        ['property uchar %s' % c for c in ('red', 'green', 'blue')] + ['end_header']
    with open(path, 'wb') as f:
        f.write(('\n'.join(header) + '\n').encode('ascii'))
        f.write(rec.tobytes())


def read_ply(path):
    """what write_ply wrote -> dict(points [m,3] float32, normals [m,3] float32, colors [m,3] uint8)"""
    with open(path, 'rb') as f:
        lines = []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("neuray_amd.geometry: %s: no end_header" % path)
            lines.append(line.decode('ascii').strip())
            if lines[-1] == 'end_header':
                break
        if lines[0] != 'ply' or lines[1] != 'format binary_little_endian 1.0':
            raise ValueError("neuray_amd.geometry: %s is not a binary little-endian PLY" % path)
        m = [int(ln.split()[2]) for ln in lines if ln.startswith('element vertex')][0]
        props = [tuple(ln.split()[1:]) for ln in lines if ln.startswith('property')]
        if props != [('float', f_) for f_ in _PLY_FIELDS] + [('uchar', c) for c in ('red', 'green', 'blue')]:
            raise ValueError("neuray_amd.geometry: %s: unexpected properties %r" % (path, props))
        data = f.read(m * _PLY_DTYPE.itemsize)
        if len(data) != m * _PLY_DTYPE.itemsize:
            raise ValueError("neuray_amd.geometry: %s: truncated" % path)
    rec = np.frombuffer(data, _PLY_DTYPE)
    return {'points': np.stack([rec[k] for k in _PLY_FIELDS[:3]], -1), 'normals': np.stack([rec[k] for k in _PLY_FIELDS[3:]], -1),
            'colors': np.stack([rec['red'], rec['green'], rec['blue']], -1)}


# ---- where the depth maps come from ------------------------------------------------------------------------------------------------------
def database_depth_maps(database, ids):
    """the database's own depth maps -> dict(depth [n,h,w], imgs [n,3,h,w] in [0,1], poses [n,3,4], Ks [n,3,3]) as float32 numpy arrays"""
    from .pipeline import build_imgs_info
    info = build_imgs_info(database, list(ids))
    return {'depth': np.ascontiguousarray(info['depth'][:, 0]), 'imgs': np.ascontiguousarray(info['imgs'], dtype=np.float32), 'poses': info['poses'],
            'Ks': info['Ks']}


def render_depth_maps(renderer, database, ids, work_num=8, pad_interval=16):
    """Every view of `ids` rendered from its nearest OTHER views, its depth read from 'render_depth_fine' (or 'render_depth') ->
    database_depth_maps' dictionary with the rendered depth (the images stay the database's) and 'working_ids' (a generalisation renderer:
    the views each image was rendered from).  A generalisation renderer takes its working views from the database
    (select_working_views_db, exclude_self); a fine-tuning renderer goes through its render_pose, which skips the nearest of its own views."""
    from . import pipeline
    out = database_depth_maps(database, ids)
    dev = next(renderer.parameters()).device
    n, h, w = out['depth'].shape
    had = renderer.cfg.get('render_depth', False)
    renderer.cfg['render_depth'] = True
    depth, working = [], []
    try:
        cache = pipeline.DeviceViewCache(database, dev, pad_interval) if not hasattr(renderer, 'render_pose') else None
        for i, view_id in enumerate(ids):
            que = pipeline.build_render_imgs_info(out['poses'][i], out['Ks'][i], (h, w), database.get_depth_range(view_id))
            que.pop('shape')
            que = {k: torch.from_numpy(v).to(dev) for k, v in que.items()}
            with torch.no_grad():
                if cache is None:
                    res = renderer.render_pose(que)
                else:
                    pool = [v for v in database.get_img_ids() if v != view_id]          # self is never a working view, whatever the distances
                    work = pipeline.select_working_views_db(database, pool, out['poses'][i:i + 1], work_num)[0]
                    working.append(list(work))
                    res = renderer({'que_imgs_info': que, 'ref_imgs_info': cache.imgs_info(list(work)), 'eval': True})
            rd = res['render_depth_fine'] if 'render_depth_fine' in res else res['render_depth']
            depth.append(rd.reshape(h, w).float())
    finally:
        renderer.cfg['render_depth'] = had
    out['depth'] = torch.stack(depth).cpu().numpy()
    if working:
        out['working_ids'] = working
    return out


# ---- ground truth ------------------------------------------------------------------------------------------------------------------------
def surface_distance(scene, points):
    """Distance of points [m,3] to a procedural scene: min over the packed primitives of |sdf_k(x)|, with the sphere's and the box's signed
    distance functions -> [m] float64.  Where primitives intersect, part of a primitive's surface lies inside another one and is not
    visible: this is a LOWER bound of the distance to the visible surface, and equal to it wherever the nearest surface point is visible."""
    scene = np.asarray(_host(scene), np.float64)
    x = np.asarray(_host(points), np.float64).reshape(-1, 3)
    best = np.full(x.shape[0], np.inf)
    for i in range(_proc.scene_prims(scene)):
        P = scene[_proc.HEADER + _proc.PRIM * i: _proc.HEADER + _proc.PRIM * (i + 1)]
        q = x - P[1:4]
        if P[0] == _proc.SPHERE:
            sdf = np.linalg.norm(q, axis=1) - P[4]
        else:
            a = np.abs(q) - P[4:7]
            sdf = np.linalg.norm(np.maximum(a, 0.0), axis=1) + np.minimum(a.max(1), 0.0)
        best = np.minimum(best, np.abs(sdf))
    return best
