"""Plane-sweep stereo: per-view depth maps from posed images.

Images + cameras + a depth range per view -> a depth map per view: the photometric stage that the databases of real scenes take from an
external dense-stereo tool (their colmap_depth/<id>.jpg.geometric.bin files).  `plane_sweep_numpy` is the definition - the reference of the
tests, the path of a machine without a GPU and the place where every constant is pinned; csrc/nr_kernels_stereo.h through
`RenderEngine.plane_sweep` evaluates the same operations, in the same order, in fp32 on the device.

Classical fronto-parallel plane sweep with ZNCC.  Cameras are world-to-camera [R|t], pixel centres at integer coordinates (geometry.py).
  gray        a = ((0.299 R + 0.587 G) + 0.114 B) - 0.5: centred on mid-gray, |a| <= 0.5, so that a window's sum of squares is <= (2r+1)^2 / 4
              and the cancellation in  S_aa / N - (S_a / N)^2  costs fp32 about N / 4 ulp(1) ~ 4e-7 of variance (var_min is 1e-5)
  constants   per (view i, slot s), j = nn_ids[i][s] (-1 or i itself: an unused slot): M = K_j R_rel K_i^-1, b = K_j t_rel with R_rel = R_j R_i^T,
              t_rel = t_j - R_rel t_i, computed in float64 and ROUNDED TO FLOAT32 (sweep_constants): reference and kernel start from these
  planes      D per view, uniform in inverse depth: t = k / (D - 1), 1 / d_k = (1 - t) (1 / near_i) + t (1 / far_i)
  warp        pixel (x, y) of view i on plane k: q = d_k (((M.0 x + M.1 y) + M.2)) + b, u = q0 / q2, v = q1 / q2; valid where q2 > 0,
              0 <= u <= w - 1, 0 <= v <= h - 1; x0 = min(floor(u), w - 2), ax = u - x0 (rows likewise);
              value = top + ay (bot - top), top = g00 + ax (g01 - g00), bot = g10 + ax (g11 - g10)
  window      (2r+1)^2 = N pixels, all inside the reference image and with valid warps (a pixel within r of the border has no estimate);
              sums as separable sums, each added left to right, then top to bottom: S_r, S_rr (reference), S_s, S_ss, S_rs
  cost        m_r = S_r / N, v_r = S_rr / N - m_r^2 (source likewise), cov = S_rs / N - m_r m_s (1 / N as a factor);
              c = clip(1 - cov / sqrt(v_r v_s), 0, 2); invalid unless v_r >= var_min and v_s >= var_min
  aggregate   m valid sources: invalid if m < min_src (2; 1 for a view with one source), else the mean of the ceil(m / 2) smallest costs,
              added in ascending order
  winner      the lowest cost, ties to the lowest k; with both neighbours valid and curv = (c[k-1] - c[k]) + (c[k+1] - c[k]) > CURV_MIN:
              off = clip(0.5 (c[k-1] - c[k+1]) / curv, -0.5, 0.5); the depth is the plane formula at t = (k + off) / (D - 1)
Outputs: depth [n,h,w] float32 (0 = none), cost [n,h,w] float32 (COST_NONE where none), plane [n,h,w] int32 (-1 = none)."""
import os

import numpy as np
import torch

from . import geometry

MAX_SRC = geometry.MAX_SRC
MIN_PLANES, MAX_PLANES = 3, 256
RADII = (1, 2, 3)
COST_NONE = 4.0            # the cost where there is no estimate: above every real cost (<= 2) and every sensible max_cost
CURV_MIN = 1e-2            # the floor of the parabola's second difference: ten times the fp32 noise of a cost at low variance (~1e-3)
VAR_MIN = 1e-5
EDGE_BAND = 2e-4           # (tests) a warp coordinate this close to the image edge decides validity by rounding
DEFAULTS = {'src': 4, 'planes': 128, 'radius': 2, 'max_cost': 0.5}


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def _check_sizes(n, h, w, planes, radius, S):
    if not MIN_PLANES <= planes <= MAX_PLANES:
        raise ValueError("neuray_amd.stereo: %d planes (%d .. %d)" % (planes, MIN_PLANES, MAX_PLANES))
    if radius not in RADII:
        raise ValueError("neuray_amd.stereo: radius %r (one of %s)" % (radius, RADII))
    if not 1 <= S <= MAX_SRC:
        raise ValueError("neuray_amd.stereo: %d source slots (1 .. %d)" % (S, MAX_SRC))
    if n < 1 or h < 2 * radius + 1 or w < 2 * radius + 1:
        raise ValueError("neuray_amd.stereo: %d views of %d x %d (at least one window of radius %d)" % (n, h, w, radius))


def _check_cameras(n, poses, Ks, depth_range, nn_ids):
    """the cameras, ranges and source table of n views -> shapes checked (ValueError), float32 / int64 numpy"""
    poses, Ks, depth_range = np.asarray(poses, np.float32), np.asarray(Ks, np.float32), np.asarray(depth_range, np.float32)
    nn_ids = np.asarray(nn_ids)
    if poses.shape != (n, 3, 4) or Ks.shape != (n, 3, 3) or depth_range.shape != (n, 2) or nn_ids.ndim != 2 or nn_ids.shape[0] != n:
        raise ValueError("neuray_amd.stereo: %d images with poses %s, Ks %s, depth_range %s, nn_ids %s" %
                         (n, poses.shape, Ks.shape, depth_range.shape, nn_ids.shape))
    if not np.all((depth_range[:, 0] > 0) & (depth_range[:, 1] > depth_range[:, 0])):
        raise ValueError("neuray_amd.stereo: depth_range needs 0 < near < far")
    return poses, Ks, depth_range, nn_ids.astype(np.int64)


def _check_inputs(imgs, poses, Ks, depth_range, nn_ids):
    """-> shapes checked (ValueError), arrays as float32 / int64 numpy"""
    imgs = np.asarray(imgs, np.float32)
    if imgs.ndim != 4 or imgs.shape[1] != 3:
        raise ValueError("neuray_amd.stereo: imgs [n,3,h,w], got %s" % (imgs.shape,))
    return (imgs,) + _check_cameras(imgs.shape[0], poses, Ks, depth_range, nn_ids)


def _used(j, i, n):
    return 0 <= j < n and j != i


def sweep_constants(poses, Ks, nn_ids):
    """M (row-major, 9) and b (3) of every (view, slot), float64 arithmetic rounded to float32 -> [n,S,12]; zeros for an unused slot"""
    P, K = np.asarray(poses, np.float32).astype(np.float64), np.asarray(Ks, np.float32).astype(np.float64)
    n = P.shape[0]
    nn_ids = np.asarray(nn_ids).reshape(n, -1)
    out = np.zeros((n, nn_ids.shape[1], 12), np.float32)
    for i in range(n):
        Ki_inv = np.linalg.inv(K[i])
        for s, j in enumerate(nn_ids[i]):
            j = int(j)
            if not _used(j, i, n):
                continue
            R_rel = P[j, :, :3] @ P[i, :, :3].T
            t_rel = P[j, :, 3] - R_rel @ P[i, :, 3]
            out[i, s, :9] = (K[j] @ R_rel @ Ki_inv).reshape(9)
            out[i, s, 9:] = K[j] @ t_rel
    return out


def gray_numpy(imgs, T):
    x = np.asarray(imgs, np.float32).astype(T)
    return ((T(0.299) * x[:, 0] + T(0.587) * x[:, 1]) + T(0.114) * x[:, 2]) - T(0.5)


def _plane_depth(t, inv_near, inv_far, T):
    return T(1) / ((T(1) - t) * inv_near + t * inv_far)


def plane_depths(depth_range, planes, dtype=np.float64):
    """the plane table [n,D]"""
    T = np.dtype(dtype).type
    rng = np.asarray(depth_range, np.float32).astype(T)
    t = np.arange(planes).astype(T) / T(planes - 1)
    return _plane_depth(t[None], (T(1) / rng[:, 0])[:, None], (T(1) / rng[:, 1])[:, None], T)


def _box(a, r):
    """window sums of a [h,w]: left to right, then top to bottom; NaN where the window leaves the image (or holds a NaN)"""
    h, w = a.shape
    p = np.full((h + 2 * r, w + 2 * r), np.nan, a.dtype)
    p[r:r + h, r:r + w] = a
    rows = p[:, 0:w]
    for d in range(1, 2 * r + 1):
        rows = rows + p[:, d:d + w]
    out = rows[0:h]
    for d in range(1, 2 * r + 1):
        out = out + rows[d:d + h]
    return out


def plane_sweep_numpy(imgs, poses, Ks, depth_range, nn_ids, planes=128, radius=2, var_min=VAR_MIN, min_src=None, dtype=np.float64,
                      details=False, views=None):
    """The definition (module docstring) -> dict(depth [n,h,w] float32, cost [n,h,w] float32, plane [n,h,w] int32) and, with details:
    'volume' [n,D,h,w] (the aggregated cost, NaN where invalid), 'src_cost' [n,D,S,h,w] (NaN where invalid), 'src_var' [n,D,S,h,w],
    'ref_var' [n,h,w], 'near_edge' [n,D,S,h,w] bool (some warp of the window within EDGE_BAND of an image edge or of z = 0), 'curv' and
    'offset' [n,h,w] (the parabola's second difference and offset, NaN / 0 where it does not apply).  views: (v0, v1), sweep only those
    (the outputs then hold v1 - v0 views); the sources are looked up among all n."""
    imgs, poses, Ks, depth_range, nn_ids = _check_inputs(imgs, poses, Ks, depth_range, nn_ids)
    T = np.dtype(dtype).type
    n, _, h, w = imgs.shape
    S, D, r = nn_ids.shape[1], int(planes), radius
    _check_sizes(n, h, w, D, r, S)
    v0, v1 = (0, n) if views is None else (int(views[0]), int(views[1]))
    if not 0 <= v0 < v1 <= n:
        raise ValueError("neuray_amd.stereo: views [%d, %d) of %d" % (v0, v1, n))
    nv = v1 - v0
    gray = gray_numpy(imgs, T)
    cams = sweep_constants(poses, Ks, nn_ids).astype(T)
    rng = depth_range.astype(T)
    var_minT, inv_n = T(np.float32(var_min)), T(1) / T((2 * r + 1) ** 2)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    fx, fy = xs.astype(T), ys.astype(T)
    wm1, hm1 = T(w - 1), T(h - 1)
    out = {'depth': np.zeros((nv, h, w), np.float32), 'cost': np.full((nv, h, w), COST_NONE, np.float32), 'plane': np.full((nv, h, w), -1, np.int32)}
    if details:
        out.update(volume=np.full((nv, D, h, w), np.nan), src_cost=np.full((nv, D, S, h, w), np.nan), src_var=np.full((nv, D, S, h, w), np.nan),
                   ref_var=np.zeros((nv, h, w)), near_edge=np.zeros((nv, D, S, h, w), bool), curv=np.full((nv, h, w), np.nan),
                   offset=np.zeros((nv, h, w)))
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i in range(v0, v1):
            o = i - v0
            used = [s for s in range(S) if _used(int(nn_ids[i, s]), i, n)]
            need = int(min_src) if min_src else (1 if len(used) == 1 else 2)
            A = gray[i]
            m_r = _box(A, r) * inv_n
            v_r = _box(A * A, r) * inv_n - m_r * m_r
            inv_near, inv_far = T(1) / rng[i, 0], T(1) / rng[i, 1]
            best, best_k = np.full((h, w), np.inf, T), np.full((h, w), -1, np.int64)
            c_prev, c_next, c_last = (np.full((h, w), np.nan, T) for _ in range(3))
            for k in range(D):
                d = _plane_depth(T(k) / T(D - 1), inv_near, inv_far, T)
                costs = []
                for s in used:
                    j = int(nn_ids[i, s])
                    M = cams[i, s]
                    q0 = d * ((M[0] * fx + M[1] * fy) + M[2]) + M[9]
                    q1 = d * ((M[3] * fx + M[4] * fy) + M[5]) + M[10]
                    q2 = d * ((M[6] * fx + M[7] * fy) + M[8]) + M[11]
                    u, v = q0 / q2, q1 / q2
                    ok = (q2 > 0) & (u >= 0) & (u <= wm1) & (v >= 0) & (v <= hm1)
                    us, vs = np.where(ok, u, T(0)), np.where(ok, v, T(0))
                    x0, y0 = np.minimum(np.floor(us), T(w - 2)), np.minimum(np.floor(vs), T(h - 2))
                    ax, ay = us - x0, vs - y0
                    t = y0.astype(np.int64) * w + x0.astype(np.int64)
                    g = gray[j].reshape(-1)
                    g00, g01, g10, g11 = g[t], g[t + 1], g[t + w], g[t + w + 1]
                    top, bot = g00 + ax * (g01 - g00), g10 + ax * (g11 - g10)
                    B = np.where(ok, top + ay * (bot - top), T(np.nan))
                    m_s = _box(B, r) * inv_n
                    v_s = _box(B * B, r) * inv_n - m_s * m_s
                    cov = _box(A * B, r) * inv_n - m_r * m_s
                    c = np.minimum(np.maximum(T(1) - cov / np.sqrt(v_r * v_s), T(0)), T(2))
                    c = np.where((v_r >= var_minT) & (v_s >= var_minT), c, T(np.inf))           # (a NaN variance compares false)
                    costs.append(c)
                    if details:
                        out['src_cost'][o, k, s] = np.where(np.isfinite(c), c, np.nan)
                        out['src_var'][o, k, s] = v_s
                        band = T(EDGE_BAND)
                        near = (np.abs(u) < band) | (np.abs(u - wm1) < band) | (np.abs(v) < band) | (np.abs(v - hm1) < band) | (np.abs(q2) < T(1e-4))
                        out['near_edge'][o, k, s] = np.nan_to_num(_box(near.astype(np.float64), r), nan=0.0) > 0
                if costs:
                    srt = np.sort(np.stack(costs), 0)
                    m = np.isfinite(srt).sum(0)
                    kk = (m + 1) // 2
                    acc = srt[0]
                    for q in range(1, srt.shape[0]):
                        acc = np.where(q < kk, acc + srt[q], acc)
                    agg = np.where((m >= need) & (m > 0), acc / np.maximum(kk, 1).astype(T), T(np.nan))
                else:
                    agg = np.full((h, w), np.nan, T)
                if details:
                    out['volume'][o, k] = agg
                c_next = np.where((best_k == k - 1) & (best_k >= 0), agg, c_next)
                better = agg < best
                best, best_k = np.where(better, agg, best), np.where(better, k, best_k)
                c_prev, c_next = np.where(better, c_last, c_prev), np.where(better, T(np.nan), c_next)
                c_last = agg
            have = best_k >= 0
            curv = (c_prev - best) + (c_next - best)
            fit = have & (curv > T(CURV_MIN))
            off = np.where(fit, np.minimum(np.maximum(T(0.5) * (c_prev - c_next) / curv, T(-0.5)), T(0.5)), T(0))
            depth = _plane_depth((best_k.astype(T) + off) / T(D - 1), inv_near, inv_far, T)
            out['depth'][o] = np.where(have, depth, T(0))
            out['cost'][o] = np.where(have, best, T(COST_NONE))
            out['plane'][o] = best_k
            if details:
                out['ref_var'][o], out['curv'][o], out['offset'][o] = v_r, np.where(have, curv, np.nan), off
    return out


# ---- the public surface --------------------------------------------------------------------------------------------------------------
def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def estimate_depth(imgs, poses, Ks, depth_range, nn_ids=None, src=4, planes=128, radius=2, max_cost=0.5, geometric=True, engine=None):
    """Posed images [n,3,h,w] in [0,1] -> dict of tensors: 'photometric_depth' [n,h,w] (the sweep's depth where cost <= max_cost, else 0),
    'cost', 'plane', and 'depth': with geometric=True photometric_depth after geometry.filter_depth over the same source table (then also
    'count'), else photometric_depth itself.  nn_ids=None: the `src` nearest other cameras.  On the device when there is one (or `engine`
    is given), through plane_sweep_numpy(float32) otherwise.  The sweep does not synchronise with the host."""
    nn_ids = geometry.nearest_sources(_host(poses), src) if nn_ids is None else nn_ids
    eng = geometry._engine(engine)
    if eng is not None:
        res = eng.plane_sweep(imgs, poses, Ks, depth_range, nn_ids, planes=planes, radius=radius)
    else:
        ref = plane_sweep_numpy(_host(imgs), _host(poses), _host(Ks), _host(depth_range), _host(nn_ids), planes, radius, dtype=np.float32)
        res = {k: torch.from_numpy(v) for k, v in ref.items()}
    photo = torch.where(res['cost'] > max_cost, torch.zeros_like(res['depth']), res['depth'])
    out = {'depth': photo, 'photometric_depth': photo, 'cost': res['cost'], 'plane': res['plane']}
    if geometric:
        flt = geometry.filter_depth(photo, poses, Ks, nn_ids, engine=eng)
        out['depth'], out['count'] = flt['depth'], flt['count']
    return out


def stereo_depth_maps(database, ids, **kw):
    """Every view of `ids` with the depth estimate_depth(**kw) gives it from the other views of `ids` -> geometry.database_depth_maps'
    dictionary (float32 numpy arrays) with the estimated depth; the database's own depth maps are not read."""
    from .pipeline import build_imgs_info
    ids = list(ids)
    info = build_imgs_info(database, ids, has_depth=False)
    imgs = np.ascontiguousarray(info['imgs'], dtype=np.float32)
    est = estimate_depth(imgs, info['poses'], info['Ks'], info['depth_range'], **kw)
    return {'depth': np.ascontiguousarray(est['depth'].cpu().numpy(), dtype=np.float32), 'imgs': imgs, 'poses': info['poses'], 'Ks': info['Ks']}


class WithStereoDepth:
    """A database whose get_depth returns estimated maps: `depths` is {img_id: [h,w]} or stereo_depth_maps' dictionary together with `ids`.
    Everything else is the wrapped database's, so build_imgs_info(..., has_depth=True) and what is built on it work without depth files."""

    def __init__(self, database, depths, ids=None):
        self._database = database
        if ids is not None:
            depths = {str(i): np.asarray(depths['depth'][k], np.float32) for k, i in enumerate(ids)}
        self._depths = {str(k): np.asarray(v, np.float32) for k, v in depths.items()}

    def __getattr__(self, name):
        return getattr(self._database, name)

    def get_depth(self, img_id):
        if str(img_id) not in self._depths:
            raise KeyError("neuray_amd.stereo: no estimated depth for view %r" % (img_id,))
        return self._depths[str(img_id)]

    def get_img_ids(self, check_depth_exist=False):
        ids = self._database.get_img_ids()
        return [i for i in ids if str(i) in self._depths] if check_depth_exist else ids


def depth_path(database, img_id, root=None):
    """where `database`.get_depth looks for the depth map of a view (root: in place of the database's own directory; a database that keeps
    no files, as the procedural one, has no place of its own)"""
    if root is None:
        root = getattr(database, 'root_dir', None)
        if root is None:
            raise ValueError("neuray_amd.stereo: %s keeps no depth files: name a directory" % type(database).__name__)
    if hasattr(database, '_depth_fn') and root == getattr(database, 'root_dir', None):
        return database._depth_fn(img_id)
    ext = 'png' if type(database).__name__ == 'NeRFSyntheticDatabase' else 'jpg'
    return os.path.join(root, 'colmap_depth', '%s.%s.geometric.bin' % (img_id, ext))
