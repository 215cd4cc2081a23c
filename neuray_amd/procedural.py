"""Procedural 3-D scenes: ground truth to train and evaluate on.

Every other scene this package can make is noise on correctly posed cameras (synthetic.make_scene, synthetic.MemoryDatabase): no two
views show the same surface.  Here a scene is real geometry - up to 32 spheres and axis-aligned boxes that occlude one another, a
procedural texture in object space, a diffuse + specular shading - small enough to be a flat float32 array built from a seed, and a ray
caster renders it from any camera with exact z-depth, mask and primitive index: `render_numpy` (the formulas, vectorised, in float64 or
float32: the reference of the tests and the renderer of a machine without a GPU) and csrc/nr_kernels_proc.h through
`RenderEngine.procedural_render` (the same operations in fp32 on the device).

Scene array (include/neuray_hip.h, neuray_procedural_render): HEADER floats [n_prims, L (3), ambient, background (3), 0 ...], then PRIM
floats per primitive [kind, p (3), e (3), b (3), s, m, 4 x (k (3), phi, a (3)), 0 ...].

A ray of pixel (x, y) with sub-sample offset (ox, oy): origin c = -R^T t, direction d = R^T K^-1 [x + ox, y + oy, 1]^T, un-normalised
(oracle.coords2rays): the ray parameter is the z-depth that depth2points expects.
  sphere   the smaller root of |c + t d - p|^2 = r^2, a hit where it is > 0 (an origin inside a sphere is a miss, as for a box)
  box      slab method: the entry t_in > 0 with t_in <= t_out; an origin inside is a miss; an axis with d == 0 is its own branch (inside the
           slab: unbounded, outside: a miss); the axis of t_in is the first one that attains the maximum
  nearest hit wins, the lower primitive index on a tie
  normal   sphere (x - p) / r; box: the axis of t_in, signed against d
  albedo   clamp(b + sum_w a_w sin(2 pi k_w . (x - p) + phi_w), 0, 1)
  rgb      clamp(albedo (alpha + (1 - alpha) max(0, n . L)) + s max(0, n . h)^m, 0, 1), v = -d / |d|, h = (L + v) / |L + v|
  a miss   the background colour, mask 0, depth 0, primitive -1;  no shadows
ss sub-rays per axis at offsets (i + 1/2) / ss - 1/2: the colour is their mean, depth / mask / primitive are the centre ray's."""
import numpy as np
import torch

from . import synthetic
from . import database as _database
from .database import BaseDatabase, color_map_backward

HEADER, PRIM, MAX_PRIMS, WAVES = 16, 48, 32, 4
SPHERE, BOX = 0, 1
SCENE_RADIUS = 1.9                 # everything lies inside this ball around the origin ...
CAMERA_RADIUS = 4.03               # ... the cameras on this sphere, looking at the origin: z-depths in [2.13, 5.93]
DEPTH_RANGE = (2.0, 6.0)
FOV_X = 0.6911112070083618


# ---- the scene array ---------------------------------------------------------------------------------------------------------------
def pack_scene(prims, light=(0.0, 0.0, 1.0), ambient=0.35, background='white'):
    """prims: list of dict(kind, p, e, b, s, m, waves=[(k, phi, a) x <= 4]) -> the flat float32 scene array"""
    if background not in ('white', 'black'):
        raise NotImplementedError(background)
    if len(prims) > MAX_PRIMS:
        raise ValueError("neuray_amd.procedural: %d primitives (at most %d)" % (len(prims), MAX_PRIMS))
    out = np.zeros(HEADER + PRIM * len(prims), np.float64)
    L = np.asarray(light, np.float64)
    out[0], out[1:4], out[4] = len(prims), L / np.linalg.norm(L), ambient
    out[5:8] = 1.0 if background == 'white' else 0.0
    for i, pr in enumerate(prims):
        P = out[HEADER + PRIM * i: HEADER + PRIM * (i + 1)]
        P[0] = {'sphere': SPHERE, 'box': BOX}[pr['kind']]
        P[1:4] = pr['p']
        P[4:7] = pr['e'] if pr['kind'] == 'box' else (pr['e'], 0.0, 0.0) if np.isscalar(pr['e']) else pr['e']
        P[7:10] = pr['b']
        P[10], P[11] = pr.get('s', 0.0), pr.get('m', 1.0)
        for w, (k, phi, a) in enumerate(pr.get('waves', ())[:WAVES]):
            P[12 + 7 * w: 15 + 7 * w], P[15 + 7 * w], P[16 + 7 * w: 19 + 7 * w] = k, phi, a
    return out.astype(np.float32)


def scene_prims(scene):
    return int((np.asarray(scene).size - HEADER) // PRIM)


def _extent(pr):
    return float(pr['e']) if pr['kind'] == 'sphere' else float(np.linalg.norm(pr['e']))


def random_prim(rng, kind, p=None, e=None):
    if p is None:
        p = np.array([rng.uniform(-0.85, 0.85), rng.uniform(-0.85, 0.85), rng.uniform(-0.6, 0.55)])
    if e is None:
        e = rng.uniform(0.22, 0.5) if kind == 'sphere' else rng.uniform(0.15, 0.42, size=3)
    waves = [(rng.uniform(-1.6, 1.6, size=3), rng.uniform(0.0, 2.0 * np.pi), rng.uniform(-0.16, 0.16, size=3)) for _ in range(WAVES)]
    return {'kind': kind, 'p': p, 'e': e, 'b': rng.uniform(0.25, 0.85, size=3), 's': rng.uniform(0.05, 0.4), 'm': rng.uniform(8.0, 40.0),
            'waves': waves}


def make_scene(seed, background='white', n_prims=None):
    """The default generator: a thin box as ground plate and 5 .. 11 further spheres and boxes (both kinds) clustered above it, so that
    they occlude one another from every side; everything inside the ball of SCENE_RADIUS.  The same seed gives the same bytes."""
    rng = np.random.RandomState(seed)
    n = int(rng.randint(6, 13)) if n_prims is None else int(n_prims)
    prims = [random_prim(rng, 'box', p=np.array([0.0, 0.0, -0.9]), e=np.array([1.1, 1.1, 0.04]))]
    kinds = ['sphere', 'box'] + [('sphere', 'box')[int(rng.randint(0, 2))] for _ in range(max(n - 3, 0))]
    for kind in kinds[:max(n - 1, 0)]:
        while True:
            pr = random_prim(rng, kind)
            if np.linalg.norm(pr['p']) + _extent(pr) <= SCENE_RADIUS - 0.05 and pr['p'][2] - (pr['e'] if kind == 'sphere' else pr['e'][2]) >= -0.95:
                break
        prims.append(pr)
    light = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 1.0])
    return pack_scene(prims, light, rng.uniform(0.25, 0.45), background)


def intrinsics(h, w, fov_x=FOV_X):
    f = 0.5 * w / np.tan(0.5 * fov_x)
    return np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], np.float32)


def ring_cameras(rng, n, elev=(15.0, 55.0)):
    """n cameras around the scene on the sphere of CAMERA_RADIUS, seeded jitter in azimuth and elevation -> poses [n,3,4]"""
    return np.stack([synthetic.look_at_pose(synthetic.sphere_pos(CAMERA_RADIUS, 360.0 * i / n + 5.0 * rng.rand(), rng.uniform(*elev)))
                     for i in range(n)]).astype(np.float32)


# ---- the reference renderer ----------------------------------------------------------------------------------------------------------
def _rays(poses, Ks_inv, coords, T):
    """poses [n,3,4], Ks_inv [n,3,3], coords [n,m,2] (already with the sub-sample offset) -> origins [n,1,3], dirs [n,m,3] in dtype T"""
    R, t = poses[:, :, :3].astype(T), poses[:, :, 3].astype(T)
    Ki = Ks_inv.astype(T)
    px, py = coords[..., 0].astype(T), coords[..., 1].astype(T)
    cam = [Ki[:, i, 0, None] * px + Ki[:, i, 1, None] * py + Ki[:, i, 2, None] for i in range(3)]
    d = np.stack([R[:, 0, i, None] * cam[0] + R[:, 1, i, None] * cam[1] + R[:, 2, i, None] * cam[2] for i in range(3)], -1)
    c = np.stack([-(R[:, 0, i] * t[:, 0] + R[:, 1, i] * t[:, 1] + R[:, 2, i] * t[:, 2]) for i in range(3)], -1)
    return c[:, None, :], d


def _cast(scene, o, d, T, rel=None):
    """o, d [..., 3] in dtype T -> (t [...] (inf on a miss), prim [...] int (-1), axis [...] int) and, with rel, the near-degenerate flag of
    every ray: some sphere with |discriminant| < rel B^2, some box with |t_out - t_in| < rel t_in or its entry shared by two axes within
    rel, or the two nearest hits within rel of one another."""
    scene = np.asarray(scene, np.float32)
    shape = d.shape[:-1]
    o = np.broadcast_to(o, d.shape)
    best, second = np.full(shape, np.inf, T), np.full(shape, np.inf, T)
    bi, bax = np.full(shape, -1, np.int64), np.zeros(shape, np.int64)
    flag = np.zeros(shape, bool)
    A = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i in range(scene_prims(scene)):
            P = scene[HEADER + PRIM * i: HEADER + PRIM * (i + 1)].astype(T)
            oc = [o[..., a] - P[1 + a] for a in range(3)]
            ax = np.zeros(shape, np.int64)
            if P[0] == SPHERE:
                B = oc[0] * d[..., 0] + oc[1] * d[..., 1] + oc[2] * d[..., 2]
                Cc = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - P[4] * P[4]
                disc = B * B - A * Cc
                t = (-B - np.sqrt(np.maximum(disc, T(0)))) / A
                hit = (disc >= 0) & (t > 0)
                if rel is not None:
                    flag |= np.abs(disc) < rel * B * B
            else:
                t_in, t_out = np.full(shape, -np.inf, T), np.full(shape, np.inf, T)
                runner = np.full(shape, -np.inf, T)                  # the second-largest per-axis entry
                ok = np.ones(shape, bool)
                for a in range(3):
                    da, e = d[..., a], P[4 + a]
                    zero = da == 0
                    ok &= ~(zero & (np.abs(oc[a]) > e))
                    safe = np.where(zero, T(1), da)
                    t1, t2 = (-e - oc[a]) / safe, (e - oc[a]) / safe
                    lo = np.where(zero, T(-np.inf), np.minimum(t1, t2))
                    hi = np.where(zero, T(np.inf), np.maximum(t1, t2))
                    gt = lo > t_in
                    runner = np.where(gt, t_in, np.maximum(runner, lo))
                    ax = np.where(gt, a, ax)
                    t_in = np.where(gt, lo, t_in)
                    t_out = np.minimum(t_out, hi)
                t = t_in
                hit = ok & (t_in > 0) & (t_in <= t_out)
                if rel is not None:
                    pos = ok & (t_in > 0)
                    flag |= pos & (np.abs(t_out - t_in) < rel * t_in)
                    flag |= hit & (np.abs(t_in - runner) < rel * t_in)
            t = np.where(hit, t, T(np.inf))
            closer = t < best
            second = np.where(closer, best, np.minimum(second, t))
            bi, bax = np.where(closer, i, bi), np.where(closer, ax, bax)
            best = np.where(closer, t, best)
        if rel is not None:
            flag |= np.isfinite(second) & (np.abs(second - best) < rel * best)
    return (best, bi, bax) if rel is None else (best, bi, bax, flag)


def _shade(scene, o, d, t, prim, axis, T, albedo_only=False):
    """-> rgb [..., 3]: the colour of every ray (the background on a miss)"""
    scene = np.asarray(scene, np.float32)
    o = np.broadcast_to(o, d.shape)
    H = scene[:HEADER].astype(T)
    L, amb = H[1:4], H[4]
    rgb = np.empty(d.shape, T)
    rgb[...] = H[5:8]
    dn = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    for i in range(scene_prims(scene)):
        sel = prim == i
        if not sel.any():
            continue
        P = scene[HEADER + PRIM * i: HEADER + PRIM * (i + 1)].astype(T)
        oo, dd, tt, ddn = o[sel], d[sel], t[sel], dn[sel]
        q = [(oo[:, a] + tt * dd[:, a]) - P[1 + a] for a in range(3)]
        if P[0] == SPHERE:
            nrm = [q[a] / P[4] for a in range(3)]
        else:
            ax = axis[sel]
            da = np.where(ax == 0, dd[:, 0], np.where(ax == 1, dd[:, 1], dd[:, 2]))
            s = np.where(da > 0, T(-1), T(1))
            nrm = [np.where(ax == a, s, T(0)) for a in range(3)]
        alb = [np.full(tt.shape, P[7 + c], T) for c in range(3)]
        for w in range(WAVES):
            W = P[12 + 7 * w: 19 + 7 * w]
            ph = T(6.28318530717958647692) * (W[0] * q[0] + W[1] * q[1] + W[2] * q[2]) + W[3]
            sn = np.sin(ph)
            alb = [alb[c] + W[4 + c] * sn for c in range(3)]
        alb = [np.minimum(np.maximum(a_, T(0)), T(1)) for a_ in alb]
        if albedo_only:
            rgb[sel] = np.stack(alb, -1)
            continue
        hv = [L[a] + (-dd[:, a]) / ddn for a in range(3)]
        hn = np.sqrt(hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2])
        ndl = np.maximum(T(0), nrm[0] * L[0] + nrm[1] * L[1] + nrm[2] * L[2])
        with np.errstate(divide='ignore', invalid='ignore'):
            ndh = np.where(hn > 0, np.maximum(T(0), (nrm[0] * hv[0] + nrm[1] * hv[1] + nrm[2] * hv[2]) / hn), T(0))
        shade = amb + (T(1) - amb) * ndl
        spec = P[10] * np.power(ndh, P[11])
        rgb[sel] = np.stack([np.minimum(np.maximum(a_ * shade + spec, T(0)), T(1)) for a_ in alb], -1)
    return rgb


def _inverse(Ks, T):
    if T == np.float64:
        return np.linalg.inv(np.asarray(Ks, np.float64))
    from .engine import host_inverse
    return host_inverse(torch.from_numpy(np.ascontiguousarray(Ks, np.float32))).numpy()


def _offsets(ss, T):
    """the sub-ray offsets in the kernel's order (y outer, x inner), evaluated in dtype T as the kernel evaluates them in fp32"""
    o = [(T(i) + T(0.5)) / T(ss) - T(0.5) for i in range(ss)]
    return [(o[i], o[j]) for j in range(ss) for i in range(ss)]


def render_numpy(scene, poses, Ks, h, w, ss=1, dtype=np.float64, albedo_only=False, degenerate_rel=None):
    """The reference renderer -> dict(rgb [n,3,h,w] dtype, depth [n,h,w] dtype, mask [n,h,w] uint8, prim [n,h,w] int8) and, with
    degenerate_rel, 'degenerate' [n,h,w] bool: some sub-ray or the centre ray of the pixel is near-degenerate (see _cast)."""
    if ss not in (1, 2, 3, 4):
        raise ValueError("neuray_amd.procedural: ss=%r (1 .. 4)" % (ss,))
    T = np.dtype(dtype).type
    poses = np.asarray(poses, np.float32).reshape(-1, 3, 4)
    n = poses.shape[0]
    Ki = _inverse(np.asarray(Ks, np.float32).reshape(-1, 3, 3), T)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    grid = np.broadcast_to(np.stack([xs, ys], -1).reshape(1, h * w, 2).astype(T), (n, h * w, 2))
    acc = np.zeros((n, h * w, 3), T)
    flag = np.zeros((n, h * w), bool)
    centre = None

    def cast(ox, oy):
        o, d = _rays(poses, Ki, grid + np.array([ox, oy], T), T)
        res = _cast(scene, o, d, T, degenerate_rel)
        if degenerate_rel is not None:
            np.logical_or(flag, res[3], out=flag)
        return o, d, res
    for ox, oy in _offsets(ss, T):
        o, d, res = cast(ox, oy)
        acc = acc + _shade(scene, o, d, res[0], res[1], res[2], T, albedo_only)
        if ox == 0 and oy == 0:                  # odd ss: the middle sub-ray is the centre ray
            centre = res
    if centre is None:                           # even ss: the centre ray is a ray of its own and carries no colour
        centre = cast(T(0), T(0))[2]
    t, prim = centre[0], centre[1]
    hit = prim >= 0
    out = {'rgb': (acc / T(ss * ss)).reshape(n, h, w, 3).transpose(0, 3, 1, 2).copy(),
           'depth': np.where(hit, t, T(0)).reshape(n, h, w), 'mask': hit.astype(np.uint8).reshape(n, h, w),
           'prim': prim.astype(np.int8).reshape(n, h, w)}
    if degenerate_rel is not None:
        out['degenerate'] = flag.reshape(n, h, w)
    return out


def cast_numpy(scene, origins, dirs, dtype=np.float64):
    """Nearest hit of arbitrary rays origins + t dirs ([..., 3]) -> (t [...] (inf on a miss), prim [...] int64 (-1 on a miss))"""
    T = np.dtype(dtype).type
    t, prim, _ = _cast(scene, np.asarray(origins).astype(T), np.asarray(dirs).astype(T), T)
    return t, prim


def albedo_numpy(scene, points, prim, dtype=np.float64):
    """The object-space albedo of primitive prim [...] at world points [..., 3] (what rgb is with s = 0 and ambient 1)"""
    T = np.dtype(dtype).type
    pts = np.asarray(points).astype(T)
    zero = np.zeros_like(pts)
    return _shade(scene, pts, zero + T(1), np.zeros(pts.shape[:-1], T), np.asarray(prim), np.zeros(pts.shape[:-1], np.int64), T, albedo_only=True)


# ---- rendering where the hardware is ---------------------------------------------------------------------------------------------------
def _device_engine(device=None):
    """a RenderEngine when a HIP device is there, else None (the database then renders through render_numpy)"""
    if device is None:
        if not torch.cuda.is_available():
            return None
        device = 'cuda:0'
    if torch.device(device).type != 'cuda':
        return None
    from .network import render_ops
    return render_ops.engine_for(device)


def _fresh_engine(device):
    from .network import render_ops
    return render_ops.engine_for(device)


class ProceduralDatabase(BaseDatabase):
    """database_name = 'procedural/<seed>/<white|black>_<size>': make_scene(seed) seen from `n_views` seeded cameras around it (48: every
    8th one is a validation / test view, the LLFF rule of get_database_split), <size> x <size> pixels unless h / w are given.  The accessor
    methods of the reference's BaseDatabase; the views are rendered once, on first use: through the kernel when a HIP device is there,
    through render_numpy otherwise."""

    def __init__(self, database_name, root=None, n_views=48, h=None, w=None, ss=2, device=None):
        super().__init__(database_name)
        _, seed, background_size = database_name.split('/')
        background, size = background_size.split('_')
        if background not in ('black', 'white'):
            raise NotImplementedError(background)
        self.seed, self.background, self.img_size = int(seed), background, int(size)
        self.h, self.w = int(h or size), int(w or size)
        self.ss, self.device = ss, device
        self.scene = make_scene(self.seed, background)
        self.img_ids = [str(i) for i in range(n_views)]
        self.poses = ring_cameras(np.random.RandomState((self.seed + 1000003) % (2 ** 32)), n_views)
        self.K = intrinsics(self.h, self.w)
        self.depth_range = np.asarray(DEPTH_RANGE, np.float32)
        self._views = {}
        self.rendered_on = None

    def _render(self, idx):
        eng = _device_engine(self.device)
        Ks = np.repeat(self.K[None], len(idx), 0)
        if eng is not None:
            out = {k: v.cpu().numpy() for k, v in eng.procedural_render(self.scene, self.poses[idx], Ks, self.h, self.w, self.ss).items()}
            self.rendered_on = 'hip'
        else:
            out = render_numpy(self.scene, self.poses[idx], Ks, self.h, self.w, self.ss)
            self.rendered_on = 'numpy'
        for j, i in enumerate(idx):
            self._views[i] = (color_map_backward(np.ascontiguousarray(out['rgb'][j].transpose(1, 2, 0)).astype(np.float32)),
                              out['mask'][j] > 0, np.ascontiguousarray(out['depth'][j], dtype=np.float32))

    def _view(self, img_id):
        i = self.img_ids.index(str(img_id))
        if i not in self._views:
            # on a device: every view in one launch; on the host: the view asked for (a numpy ray cast of a whole scene takes a while)
            on_device = _device_engine(self.device) is not None
            self._render([k for k in range(len(self.img_ids)) if k not in self._views] if on_device else [i])
        return self._views[i]

    def get_img_ids(self, check_depth_exist=False):
        return list(self.img_ids)

    def get_image(self, img_id):
        return self._view(img_id)[0]

    def get_mask(self, img_id):
        return self._view(img_id)[1]

    def get_depth(self, img_id):
        return self._view(img_id)[2]

    def get_K(self, img_id):
        return self.K.copy()

    def get_pose(self, img_id):
        return self.poses[self.img_ids.index(str(img_id))].copy()

    def get_depth_range(self, img_id):
        return self.depth_range.copy()

    def get_bbox(self, img_id):
        ys, xs = np.nonzero(self.get_mask(img_id))
        return [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]


# ---- augmentation of a training sample -----------------------------------------------------------------------------------
# What the reference's GeneralRendererDataset.__getitem__ does to a `gso` sample (objects, masks, exact depth), in its order: the depth
# ranges of all views are shrunk towards the masked depth and widened; the depth maps the init net sees are corrupted (two offset regions
# and a global noise per working view, scaled by the view's augmented range) while true_depth keeps the exact map; the ranges are made
# consistent; half of the rays are drawn from the query view's foreground.  The host draws the numbers that do not depend on device data
# (augment_host_numbers); per-pixel randomness is Philox4x32-10, key = (stream seed, batch index), counter = (y * w + x, view, purpose, 0),
# purposes 0 / 1: the local noise of the large / small region, 2: the global noise, 3: the ray selection.  augment_numpy and
# sample_coords_numpy are the formulas (the reference of the tests, the path of a machine without a GPU); csrc/nr_kernels_aug.h through
# RenderEngine.augment_stats / augment_depth / sample_coords evaluates them in fp32 on the device.
AUGMENT_DEFAULTS = {
    'aug_gso_shrink_range_prob': 0.5,
    'aug_use_depth_offset': True, 'aug_depth_offset_prob': 0.25, 'aug_depth_offset_region_min': 0.05, 'aug_depth_offset_region_max': 0.1,
    'aug_depth_offset_min': 0.5, 'aug_depth_offset_max': 1.0, 'aug_depth_offset_local': 0.1,
    'aug_use_depth_small_offset': True, 'aug_depth_small_offset_prob': 0.5,
    'aug_use_global_noise': True, 'aug_global_noise_prob': 0.5,
    'foreground_ratio': 0.5, 'use_consistent_depth_range': True,
}
AUG_HOST = 16                                        # floats of the host array's head and of every working view (include/neuray_hip.h)
_SMALL_REGION = (0.1, 0.2, 0.01, 0.05, 0.005)        # region min / max, offset min / max, local amplitude: the reference's literals
_M32 = 0xffffffff


def augment_config(augment):
    """None / False -> None (no augmentation); True -> the reference's defaults; a dict overrides keys of AUGMENT_DEFAULTS"""
    if augment is None or augment is False:
        return None
    cfg = dict(AUGMENT_DEFAULTS)
    if augment is not True:
        unknown = set(augment) - set(cfg)
        if unknown:
            raise KeyError("neuray_amd.procedural: unknown augmentation keys %s" % sorted(unknown))
        cfg.update(augment)
    return cfg


def philox4x32(counter, key, rounds=10):
    """Philox4x32-10 (Random123): counter [..., 4] and key (k0, k1) as uint32 -> [..., 4] uint32"""
    c = np.asarray(counter, np.uint64)
    c = [c[..., i] for i in range(4)]
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    m = np.uint64(_M32)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return np.stack(c, -1).astype(np.uint32)


def _pixel_words(h, w, view, purpose, key):
    """the Philox block of every pixel of a view -> [h * w, 4] uint32"""
    ctr = np.zeros((h * w, 4), np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = np.arange(h * w), view, purpose
    return philox4x32(ctr, key)


def augment_host_numbers(rng, rfn, cfg):
    """The numbers of one batch that do not depend on device data, drawn from `rng` in a fixed order -> float32 [AUG_HOST (1 + rfn)]
    (the layout: include/neuray_hip.h, neuray_augment_depth).  A uniform is randint(0, 2^24) / 2^24: exact in float32, never 1."""
    def u():
        return rng.randint(0, 2 ** 24) / 2.0 ** 24
    out = np.zeros((1 + rfn, AUG_HOST), np.float32)
    out[0, :7] = [u() < cfg['aug_gso_shrink_range_prob'], u(), u(), u() < 0.8, u(), u(), bool(cfg['use_consistent_depth_range'])]
    out[0, 8:13] = [cfg['aug_depth_offset_region_min'], cfg['aug_depth_offset_region_max'], cfg['aug_depth_offset_min'],
                    cfg['aug_depth_offset_max'], cfg['aug_depth_offset_local']]
    for r in range(rfn):
        for k, (use, prob) in enumerate((('aug_use_depth_offset', 'aug_depth_offset_prob'), ('aug_use_depth_small_offset', 'aug_depth_small_offset_prob'))):
            on = u() < cfg[prob]
            out[1 + r, 6 * k: 6 * k + 6] = [bool(cfg[use]) and on, u(), u(), u(), u(), u() < 0.5]
        on = u() < cfg['aug_global_noise_prob']
        out[1 + r, 12] = bool(cfg['aug_use_global_noise']) and on
    return out.reshape(-1)


def stats_numpy(mask, depth):
    """per view over mask > 0 -> dict(count [n], bbox [n,4] (xmin, xmax, ymin, ymax), depth_min / depth_max [n] float32 over the pixels
    with 1e-3 < d < 1e4, row_counts [n,h]); an empty mask: count 0, bbox (w, -1, h, -1); no valid depth: +inf / -inf"""
    mask, depth = np.asarray(mask), np.asarray(depth, np.float32)
    n, h, w = mask.shape
    out = {'count': np.zeros(n, np.int32), 'bbox': np.zeros((n, 4), np.int32), 'depth_min': np.full(n, np.inf, np.float32),
           'depth_max': np.full(n, -np.inf, np.float32), 'row_counts': (mask > 0).sum(2).astype(np.int32)}
    for v in range(n):
        ys, xs = np.nonzero(mask[v] > 0)
        out['count'][v] = ys.size
        out['bbox'][v] = (xs.min(), xs.max(), ys.min(), ys.max()) if ys.size else (w, -1, h, -1)
        d = depth[v][mask[v] > 0]
        d = d[(d > np.float32(1e-3)) & (d < np.float32(1e4))]
        if d.size:
            out['depth_min'][v], out['depth_max'][v] = d.min(), d.max()
    return out


def _uni(lo, hi, u, T):
    return T(lo) + (T(hi) - T(lo)) * T(u)


def augment_numpy(depth, mask, depth_range, host, key, view0, rfn, dtype=np.float32, depth_range_aug=None):
    """The reference of neuray_augment_depth (include/neuray_hip.h states the formulas): depth / mask [n,h,w], depth_range [n,2], host:
    augment_host_numbers' array, key: (seed, batch index), the working views are [view0, view0 + rfn) -> dict(stats, depth_range_aug
    [n,2], depth_range [n,2], plan [rfn,2,8], depth_aug [rfn,h,w]) in `dtype`, every operation in the kernel's order.  depth_range_aug:
    use these ranges as the result of step 1 (a test hands over the kernel's own, so that what follows can be compared bit for bit).  The
    centre's rank is evaluated in float32 in either dtype: it selects a pixel."""
    T = np.dtype(dtype).type
    mask, depth = np.asarray(mask), np.asarray(depth, np.float32)
    n, h, w = mask.shape
    H = np.asarray(host, np.float32).reshape(-1, AUG_HOST)
    st = stats_numpy(mask, depth)
    near, far = np.asarray(depth_range, np.float32)[:, 0].astype(T), np.asarray(depth_range, np.float32)[:, 1].astype(T)
    # 1. the range augmentation
    part = np.isfinite(st['depth_min'])
    if H[0, 0] != 0 and part.any():
        far_ratio = np.max((st['depth_max'][part].astype(T) * T(1.1)) / far[part])
        near_ratio = np.max(near[part] / (st['depth_min'][part].astype(T) * T(0.9)))
        if far_ratio < 1:
            far = far * _uni(far_ratio, 1.0, H[0, 1], T)
        if near_ratio < 1:
            near = near / _uni(near_ratio, 1.0, H[0, 2], T)
    if H[0, 3] != 0:
        near, far = near * (T(1) - _uni(0.025, 0.1, H[0, 4], T)), far * (T(1) + _uni(0.025, 0.1, H[0, 5], T))
    if depth_range_aug is not None:
        near, far = np.asarray(depth_range_aug)[:, 0].astype(T), np.asarray(depth_range_aug)[:, 1].astype(T)
    range_aug = np.stack([near, far], -1)
    # 2. the depth noise of the working views
    plan, depth_aug = np.zeros((rfn, 2, 8), T), np.zeros((rfn, h, w), T)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    for r in range(rfn):
        v = view0 + r
        L = far[v] - near[v]
        d, fg, count = depth[v].astype(T), mask[v] > 0, int(st['count'][v])
        xmin, xmax, ymin, ymax = (int(b) for b in st['bbox'][v])
        for k in range(2):
            R = H[1 + r, 6 * k: 6 * k + 6]
            plan[r, k, 7] = L
            if R[0] == 0 or count == 0:
                continue
            rank = min(int(np.float32(R[1]) * np.float32(count)), count - 1)
            cy, cx = divmod(int(np.flatnonzero(fg)[rank]), w)
            rmin, rmax, omin, omax, amp = (H[0, 8:13] if k == 0 else _SMALL_REGION)
            lx, ly = _uni(rmin, rmax, R[2], T) * T(xmax - xmin), _uni(rmin, rmax, R[3], T) * T(ymax - ymin)
            off = _uni(omin, omax, R[4], T) * L
            if R[5] != 0:
                off = -off
            plan[r, k] = [1, cx, cy, lx, ly, off, T(amp), L]
            region = fg & (np.abs((xs - cx).astype(T)) < lx) & (np.abs((ys - cy).astype(T)) < ly)
            unit = (_pixel_words(h, w, v, k, key)[:, 0] >> np.uint32(8)).astype(T).reshape(h, w) * T(2.0 ** -24)
            d = np.where(region, d + ((((T(2) * unit - T(1)) * T(amp)) * L) + off), d)
        if H[1 + r, 12] != 0:
            unit = (_pixel_words(h, w, v, 2, key)[:, 0] >> np.uint32(8)).astype(T).reshape(h, w) * T(2.0 ** -24)
            d = d + ((T(2) * unit - T(1)) * T(0.005)) * L
        depth_aug[r] = d
    # 3. consistent_depth_range (the use_consistent_min_max: False branch)
    if H[0, 6] != 0:
        length = far - near
        max_len = np.max(length)
        near = np.maximum(near - (max_len - length) / T(2), near * T(0.5))
        far = near + max_len
    return {'stats': st, 'depth_range_aug': range_aug, 'depth_range': np.stack([near, far], -1), 'plan': plan, 'depth_aug': depth_aug}


def sample_coords_numpy(mask, ray_num, foreground_ratio, key, view=0):
    """The reference of neuray_sample_coords: a uniform draw without replacement as the k smallest of independent random keys.  mask
    [h,w] -> coords [1,ray_num,2] float32 (x, y): the min(int(ray_num * foreground_ratio), foreground) foreground pixels with the
    smallest (word0 << 32) | p, then the rest with the smallest (word1 << 32) | p among all pixels not yet picked, each part in row-major
    order (p = y * w + x; the words: the pixel's purpose-3 Philox block)."""
    fg = np.asarray(mask) > 0
    h, w = fg.shape
    if not 1 <= ray_num <= h * w:
        raise ValueError("neuray_amd.procedural: ray_num=%d outside [1, h*w=%d]" % (ray_num, h * w))
    words = _pixel_words(h, w, view, 3, key).astype(np.uint64)
    p = np.arange(h * w, dtype=np.uint64)
    c1, c2 = (words[:, 0] << np.uint64(32)) | p, (words[:, 1] << np.uint64(32)) | p
    cand = np.flatnonzero(fg.reshape(-1))
    k1 = min(int(ray_num * foreground_ratio), cand.size)
    pick1 = np.sort(cand[np.argsort(c1[cand], kind='stable')[:k1]])
    left = np.ones(h * w, bool)
    left[pick1] = False
    pool = np.flatnonzero(left)
    pick2 = np.sort(pool[np.argsort(c2[pool], kind='stable')[:ray_num - k1]])
    pix = np.concatenate([pick1, pick2]).astype(np.int64)
    return np.stack([pix % w, pix // w], -1)[None].astype(np.float32)


# ---- a fresh scene per training step ---------------------------------------------------------------------------------------------------
# offsets (azimuth, elevation) in degrees of the source views from the query view, before the seeded jitter
_SRC_OFFS = [(-5, 5), (5, -5), (-10, -8), (10, 8), (-15, 12), (15, -12), (-20, -3), (20, 3), (-25, 15), (25, -15), (-30, 6), (30, -6),
             (0, 20), (0, -20), (12, 18), (-12, -18)]


def _upload(array, device):
    t = torch.from_numpy(np.ascontiguousarray(array))
    if torch.device(device).type == 'cuda':
        return t.pin_memory().to(device, non_blocking=True)
    return t.to(device)


class ProceduralStream:
    """An endless iterator of generalisation-training batches, the dictionary NeuralRayGenRenderer trains on (bench.gen_train_case builds
    one by hand on random images): every batch a new scene and new cameras - 1 query view, `rfn` working views and `extra_src` further
    source views for the cost volumes -, rendered on the device by one kernel launch.  The host prepares the scene array, the poses, the
    inverse intrinsics, the ray coordinates and the neighbour table and uploads them from pinned memory without blocking; nothing is read
    back.  augment: None / False - the sample as rendered (depth is true_depth, the range (2, 6), uniform rays); True or a dict of
    AUGMENT_DEFAULTS keys - the reference's training augmentation on the device: augmented and consistent depth ranges, a noisy `depth`
    beside the exact `true_depth`, half of the rays from the query view's foreground (three more entries, still nothing read back)."""

    def __init__(self, device, seed=0, h=416, w=608, rfn=8, extra_src=4, rays=512, ss=1, background='white', engine=None, augment=None):
        if rfn + extra_src > len(_SRC_OFFS):
            raise ValueError("neuray_amd.procedural: at most %d source views" % len(_SRC_OFFS))
        self.device = torch.device(device)
        self.augment = augment_config(augment)       # None: the plain stream; else the reference's augmentation
        self.last_augment = None                     # with augmentation: the host numbers and the kernels' plan / ranges of the last batch
        self.seed, self.h, self.w, self.rfn, self.extra_src, self.rays, self.ss, self.background = seed, h, w, rfn, extra_src, rays, ss, background
        self.engine = engine if engine is not None else _fresh_engine(self.device)
        self.index = 0
        self.K = intrinsics(h, w)
        from .engine import host_inverse
        self.K_inv = host_inverse(torch.from_numpy(self.K[None])).numpy()[0]

    def __iter__(self):
        return self

    def host_batch(self, index):
        """what the host prepares for batch `index`: scene array, poses [1 + n_src,3,4] (the query view first), coords, nn_ids"""
        return self._host_draws(index)[:4]

    def _host_draws(self, index):
        """host_batch and the batch's RandomState after its draws (the augmentation draws its numbers from there on)"""
        from .network.renderer import nearest_view_table
        rng = np.random.RandomState((self.seed * 1000003 + index) % (2 ** 32))
        scene = make_scene(int(rng.randint(0, 2 ** 31 - 1)), self.background)
        n_src = self.rfn + self.extra_src
        az, el = rng.uniform(0.0, 360.0), rng.uniform(22.0, 42.0)
        angles = [(az, el)] + [(az + a + rng.uniform(-2.0, 2.0), max(el + e + rng.uniform(-2.0, 2.0), 4.0)) for a, e in _SRC_OFFS[:n_src]]
        poses = np.stack([synthetic.look_at_pose(synthetic.sphere_pos(CAMERA_RADIUS, a, e)) for a, e in angles]).astype(np.float32)
        coords = np.stack([rng.randint(0, self.w, size=self.rays), rng.randint(0, self.h, size=self.rays)], -1)[None].astype(np.float32)
        nn_ids = nearest_view_table(poses[1:1 + self.rfn], poses[1:])[:, 1:4].astype(np.int64)          # (column 0: the view itself)
        return scene, poses, coords, nn_ids, rng

    def __next__(self):
        index, dev = self.index, self.device
        self.index += 1
        scene, poses, coords, nn_ids, rng = self._host_draws(index)
        n, rfn = poses.shape[0], self.rfn
        t_scene, t_poses = _upload(scene, dev), _upload(poses, dev)
        Ks = _upload(np.repeat(self.K[None], n, 0), dev)
        Ks_inv = _upload(np.repeat(self.K_inv[None], n, 0), dev)
        rng_ = _upload(np.repeat(np.asarray(DEPTH_RANGE, np.float32)[None], n, 0), dev)
        out = self.engine.procedural_render(t_scene, t_poses, Ks, self.h, self.w, self.ss, Ks_inv=Ks_inv, outputs=('depth', 'mask'),
                                            n_prims=scene_prims(scene))
        imgs, depth, masks = out['rgb'], out['depth'][:, None], out['mask'][:, None].float()
        src = {'imgs': imgs[1:], 'poses': t_poses[1:], 'Ks': Ks[1:], 'depth_range': rng_[1:]}
        ref = {k: v[:rfn] for k, v in src.items()}
        ref.update({'masks': masks[1:1 + rfn], 'depth': depth[1:1 + rfn], 'true_depth': depth[1:1 + rfn], 'nn_ids': _upload(nn_ids, dev)})
        que = {'imgs': imgs[:1], 'poses': t_poses[:1], 'Ks': Ks[:1], 'Ks_inv': Ks_inv[:1], 'depth_range': rng_[:1], 'coords': _upload(coords, dev),
               'masks': masks[:1], 'depth': depth[:1]}
        if self.augment is not None:
            # (in the reference's order: ranges over all views, noise on the working views, consistent ranges, rays from the query mask)
            key = (self.seed & _M32, index & _M32)
            host = augment_host_numbers(rng, rfn, self.augment)
            stats = self.engine.augment_stats(out['mask'], out['depth'])
            aug = self.engine.augment_depth(out['depth'], out['mask'], rng_, stats, _upload(host, dev), key, 1, rfn)
            final = aug['depth_range']
            src['depth_range'], ref['depth_range'], que['depth_range'] = final[1:], final[1:1 + rfn], final[:1]
            ref['depth'] = aug['depth_aug'][:, None]
            que['coords'] = self.engine.sample_coords(out['mask'][0], self.rays, self.augment['foreground_ratio'], key, view=0)
            self.last_augment = {'host': host, 'key': key, 'stats': stats, 'plan': aug['plan'], 'depth_range_aug': aug['depth_range_aug']}
        return {'que_imgs_info': que, 'ref_imgs_info': ref, 'src_imgs_info': src, 'scene_name': 'procedural/%d/%d' % (self.seed, index)}


_database.name2database['procedural'] = ProceduralDatabase
