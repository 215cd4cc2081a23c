"""Mesh export from the command line (neuray_amd/mesh.py):

    python -m neuray_amd.export_mesh --database NAME --depth database|render|stereo [--cfg CFG --ckpt CKPT] --voxel V --out mesh.ply
                                     [--trunc T --min-weight 1 --no-filter --src 8 --tau-px 1 --tau-d 0.01 --min-views 2 --json out.json]
                                     [--raycast DIR --step 0.5]

fuses the depth maps of every view of a database - its own (`--depth database`), plane-sweep stereo of its images (`--depth stereo`, neuray_amd.stereo), or the `render_depth_fine` of a renderer that renders each
view from its nearest other views (`--depth render`, as neuray_amd.export_points) - into a truncated signed distance field of voxel size V
(default: 256 lattice points on the longest side of the depths' bounding box) and writes its zero surface as a binary PLY with normals,
colours and triangles.  The printed line carries the vertex count, the face count and the number of boundary edges (0: the surface is closed)
and, for a procedural scene, the distance of the vertices to the true surface.  `--raycast DIR` casts the fused volume from every view's
camera (mesh.TSDFVolume.raycast) and writes DIR/<view id>.npz with depth [h,w], normal [3,h,w], colour [3,h,w] and status
[h,w]; for a procedural scene the line gains `raycast_depth`, for all views and for the held-out ones (every 8th, get_database_split's rule):
the share of the true foreground pixels with a hit, the share of the hits that lie on true background, and the median and 95th percentile of
|depth - true depth| over the pixels that have both.

    python -m neuray_amd.export_mesh --time

measures the kernels on the MI355X at 48 views of 800 x 800 of procedural scene 1 and a 256^3 volume over the scene's ball - the integration
of all 48 views (one launch) and the extraction (surface_cells + the two prefix sums + surface_emit, with its one read-back) - with device
events, the median of 20 after warm-up, next to an eager PyTorch composition of the same formulas in the same process, and reports the share of
the HBM peak that the compulsory traffic amounts to - and the ray casting of the fused volume from the same 48 cameras at 800 x 800: the
kernel with block skipping and without, the preparation (field, cell bytes, block bytes), an eager PyTorch composition of the same
fixed-step march without skipping, and the field samples per second from the `evaluated` output.  One JSON line."""
import argparse
import json
import os

import numpy as np
import torch

from . import database as _database
from . import geometry, mesh, procedural
from .export_points import HBM_PEAK, _median_ms, _renderer


def export(args):
    db = _database.parse_database_name(args.database)
    ids = db.get_img_ids()
    if args.depth == 'database':
        maps = geometry.database_depth_maps(db, ids)
    elif args.depth == 'stereo':
        from . import stereo
        maps = stereo.stereo_depth_maps(db, ids)
    else:
        if not args.cfg:
            raise SystemExit("neuray_amd.export_mesh: --depth render needs --cfg (and usually --ckpt)")
        if not torch.cuda.is_available():
            raise SystemExit("neuray_amd.export_mesh: --depth render needs the HIP device (the render path has no CPU fallback)")
        maps = geometry.render_depth_maps(_renderer(args.cfg, args.ckpt, db, ids, 'cuda:0'), db, ids)
    out = mesh.fuse_mesh(maps['depth'], maps['imgs'], maps['poses'], maps['Ks'], voxel_size=args.voxel, trunc=args.trunc, filter=not args.no_filter,
                         src=args.src, tau_px=args.tau_px, tau_d=args.tau_d, min_views=args.min_views, min_weight=args.min_weight)
    mesh.write_mesh_ply(args.out, out['vertices'], out['faces'], out['colors'], out['normals'])
    vol = out['volume']
    n, h, w = maps['depth'].shape
    res = {'database': args.database, 'depth': args.depth, 'views': n, 'h': h, 'w': w, 'vertices': int(out['vertices'].shape[0]),
           'faces': int(out['faces'].shape[0]), 'boundary_edges': mesh.boundary_edges(out['faces']), 'voxel_size': vol.voxel_size,
           'trunc': vol.trunc, 'dims': list(vol.dims), 'origin': list(vol.origin), 'out': args.out,
           'on': 'hip' if vol.engine is not None else 'numpy',
           'settings': {'filter': not args.no_filter, 'src': args.src, 'tau_px': args.tau_px, 'tau_d': args.tau_d, 'min_views': args.min_views,
                        'min_weight': args.min_weight}}
    if args.raycast:
        res['raycast'] = args.raycast
        res.update(raycast_export(args, db, ids, maps, vol))
    if isinstance(db, procedural.ProceduralDatabase) and res['vertices']:
        dist = geometry.surface_distance(db.scene, out['vertices'])
        res['surface_distance'] = {'mean': float(dist.mean()), 'median': float(np.median(dist)), 'p95': float(np.percentile(dist, 95)),
                                   'max': float(dist.max())}
    return res


def depth_scores(cast, status, true):
    """ray-cast depth against the true depth over views [m,h,w] -> the `raycast_depth` figures"""
    hit, fg = status == 1, true > 0
    both = hit & fg
    err = np.abs(cast.astype(np.float64) - true)[both]
    return {'views': int(cast.shape[0]), 'foreground_hit_share': float(both.sum() / max(fg.sum(), 1)),
            'hits_on_background_share': float((hit & ~fg).sum() / max(hit.sum(), 1)),
            'median': float(np.median(err)) if err.size else None, 'p95': float(np.percentile(err, 95)) if err.size else None}


def raycast_export(args, db, ids, maps, vol):
    """casts `vol` from the cameras of `maps`, writes the .npz files and scores the depth against the TRUE depth of a procedural database -
    the database's own maps, whatever depth was fused (`maps['depth']` is the renderer's with --depth render)"""
    n, h, w = maps['depth'].shape
    out = {k: geometry._host(v) for k, v in vol.raycast(maps['poses'], maps['Ks'], h, w, args.min_weight, args.step).items()}
    os.makedirs(args.raycast, exist_ok=True)
    for i, view_id in enumerate(ids):
        np.savez(os.path.join(args.raycast, '%s.npz' % view_id), depth=out['depth'][i], normal=out['normal'][i], colour=out['colors'][i],
                 status=out['status'][i])
    res = {'raycast_step': args.step, 'raycast_hits': int((out['status'] == 1).sum())}
    if isinstance(db, procedural.ProceduralDatabase):
        held = np.array([v in set(_database.get_database_split(db, 'val_all')[1]) for v in ids])
        true = maps['depth'] if args.depth == 'database' else geometry.database_depth_maps(db, ids)['depth']
        res['raycast_depth'] = {'all': depth_scores(out['depth'], out['status'], true)}
        if held.any():
            res['raycast_depth']['held_out'] = depth_scores(out['depth'][held], out['status'][held], true[held])
    return res


# ---- --time --------------------------------------------------------------------------------------------------------------------------
def eager_integrate(state, depth, rgb, P, K, origin, vs, dims, trunc):
    """mesh.integrate_numpy in eager PyTorch on the device, colour included (P, K: host tensors - their entries become kernel constants, as
    the kernel reads them through scalar loads); updates and returns `state`"""
    nx, ny, nz = dims
    dev = depth.device
    n, h, w = depth.shape
    iz, iy, ix = torch.meshgrid(torch.arange(nz, device=dev), torch.arange(ny, device=dev), torch.arange(nx, device=dev), indexing='ij')
    X = [origin[0] + ix.float() * vs, origin[1] + iy.float() * vs, origin[2] + iz.float() * vs]
    P, K = P.tolist(), K.tolist()
    flat = rgb.reshape(n, 3, h * w)
    ts, ws, cs, cw = state['tsum'], state['w'], state['csum'], state['cw']
    for i in range(n):
        c = [P[i][k][0] * X[0] + P[i][k][1] * X[1] + P[i][k][2] * X[2] + P[i][k][3] for k in range(3)]
        q = [K[i][k][0] * c[0] + K[i][k][1] * c[1] + K[i][k][2] * c[2] for k in range(3)]
        un, vn = torch.floor(q[0] / q[2] + 0.5), torch.floor(q[1] / q[2] + 0.5)
        inb = (c[2] > 0) & (un >= 0) & (un < w) & (vn >= 0) & (vn < h)
        t = torch.where(inb, vn, torch.zeros_like(vn)).long() * w + torch.where(inb, un, torch.zeros_like(un)).long()
        d = torch.where(inb, depth[i].reshape(-1)[t], torch.zeros_like(un))
        sdf = d - c[2]
        kept = inb & (d > 0) & ~(sdf < -trunc)
        ts = torch.where(kept, ts + torch.clamp(sdf / trunc, max=1.0), ts)
        ws = ws + kept
        col = kept & (sdf <= trunc)
        cs = cs + torch.where(col[None], flat[i][:, t.reshape(-1)].reshape(3, nz, ny, nx), torch.zeros_like(cs))
        cw = cw + col
    state.update(tsum=ts, w=ws, csum=cs, cw=cw)
    return state


def eager_cells(tsum, w, min_weight):
    """mesh.cells_numpy in eager PyTorch: the cell bytes alone - no vertices, normals, colours or faces: less work than the kernels do"""
    inside, ok = (tsum / w) < 0, w >= min_weight

    def corner(a, dx, dy, dz):
        nz, ny, nx = a.shape
        return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    def shift(a, sx, sy, sz):
        o = torch.zeros_like(a)
        mz, my, mx = a.shape
        o[sz:, sy:, sx:] = a[:mz - sz, :my - sy, :mx - sx]
        return o
    valid = torch.ones_like(corner(ok, 0, 0, 0))
    any_in, all_in = torch.zeros_like(valid), torch.ones_like(valid)
    for k in range(8):
        dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
        valid = valid & corner(ok, dx, dy, dz)
        any_in, all_in = any_in | corner(inside, dx, dy, dz), all_in & corner(inside, dx, dy, dz)
    cells = (valid & any_in & ~all_in).to(torch.uint8)
    lo = corner(inside, 0, 0, 0)
    for a in range(3):
        hi = corner(inside, *[1 if k == a else 0 for k in range(3)])
        b, c = mesh._CYCLIC[a]
        sb, sc = [1 if k == b else 0 for k in range(3)], [1 if k == c else 0 for k in range(3)]
        around = valid & shift(valid, *sb) & shift(valid, *sc) & shift(valid, *[p + q for p, q in zip(sb, sc)])
        cells = cells | (((lo != hi) & around).to(torch.uint8) << (a + 1))
    return cells


def eager_raycast(field, rays, origin, vs, dims, h, w, step):
    """mesh.raycast_numpy's fixed-step march in eager PyTorch on the device, every sample evaluated, depth and status only (no normals or
    colours: less work than the kernel does) -> (depth [n,h,w], status [n,h,w] uint8).  One read-back: the longest ray's sample count."""
    nx, ny, nz = dims
    dev = field.device
    n = rays.shape[0]
    F = field.reshape(-1)
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing='ij')
    M = rays[:, :, None, None]
    d = [(M[:, 3 * a] * xs + M[:, 3 * a + 1] * ys) + M[:, 3 * a + 2] for a in range(3)]
    g0 = [((M[:, 9 + a] - origin[a]) / vs).expand(n, h, w) for a in range(3)]
    gd = [d[a] / vs for a in range(3)]
    s_in, s_out = torch.zeros(n, h, w, device=dev), torch.full((n, h, w), float('inf'), device=dev)
    ok = torch.ones(n, h, w, dtype=torch.bool, device=dev)
    for a in range(3):
        hi = float(dims[a] - 1)
        zero = gd[a] == 0
        t1, t2 = (0.0 - g0[a]) / gd[a], (hi - g0[a]) / gd[a]
        s_in = torch.where(zero, s_in, torch.maximum(s_in, torch.minimum(t1, t2)))
        s_out = torch.where(zero, s_out, torch.minimum(s_out, torch.maximum(t1, t2)))
        ok = ok & ~(zero & ((g0[a] < 0) | (g0[a] > hi)))
    ds = (step * vs) / torch.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    ok = ok & (s_in <= s_out) & (ds > 0)
    kmax = torch.where(ok, torch.floor((s_out - s_in) / ds), torch.full_like(ds, -1.0))
    prev = torch.full((n, h, w), float('nan'), device=dev)
    depth, status = torch.zeros(n, h, w, device=dev), torch.zeros(n, h, w, dtype=torch.uint8, device=dev)
    done = ~ok
    for k in range(int(kmax.max()) + 1):
        s = s_in + float(k) * ds
        idx, t = 0, []
        for a, (stride, cells) in enumerate(((1, nx - 1), (nx, ny - 1), (nx * ny, nz - 1))):
            g = g0[a] + s * gd[a]
            c = torch.clamp(torch.floor(torch.nan_to_num(g)), 0, cells - 1)
            t.append(g - c)
            idx = idx + c.long() * stride
        c = [F[idx + ((j >> 2) * ny + ((j >> 1) & 1)) * nx + (j & 1)] for j in range(8)]
        a4 = [c[2 * j] + t[0] * (c[2 * j + 1] - c[2 * j]) for j in range(4)]
        b0, b1 = a4[0] + t[1] * (a4[1] - a4[0]), a4[2] + t[1] * (a4[3] - a4[2])
        cur = b0 + t[2] * (b1 - b0)
        cross = ~done & (kmax >= k) & (prev == prev) & (cur == cur) & ((prev < 0) != (cur < 0))
        front = cross & (cur < 0)
        depth = torch.where(front, (s_in + float(k - 1) * ds) + ds * (prev / (prev - cur)), depth)
        status = torch.where(cross, torch.where(front, 1, 2).to(torch.uint8), status)
        done = done | cross
        prev = cur
    return depth, status


def timing_raycast(eng, vol, t_poses, t_Ks, h, w, eager_reps=2, step=0.5):
    """the raycast leg of --time on the fused volume: the kernel launch with and without block skipping (field, blocks and ray table
    prepared once), the preparation, TSDFVolume.raycast as a whole from host cameras, and the eager march"""
    state, dims, n = vol.state(), vol.dims, t_poses.shape[0]
    prep, last = {}, {}

    def run_prepare():
        prep['f'] = vol.field()
        prep['blocks'] = eng.surface_blocks(eng.surface_cells(state, dims), dims)
    ms_prep = _median_ms(run_prepare)
    src = {'f': prep['f'], 'csum': state.get('csum'), 'cw': state.get('cw')}
    poses, Ks = t_poses.cpu().numpy(), t_Ks.cpu().numpy()
    rays = eng.ray_table(poses, Ks)
    outs = ('depth', 'normal', 'colors', 'status', 'evaluated')

    def run_skip():                                   # (the launch alone: field, blocks and ray table prepared)
        last['skip'] = eng.tsdf_raycast(src, vol.origin, vol.voxel_size, dims, None, None, h, w, step, None, prep['blocks'], outs, rays=rays)

    def run_all():
        last['all'] = eng.tsdf_raycast(src, vol.origin, vol.voxel_size, dims, None, None, h, w, step, None, None, outs, rays=rays)

    def run_whole():                                  # (everything: field, cell and block bytes, the ray table from host cameras, the launch)
        last['whole'] = vol.raycast(poses, Ks, h, w, step=step)
    ms_skip, ms_all, ms_whole = _median_ms(run_skip), _median_ms(run_all), _median_ms(run_whole)

    def run_eager():
        last['eager'] = eager_raycast(prep['f'], rays, vol.origin, vol.voxel_size, dims, h, w, step)
    ms_eager = _median_ms(run_eager, reps=eager_reps, warmup=1)
    torch.cuda.synchronize(eng.device)
    a, b = last['skip'], last['all']
    ev_skip, ev_all = int(a['evaluated'].sum()), int(b['evaluated'].sum())
    same = all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in ('depth', 'normal', 'colors', 'status'))
    hits = b['status'] == 1
    e_depth, e_status = last['eager']
    both = hits & (e_status == 1)
    return {'raycast_48_views_ms' if n == 48 else 'raycast_ms': ms_skip, 'raycast_no_skip_ms': ms_all, 'raycast_prepare_ms': ms_prep,
            'raycast_with_prepare_ms': ms_whole, 'eager_raycast_ms': ms_eager, 'raycast_step': step, 'raycast_hits': int(hits.sum()),
            'raycast_evaluated': ev_skip, 'raycast_evaluated_no_skip': ev_all, 'raycast_flagged_blocks': int(prep['blocks'].sum()),
            'raycast_blocks': int(prep['blocks'].numel()), 'raycast_evaluations_per_s': ev_skip / (ms_skip * 1e-3),
            'raycast_evaluations_per_s_no_skip': ev_all / (ms_all * 1e-3), 'raycast_skip_bitwise_equal': bool(same),
            'eager_raycast_status_agreement': float((e_status == b['status']).float().mean()),
            'eager_raycast_depth_within_1e-5': float(((e_depth - b['depth'])[both].abs() <= 1e-5).float().mean()) if bool(both.any()) else None,
            'eager_raycast_depth_max_diff': float((e_depth - b['depth'])[both].abs().max()) if bool(both.any()) else None,
            'eager_raycast_reps': eager_reps}


def timing(n=48, size=800, points=256, eager_reps=3):
    from .engine import host_inverse
    dev = torch.device('cuda:0')
    eng = procedural._device_engine(dev)
    if eng is None:
        raise SystemExit("neuray_amd.export_mesh: --time needs the HIP device")
    h = w = size
    poses = procedural.ring_cameras(np.random.RandomState(1), n)
    Ks = np.repeat(procedural.intrinsics(h, w)[None], n, 0)
    t_poses, t_Ks, t_Ki = torch.from_numpy(poses).to(dev), torch.from_numpy(Ks).to(dev), host_inverse(torch.from_numpy(Ks)).to(dev)
    view = eng.procedural_render(procedural.make_scene(1), t_poses, None, h, w, 1, Ks_inv=t_Ki, outputs=('depth',))
    depth, rgb = view['depth'], view['rgb']
    radius = float(procedural.SCENE_RADIUS)
    vs = 2 * radius / (points - 1)
    origin, dims, trunc = (-radius, -radius, -radius), (points, points, points), 3 * vs
    vol = mesh.TSDFVolume(origin, vs, dims, trunc, engine=eng)
    state = vol.state()

    def run_integrate():
        for t in state.values():
            t.zero_()
        vol.integrate(depth, rgb, t_poses, t_Ks)

    def run_zero():
        for t in state.values():
            t.zero_()
    ms_zero = _median_ms(run_zero)
    ms_i = _median_ms(run_integrate) - ms_zero
    last = {}

    def run_extract():
        last.update(vol.extract())
    ms_e = _median_ms(run_extract)

    def run_cells():
        last['cells'] = eng.surface_cells(state, dims)
    ms_cells = _median_ms(run_cells)
    torch.cuda.synchronize(dev)
    m, k = int(last['vertices'].shape[0]), int(last['faces'].shape[0])
    lattice, cells = points ** 3, (points - 1) ** 3
    # compulsory traffic.  integration: the six words of state read and written once per call (the gathers - up to 48 depth and 144 colour
    # texels per lattice point, through the caches - are not counted); extraction: W and Tsum read once by each kernel, the colour state by
    # the second; the cell bytes written and read; two int64 offsets per cell written by the scan and read by the second kernel; the outputs
    bytes_i = lattice * 6 * 4 * 2
    bytes_e = lattice * (2 * 4 + 6 * 4) + cells * (1 + 1 + 2 * 8 * 2) + m * 36 + k * 12
    P, K = torch.from_numpy(poses), torch.from_numpy(Ks)
    eager = {}

    def run_eager_i():
        z = {kk: torch.zeros_like(v) for kk, v in state.items()}
        eager.update(eager_integrate(z, depth, rgb, P, K, origin, vs, dims, trunc))
    ms_ei = _median_ms(run_eager_i, reps=eager_reps, warmup=1)

    def run_eager_c():
        eager['cells'] = eager_cells(state['tsum'], state['w'], 1.0)
    ms_ec = _median_ms(run_eager_c, reps=eager_reps, warmup=1)
    w_agree = float((eager['w'] == state['w']).float().mean())
    cells_agree = float((eager['cells'] == last['cells']).float().mean())
    dist = geometry.surface_distance(procedural.make_scene(1), last['vertices'])
    cast = timing_raycast(eng, vol, t_poses, t_Ks, h, w)
    return {**cast, 'views': n, 'h': h, 'w': w, 'dims': list(dims), 'voxel_size': vs, 'trunc': trunc, 'vertices': m, 'faces': k,
            'boundary_edges': mesh.boundary_edges(last['faces']),
            'surface_distance': {'median': float(np.median(dist)), 'p95': float(np.percentile(dist, 95))},
            'integrate_48_views_ms' if n == 48 else 'integrate_ms': ms_i, 'state_zero_ms': ms_zero, 'extract_ms': ms_e, 'surface_cells_ms': ms_cells,
            'integrate_hbm_share': bytes_i / (ms_i * 1e-3) / HBM_PEAK, 'extract_hbm_share': bytes_e / (ms_e * 1e-3) / HBM_PEAK,
            'hbm_peak_bytes_per_s': HBM_PEAK, 'eager_integrate_ms': ms_ei, 'eager_cells_only_ms': ms_ec, 'eager_w_agreement': w_agree,
            'eager_cells_agreement': cells_agree, 'reps': 20, 'eager_reps': eager_reps}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--database', type=str, default=None, help="e.g. procedural/0/white_800")
    ap.add_argument('--depth', choices=('database', 'render', 'stereo'), default='database')
    ap.add_argument('--cfg', type=str, default=None)
    ap.add_argument('--ckpt', type=str, default=None)
    ap.add_argument('--out', type=str, default='mesh.ply')
    ap.add_argument('--voxel', type=float, default=None, help='voxel size (default: 256 lattice points on the longest side)')
    ap.add_argument('--trunc', type=float, default=None, help='truncation distance (default: 3 voxels)')
    ap.add_argument('--min-weight', type=float, default=1.0)
    ap.add_argument('--no-filter', action='store_true', help='integrate the depth maps as they are, without geometry.filter_depth')
    ap.add_argument('--src', type=int, default=geometry.DEFAULTS['src'])
    ap.add_argument('--tau-px', type=float, default=geometry.DEFAULTS['tau_px'])
    ap.add_argument('--tau-d', type=float, default=geometry.DEFAULTS['tau_d'])
    ap.add_argument('--min-views', type=int, default=geometry.DEFAULTS['min_views'])
    ap.add_argument('--json', type=str, default=None, help='write the result line here as well')
    ap.add_argument('--raycast', type=str, default=None, help='cast the fused volume from every view and write DIR/<view id>.npz')
    ap.add_argument('--step', type=float, default=0.5, help='sample spacing of --raycast in voxels, in (0, 0.95]')
    ap.add_argument('--time', action='store_true')
    args = ap.parse_args(argv)
    if args.time:
        res = timing()
    else:
        if not args.database:
            ap.error('--database is required')
        if (args.voxel is not None and not args.voxel > 0) or (args.trunc is not None and not args.trunc > 0) or not args.min_weight > 0:
            ap.error('--voxel, --trunc and --min-weight must be positive')
        if not 0 < args.step <= mesh.MAX_STEP:
            ap.error('--step must be in (0, %g]' % mesh.MAX_STEP)
        if not 1 <= args.src <= geometry.MAX_SRC:
            ap.error('--src must be in 1 .. %d' % geometry.MAX_SRC)
        res = export(args)
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == '__main__':
    main()
