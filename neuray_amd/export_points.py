"""Geometry export from the command line (neuray_amd/geometry.py):

    python -m neuray_amd.export_points --database NAME --depth database|render|stereo [--cfg CFG --ckpt CKPT] --out cloud.ply
                                       [--src 8 --tau-px 1 --tau-d 0.01 --min-views 2 --tau-n 0.05 --no-dedup --json out.json]

fuses the depth maps of every view of a database - its own (`--depth database`), plane-sweep stereo of its images (`--depth stereo`, neuray_amd.stereo), or the `render_depth_fine` of a renderer that renders each
view from its nearest other views (`--depth render`; --cfg: the renderer's cfg as JSON, or YAML where PyYAML is installed, --ckpt: its
weights, a state_dict or a checkpoint with 'network_state_dict') - into one point cloud and writes it as a binary PLY with normals and
colours.  For a procedural scene the printed line carries the distance of the points to the true surface.

    python -m neuray_amd.export_points --time

measures the two kernels on the MI355X at 48 views of 800 x 800 with 8 source views each - depth_consistency (one launch) and the 48 fuse_view
launches - with device events, the median of 20 after warm-up, next to an eager PyTorch composition of the same formulas in the same
process, and reports the share of the HBM peak that the compulsory traffic amounts to.  One JSON line."""
import argparse
import json

import numpy as np
import torch

from . import database as _database
from . import geometry, procedural

HBM_PEAK = 8.0e12          # bytes per second (MI355X, HBM3E)


def _load_cfg(path):
    with open(path) as f:
        text = f.read()
    try:
        return json.loads(text)
    except ValueError:
        import yaml
        return yaml.safe_load(text)


def _renderer(cfg_path, ckpt_path, db, ids, device):
    from .network.renderer import name2network
    cfg = _load_cfg(cfg_path)
    kind = cfg.get('network', 'neuray_gen')
    if kind == 'neuray_ft':
        from .pipeline import build_imgs_info
        net = name2network[kind](cfg, scene={'ref_imgs_info': build_imgs_info(db, ids), 'database': db})
    else:
        net = name2network[kind](cfg)
    if ckpt_path:
        state = torch.load(ckpt_path, map_location='cpu')
        net.load_state_dict(state.get('network_state_dict', state), strict=True)
    return net.eval().to(device)


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
            raise SystemExit("neuray_amd.export_points: --depth render needs --cfg (and usually --ckpt)")
        if not torch.cuda.is_available():
            raise SystemExit("neuray_amd.export_points: --depth render needs the HIP device (the render path has no CPU fallback)")
        maps = geometry.render_depth_maps(_renderer(args.cfg, args.ckpt, db, ids, 'cuda:0'), db, ids)
    cloud = geometry.fuse_points(maps['depth'], maps['imgs'], maps['poses'], maps['Ks'], src=args.src, tau_px=args.tau_px, tau_d=args.tau_d,
                                 min_views=args.min_views, tau_n=args.tau_n, dedup=not args.no_dedup)
    geometry.write_ply(args.out, cloud['points'], cloud['colors'], cloud['normals'])
    n, h, w = maps['depth'].shape
    res = {'database': args.database, 'depth': args.depth, 'views': n, 'h': h, 'w': w, 'points': int(cloud['points'].shape[0]),
           'pixels_with_depth': int((maps['depth'] > 0).sum()), 'out': args.out,
           'on': 'hip' if procedural._device_engine() is not None else 'numpy',
           'settings': {'src': args.src, 'tau_px': args.tau_px, 'tau_d': args.tau_d, 'min_views': args.min_views, 'tau_n': args.tau_n,
                        'dedup': not args.no_dedup}}
    if isinstance(db, procedural.ProceduralDatabase) and res['points']:
        dist = geometry.surface_distance(db.scene, cloud['points'])
        res['surface_distance'] = {'mean': float(dist.mean()), 'median': float(np.median(dist)), 'max': float(dist.max())}
    return res


# ---- --time --------------------------------------------------------------------------------------------------------------------------
def _t_unproject(Rt, Ki, px, py, d):
    a = [(Ki[k, 0] * px + Ki[k, 1] * py + Ki[k, 2]) * d - Rt[k, 3] for k in range(3)]
    return [Rt[0, c] * a[0] + Rt[1, c] * a[1] + Rt[2, c] * a[2] for c in range(3)]


def _t_project(Rt, K, X):
    c = [Rt[k, 0] * X[0] + Rt[k, 1] * X[1] + Rt[k, 2] * X[2] + Rt[k, 3] for k in range(3)]
    q = [K[k, 0] * c[0] + K[k, 1] * c[1] + K[k, 2] * c[2] for k in range(3)]
    return q[0] / q[2], q[1] / q[2], c[2]


def eager_consistency(depth, P, K, Ki, nn, tau_px, tau_d):
    """geometry.consistency_numpy in eager PyTorch on the device (P, K, Ki, nn: host tensors - their entries become kernel constants,
    as the kernels read them through scalar loads) -> count, fused_depth, consistent_bits, texels [n][S]"""
    n, h, w = depth.shape
    dev = depth.device
    ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
    fx, fy = xs.float(), ys.float()
    P, K, Ki = P.tolist(), K.tolist(), Ki.tolist()
    idx = lambda M: {(r, c): M[r][c] for r in range(len(M)) for c in range(len(M[0]))}      # noqa: E731
    counts, fds, bits_all, tex_all = [], [], [], []
    for i in range(n):
        Pi, Kii, Kiii = idx(P[i]), idx(K[i]), idx(Ki[i])
        d = depth[i]
        have = d > 0
        X = _t_unproject(Pi, Kiii, fx, fy, d)
        acc, count, bits, texels = d.clone(), torch.zeros(h, w, dtype=torch.int32, device=dev), torch.zeros(h, w, dtype=torch.int32, device=dev), []
        for s, j in enumerate(nn[i]):
            if j < 0 or j == i or j >= n:
                texels.append(None)
                continue
            Pj, Kj, Kij = idx(P[j]), idx(K[j]), idx(Ki[j])
            u, v, z = _t_project(Pj, Kj, X)
            un, vn = torch.floor(u + 0.5), torch.floor(v + 0.5)
            inb = have & (z > 0) & (un >= 0) & (un < w) & (vn >= 0) & (vn < h)
            t = torch.where(inb, vn, torch.zeros_like(vn)).long() * w + torch.where(inb, un, torch.zeros_like(un)).long()
            dj = torch.where(inb, depth[j].reshape(-1)[t], torch.zeros_like(d))
            seen = inb & (dj > 0)
            u2, v2, qz = _t_project(Pi, Kii, _t_unproject(Pj, Kij, un, vn, dj))
            ok = seen & (qz > 0) & ((u2 - fx) ** 2 + (v2 - fy) ** 2 < tau_px * tau_px) & ((qz - d).abs() / d < tau_d)
            acc = torch.where(ok, acc + qz, acc)
            count = count + ok
            bits = bits | (ok.int() << s)
            texels.append(torch.where(seen, t, torch.full_like(t, -1)))
        counts.append(count)
        fds.append(torch.where(have, acc / (count + 1).float(), torch.zeros_like(d)))
        bits_all.append(bits)
        tex_all.append(texels)
    return torch.stack(counts), torch.stack(fds), torch.stack(bits_all), tex_all


def eager_fuse(depth, rgb, P, Ki, nn, count, fd, bits, texels, min_views):
    """the fusion's emit / taken / xyz / colour in eager PyTorch (the normals are left out: the eager side does less work than the kernel)"""
    n, h, w = depth.shape
    dev = depth.device
    ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
    fx, fy = xs.float(), ys.float()
    taken = torch.zeros(n, h * w, dtype=torch.uint8, device=dev)
    flat = rgb.reshape(n, 3, h * w)
    P, Ki = P.tolist(), Ki.tolist()
    idx = lambda M: {(r, c): M[r][c] for r in range(len(M)) for c in range(len(M[0]))}      # noqa: E731
    out = []
    for i in range(n):
        emit = (count[i] >= min_views) & (taken[i].reshape(h, w) == 0)
        col = rgb[i].clone()
        for s, j in enumerate(nn[i]):
            if texels[i][s] is None:
                continue
            on = emit & (((bits[i] >> s) & 1) > 0)
            t = torch.where(on, texels[i][s], torch.zeros_like(texels[i][s]))
            taken[j].scatter_reduce_(0, t.reshape(-1), on.reshape(-1).to(torch.uint8), 'amax')      # (no boolean index: no read-back)
            col = col + torch.where(on[None], flat[j][:, t.reshape(-1)].reshape(3, h, w), torch.zeros_like(col))
        xyz = torch.stack(_t_unproject(idx(P[i]), idx(Ki[i]), fx, fy, fd[i]), -1)
        out.append((emit, torch.where(emit[..., None], xyz, torch.zeros_like(xyz)), col / (count[i] + 1).float()))
    return out


def _median_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def timing(n=48, size=800, src=8, eager_reps=3):
    from .engine import host_inverse
    dev = torch.device('cuda:0')
    eng = procedural._device_engine(dev)
    h = w = size
    poses = procedural.ring_cameras(np.random.RandomState(1), n)
    Ks = np.repeat(procedural.intrinsics(h, w)[None], n, 0)
    Ki = host_inverse(torch.from_numpy(Ks))
    nn = geometry.nearest_sources(poses, src)
    t_poses, t_Ks, t_Ki, t_nn = torch.from_numpy(poses).to(dev), torch.from_numpy(Ks).to(dev), Ki.to(dev), torch.from_numpy(nn).to(dev)
    view = eng.procedural_render(procedural.make_scene(1), t_poses, None, h, w, 1, Ks_inv=t_Ki, outputs=('depth',))
    depth, rgb = view['depth'], view['rgb']
    cons = {}

    def run_consistency():
        cons.update(eng.depth_consistency(depth, t_poses, t_Ks, t_nn, Ks_inv=t_Ki, outputs=('count', 'fused_depth', 'consistent_bits', 'occluded_bits')))
    ms_c = _median_ms(run_consistency)
    taken = torch.zeros(n, h, w, dtype=torch.uint8, device=dev)
    last = {}

    def run_fuse():
        taken.zero_()
        for i in range(n):
            last[i] = eng.fuse_view(i, depth, rgb, t_poses, t_Ks, t_nn, cons, taken, Ks_inv=t_Ki)
    ms_f = _median_ms(run_fuse)
    torch.cuda.synchronize(dev)
    valid = float((depth > 0).float().mean())
    mean_count = float(cons['count'].float().mean())
    points = int(sum(int(v['emit'].sum()) for v in last.values()))
    px = n * h * w
    # compulsory traffic.  consistency: the pixel's depth, one source depth per slot (a 4-byte gather), count + fused depth + two bit masks;
    # fusion: depth, count, fused depth, bits, taken, colour in; emit, xyz, colour, normal out; a colour gather per consistent slot
    bytes_c = px * (4 + 4 * src + 1 + 4 + 4 + 4)
    bytes_f = px * (4 + 1 + 4 + 4 + 1 + 12 + 1 + 36) + px * mean_count * 12 + px
    tbl = [[int(j) for j in row] for row in nn]
    eager_out = {}

    def run_eager_c():
        eager_out['c'] = eager_consistency(depth, torch.from_numpy(poses), torch.from_numpy(Ks), Ki, tbl, 1.0, 0.01)
    ms_ec = _median_ms(run_eager_c, reps=eager_reps, warmup=1)
    cnt, fd, bits, tex = eager_out['c']
    ms_ef = _median_ms(lambda: eager_fuse(depth, rgb, torch.from_numpy(poses), Ki, tbl, cnt, fd, bits, tex, 2), reps=eager_reps, warmup=1)
    agree = float((cnt.to(torch.uint8) == cons['count']).float().mean())
    return {'views': n, 'h': h, 'w': w, 'src': src, 'pixels_with_depth': valid, 'mean_consistent_slots': mean_count, 'points': points,
            'depth_consistency_ms': ms_c, 'fuse_48_views_ms' if n == 48 else 'fuse_views_ms': ms_f,
            'depth_consistency_hbm_share': bytes_c / (ms_c * 1e-3) / HBM_PEAK, 'fuse_hbm_share': bytes_f / (ms_f * 1e-3) / HBM_PEAK,
            'hbm_peak_bytes_per_s': HBM_PEAK, 'eager_consistency_ms': ms_ec, 'eager_fuse_without_normals_ms': ms_ef,
            'eager_count_agreement': agree, 'reps': 20, 'eager_reps': eager_reps}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--database', type=str, default=None, help="e.g. procedural/0/white_800")
    ap.add_argument('--depth', choices=('database', 'render', 'stereo'), default='database')
    ap.add_argument('--cfg', type=str, default=None)
    ap.add_argument('--ckpt', type=str, default=None)
    ap.add_argument('--out', type=str, default='cloud.ply')
    ap.add_argument('--src', type=int, default=geometry.DEFAULTS['src'])
    ap.add_argument('--tau-px', type=float, default=geometry.DEFAULTS['tau_px'])
    ap.add_argument('--tau-d', type=float, default=geometry.DEFAULTS['tau_d'])
    ap.add_argument('--min-views', type=int, default=geometry.DEFAULTS['min_views'])
    ap.add_argument('--tau-n', type=float, default=geometry.DEFAULTS['tau_n'])
    ap.add_argument('--no-dedup', action='store_true')
    ap.add_argument('--json', type=str, default=None, help='write the result line here as well')
    ap.add_argument('--time', action='store_true')
    args = ap.parse_args(argv)
    if args.time:
        res = timing()
    else:
        if not args.database:
            ap.error('--database is required')
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
