"""Times the plane sweep (csrc/nr_kernels_stereo.h) on a procedural database and scores its depth.

    python tools/bench_stereo.py [--database procedural/0/white_800 --src 4 --planes 128 --radius 2 --reps 20 --eager-views 2 --mesh]

Device events around RenderEngine.plane_sweep over all views, median of --reps; in the same process an eager PyTorch composition of the same
formulas (grid_sample + avg_pool2d, per view and plane, on --eager-views views) for the ratio; coverage and depth error against the true
depth, photometric and after the geometric filter; with --mesh the fuse_mesh surface error from the stereo depth.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuray_amd import geometry, procedural, stereo  # noqa: E402
from neuray_amd.pipeline import build_imgs_info  # noqa: E402

HBM_PEAK = 8.0e12          # bytes per second (MI355X, HBM3E)


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def eager_sweep(gray, cams, rng, nn, view, planes, radius, var_min=stereo.VAR_MIN):
    """the formulas of stereo.plane_sweep_numpy for one view in eager PyTorch (window sums by avg_pool2d: not the reference's order)"""
    n, h, w = gray.shape
    dev = gray.device
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing='ij')
    pool = lambda a: F.avg_pool2d(a[None, None], 2 * radius + 1, 1)[0, 0]          # noqa: E731
    A = gray[view]
    m_r = pool(A)
    v_r = pool(A * A) - m_r * m_r
    best = torch.full_like(m_r, float('inf'))
    best_k = torch.full_like(m_r, -1)
    used = [(s, int(j)) for s, j in enumerate(nn[view]) if 0 <= int(j) < n and int(j) != view]
    need = 1 if len(used) == 1 else 2
    for k in range(planes):
        t = k / (planes - 1)
        d = 1.0 / ((1 - t) / float(rng[view, 0]) + t / float(rng[view, 1]))
        costs = []
        for s, j in used:
            M = cams[view, s]
            q0 = d * (M[0] * xs + M[1] * ys + M[2]) + M[9]
            q1 = d * (M[3] * xs + M[4] * ys + M[5]) + M[10]
            q2 = d * (M[6] * xs + M[7] * ys + M[8]) + M[11]
            u, v = q0 / q2, q1 / q2
            ok = (q2 > 0) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
            grid = torch.stack([u / (w - 1) * 2 - 1, v / (h - 1) * 2 - 1], -1)[None]
            B = F.grid_sample(gray[j][None, None], grid, mode='bilinear', padding_mode='zeros', align_corners=True)[0, 0]
            okw = pool(ok.float()) > 1 - 1e-6
            m_s = pool(B)
            v_s = pool(B * B) - m_s * m_s
            c = (1 - (pool(A * B) - m_r * m_s) / torch.sqrt(v_r * v_s)).clamp(0, 2)
            costs.append(torch.where(okw & (v_r >= var_min) & (v_s >= var_min), c, torch.full_like(c, float('inf'))))
        srt = torch.sort(torch.stack(costs), 0)[0]
        m = torch.isfinite(srt).sum(0)
        kk = (m + 1) // 2
        take = torch.arange(srt.shape[0], device=dev)[:, None, None] < kk[None]
        agg = torch.where(take, srt, torch.zeros_like(srt)).sum(0) / kk.clamp(min=1)
        agg = torch.where((m >= need) & (m > 0), agg, torch.full_like(agg, float('inf')))
        better = agg < best
        best, best_k = torch.where(better, agg, best), torch.where(better, torch.full_like(best_k, k), best_k)
    return best, best_k


def score(depth, true):
    ok = (depth > 0) & (true > 0)
    err = np.abs(depth - true)[ok] / true[ok]
    return {'coverage': float(ok.sum() / max((true > 0).sum(), 1)), 'median_rel_error': float(np.median(err)) if err.size else None,
            'outside_surface': float(((depth > 0) & ~(true > 0)).sum() / max((depth > 0).sum(), 1))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--database', default='procedural/0/white_800')
    ap.add_argument('--src', type=int, default=4)
    ap.add_argument('--planes', type=int, default=128)
    ap.add_argument('--radius', type=int, default=2)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--eager-views', type=int, default=2)
    ap.add_argument('--mesh', action='store_true')
    args = ap.parse_args(argv)
    eng = procedural._device_engine()
    if eng is None:
        raise SystemExit("tools/bench_stereo.py needs the HIP device")
    from neuray_amd import database as _database
    db = _database.parse_database_name(args.database)
    ids = db.get_img_ids()
    info = build_imgs_info(db, ids)
    true = np.ascontiguousarray(info['depth'][:, 0])
    n, _, h, w = info['imgs'].shape
    nn = geometry.nearest_sources(info['poses'], args.src)
    imgs = torch.from_numpy(np.ascontiguousarray(info['imgs'], dtype=np.float32)).to(eng.device)
    sweep = lambda: eng.plane_sweep(imgs, info['poses'], info['Ks'], info['depth_range'], nn, args.planes, args.radius)     # noqa: E731
    res = sweep()
    torch.cuda.synchronize()
    ms = median_ms(sweep, args.reps)
    warps = float(n) * h * w * args.planes * (nn >= 0).sum(1).mean()        # one bilinear warp per (pixel, plane, used source), halo not counted
    compulsory = n * h * w * (3 * 4 + 4 + 3 * 4) + n * h * w * 4 * args.src            # imgs in, gray out, three maps out; each source's gray once per view
    out = {'database': args.database, 'views': n, 'h': h, 'w': w, 'src': args.src, 'planes': args.planes, 'radius': args.radius,
           'sweep_ms': ms, 'ms_per_view': ms / n, 'warps_per_s': warps / (ms * 1e-3), 'compulsory_hbm_share': compulsory / (ms * 1e-3) / HBM_PEAK}
    if args.eager_views > 0:
        gray = torch.from_numpy(stereo.gray_numpy(info['imgs'], np.float32)).to(eng.device)
        cams = torch.from_numpy(stereo.sweep_constants(info['poses'], info['Ks'], nn)).to(eng.device)
        views = list(range(min(args.eager_views, n)))
        eager = lambda: [eager_sweep(gray, cams, info['depth_range'], nn, v, args.planes, args.radius) for v in views]       # noqa: E731
        got = eager()
        torch.cuda.synchronize()
        ems = median_ms(eager, 3) / len(views)
        r = args.radius
        same = [float((got[v][1].cpu().numpy() == res['plane'][v, r:h - r, r:w - r].cpu().numpy()).mean()) for v in views]
        out.update(eager_ms_per_view=ems, eager_over_kernel=ems / (ms / n), eager_same_plane=float(np.mean(same)))
    photo = torch.where(res['cost'] > stereo.DEFAULTS['max_cost'], torch.zeros_like(res['depth']), res['depth'])
    flt = geometry.filter_depth(photo, info['poses'], info['Ks'], nn, engine=eng)['depth']
    out['photometric'] = score(photo.cpu().numpy(), true)
    out['geometric'] = score(flt.cpu().numpy(), true)
    if args.mesh:
        from neuray_amd import mesh
        m = mesh.fuse_mesh(flt.cpu().numpy(), info['imgs'], info['poses'], info['Ks'], filter=False)
        dist = geometry.surface_distance(db.scene, m['vertices'])
        out['mesh'] = {'vertices': int(m['vertices'].shape[0]), 'surface_distance_median': float(np.median(dist)),
                       'surface_distance_p95': float(np.percentile(dist, 95))}
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
