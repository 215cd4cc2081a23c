"""Procedural ground truth at work: what the ray-cast kernel costs, and a first look at image quality against
ground truth - a NeuralRayFtRenderer trained from scratch on one procedural scene, its held-out views rendered in three modes.

    python tools/train_procedural.py --time
        kernel time (device events, median of 20 after warm-up) of one ProceduralStream batch - 13 views of 416 x 608, ss 1 and 2 - and of
        one 800 x 800 view, and the generalisation step of bench.gen_train_case fed by its fixed batch against the same step fed by the
        stream, in one process.  One JSON line.  With --augment additionally the kernel time per batch of the three augmentation entries
        (augment_stats, augment_depth, sample_coords: DESIGN.md 4.23) next to the render launch of the same batch, and the generalisation
        step fed by the augmented stream.
    python tools/train_procedural.py --scene procedural/0/white_800 --steps N
        trains every network of a NeuralRayFtRenderer on the scene's 42 training views (render + consistency loss of neuray_amd.loss, Adam),
        then renders the 6 held-out views with hip_arith f32 / x3 and the network coarse pass, and x3 with hip_coarse_pass = 'visibility':
        PSNR / SSIM (engine.image_metrics) against the ray-cast images and the rendered depth against the true depth.  One JSON line.
        With --export-points the rendered depth of the training views is fused into a point cloud in each of the three modes
        (neuray_amd/geometry.py) and the line gains, per mode, the point count, the mean / median distance of the points to the
        true surface and the completeness at 2 x tau_d x mean depth: the share of the held-out views' back-projected true-depth pixels that
        have a fused point within that radius.

These numbers are about ONE procedurally generated scene and a model trained from scratch for minutes - not the paper's checkpoints."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuray_amd import database, geometry, pipeline, procedural  # noqa: E402
from neuray_amd.loss import name2loss, total_loss  # noqa: E402
from neuray_amd.network import render_ops  # noqa: E402


def median_ms(fn, reps=20, warmup=3):
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


def kernel_times(dev):
    eng = render_ops.engine_for(dev)
    res = {}
    from neuray_amd.engine import host_inverse
    scene = procedural.make_scene(1)
    t_scene = torch.from_numpy(scene).to(dev)
    for tag, n, h, w in (('stream_batch_13x416x608', 13, 416, 608), ('one_view_800x800', 1, 800, 800)):
        t_poses = torch.from_numpy(procedural.ring_cameras(np.random.RandomState(1), n)).to(dev)
        Ks_inv = host_inverse(torch.from_numpy(procedural.intrinsics(h, w)[None])).repeat(n, 1, 1).to(dev)
        for ss in (1, 2):
            res['%s_ss%d_ms' % (tag, ss)] = median_ms(lambda: eng.procedural_render(t_scene, t_poses, None, h, w, ss, Ks_inv=Ks_inv,
                                                                                    outputs=('depth', 'mask')))
    res['prims'] = procedural.scene_prims(scene)
    return res


def augment_times(dev, reps=20, warmup=3):
    """device-event time per batch of every engine entry a ProceduralStream batch with augmentation launches (median of `reps`)"""
    eng = render_ops.engine_for(dev)
    stream = procedural.ProceduralStream(dev, seed=0, h=416, w=608, rfn=8, extra_src=4, rays=512, augment=True, engine=eng)
    for _ in range(warmup):
        next(stream)
    per = {}
    for _ in range(reps):
        eng.timing = []
        next(stream)
        torch.cuda.synchronize(dev)
        batch = {}
        for name, e0, e1, _n in eng.timing:
            batch[name] = batch.get(name, 0.0) + e0.elapsed_time(e1)
        for name, ms in batch.items():
            per.setdefault(name, []).append(ms)
    eng.timing = None
    return {'augment_batch_13x416x608_%s_ms' % ('render' if k == 'procedural' else k): float(np.median(v)) for k, v in per.items()}


def gen_step_times(dev, steps=10, augment=False):
    """bench.gen_train_case's loop on its fixed batch, then the same model / optimiser / losses on a fresh stream batch per step"""
    import bench
    model, opt, step = bench.gen_train_case(dev, host_ks_inv=True)
    rfn, h, w = 8, 416, 608

    def timed(fn):
        for _ in range(6):
            fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t0) / steps
    fixed = timed(step)
    stream = procedural.ProceduralStream(dev, seed=0, h=h, w=w, rfn=rfn, extra_src=4, rays=512)

    def stream_step():
        batch = next(stream)
        ref = batch['ref_imgs_info']
        opt.zero_grad(set_to_none=True)
        out = model({k: dict(v) if isinstance(v, dict) else v for k, v in batch.items()})
        gt = out['pixel_colors_gt']
        loss = ((out['pixel_colors_nr'] - gt) ** 2).mean() + ((out['pixel_colors_nr_fine'] - gt) ** 2).mean()
        c = out['depth_coords'].long()
        d = ref['true_depth'][torch.arange(rfn, device=dev)[:, None], 0, c[..., 1].clamp(max=h - 1), c[..., 0].clamp(max=w - 1)]
        near, far = -1 / ref['depth_range'][:, 0:1], -1 / ref['depth_range'][:, 1:2]
        d = (((-1 / d.clamp(min=1e-5)) - near) / (far - near)).clamp(0, 1)
        loss = loss + ((d - out['depth_mean']) ** 2).mean() + ((d - out['depth_mean_fine']) ** 2).mean()
        loss.backward()
        opt.step()
    res = {'gen_step_fixed_batch_ms': fixed, 'gen_step_stream_ms': timed(stream_step)}
    if augment:
        stream = procedural.ProceduralStream(dev, seed=0, h=h, w=w, rfn=rfn, extra_src=4, rays=512, augment=True)
        res['gen_step_stream_augment_ms'] = timed(stream_step)
    render_ops.check_deferred_inputs(dev, wait=True)
    return res


def evaluate(ft, db, val_ids, dev):
    """the held-out views in the three modes -> {mode: {psnr, ssim, depth_abs_err, ms_per_image}}"""
    modes = (('f32_network', 'f32', 'network'), ('x3_network', 'x3', 'network'), ('x3_visibility', 'x3', 'visibility'))
    gt = ft.val_imgs_info['imgs'].to(dev)
    n, _, h, w = gt.shape
    true_depth = torch.from_numpy(np.stack([db.get_depth(i) for i in val_ids])).to(dev)
    mask = torch.from_numpy(np.stack([db.get_mask(i) for i in val_ids])).to(dev)
    res = {}
    ft.eval()
    for tag, arith, coarse in modes:
        ft.cfg['hip_arith'], ft.cfg['hip_coarse_pass'] = arith, coarse
        ft.__dict__['_engine'] = None                      # the next render builds the engine of this arithmetic
        eng = render_ops.engine_for(dev)
        psnr, ssim, derr, ms = [], [], [], []
        for vi in range(n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.no_grad():
                out = ft({'index': vi, 'eval': True})
            torch.cuda.synchronize(dev)
            ms.append(1e3 * (time.perf_counter() - t0))
            m = eng.image_metrics(out['pixel_colors_nr_fine'].reshape(1, h * w, 3).contiguous(),
                                  gt[vi].permute(1, 2, 0).reshape(1, h * w, 3).contiguous(), h, w)
            psnr.append(float(m['psnr'][0]))
            ssim.append(float(m['ssim'][0]))
            rd = out.get('render_depth_fine', out.get('render_depth'))
            if rd is not None:
                rd = rd.reshape(h, w)
                derr.append(float((rd - true_depth[vi]).abs()[mask[vi]].mean()))
        res[tag] = {'psnr': float(np.mean(psnr)), 'ssim': float(np.mean(ssim)), 'depth_abs_err': float(np.mean(derr)) if derr else None,
                    'ms_per_image': float(np.median(ms))}
    return res


def within_radius(points, queries, radius):
    """[q] bool: some point lies within `radius` of the query.  A voxel hash of cell size `radius` (sorted integer keys, searchsorted) finds
    the candidates: the 27 cells around the query's cell; the distance is then checked exactly."""
    lo = torch.minimum(points.min(0).values, queries.min(0).values) - radius
    cell = lambda x: ((x - lo) / radius).floor().long()                    # noqa: E731
    dims = cell(torch.maximum(points.max(0).values, queries.max(0).values)) + 2
    key = lambda c: (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]      # noqa: E731
    keys, order = torch.sort(key(cell(points)))
    pts = points[order]
    found = torch.zeros(queries.shape[0], dtype=torch.bool, device=queries.device)
    qc = cell(queries)
    width = int(torch.unique_consecutive(keys, return_counts=True)[1].max()) if keys.numel() else 0
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = key(qc + torch.tensor([dx, dy, dz], device=qc.device))
                start = torch.searchsorted(keys, k)
                for o in range(width):                                      # (at most `width` points share a cell)
                    i = (start + o).clamp(max=keys.numel() - 1)
                    hit = (keys[i] == k) & (start + o < keys.numel())
                    found |= hit & (((pts[i] - queries) ** 2).sum(-1) <= radius * radius)
    return found


def export_points(ft, db, train_ids, val_ids, dev, tau_d=0.01):
    """the rendered depth of the training views, fused, in the three render modes -> {mode: {points, surface_mean, surface_median,
    completeness, radius}}"""
    from neuray_amd.engine import host_inverse
    val = geometry.database_depth_maps(db, val_ids)
    d = torch.from_numpy(val['depth']).to(dev)
    n, h, w = d.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1).float()
    Ki, P = host_inverse(torch.from_numpy(val['Ks'])).to(dev), torch.from_numpy(val['poses']).to(dev)
    cam = torch.einsum('nij,hwj->nhwi', Ki, pix) * d[..., None]
    truth = torch.einsum('nji,nhwj->nhwi', P[:, :, :3], cam - P[:, None, None, :, 3])[d > 0]         # R^T (K^-1 [x,y,1] d - t)
    radius = 2 * tau_d * float(d[d > 0].mean())
    res = {}
    ft.eval()
    for tag, arith, coarse in (('f32_network', 'f32', 'network'), ('x3_network', 'x3', 'network'), ('x3_visibility', 'x3', 'visibility')):
        ft.cfg['hip_arith'], ft.cfg['hip_coarse_pass'] = arith, coarse
        ft.__dict__['_engine'] = None
        maps = geometry.render_depth_maps(ft, db, train_ids)
        cloud = geometry.fuse_points(maps['depth'], maps['imgs'], maps['poses'], maps['Ks'], tau_d=tau_d)
        m = int(cloud['points'].shape[0])
        rec = {'points': m, 'radius': radius, 'surface_mean': None, 'surface_median': None, 'completeness': 0.0}
        if m:
            dist = geometry.surface_distance(db.scene, cloud['points'])
            rec.update(surface_mean=float(dist.mean()), surface_median=float(np.median(dist)),
                       completeness=float(within_radius(cloud['points'].to(dev), truth, radius).float().mean()))
        res[tag] = rec
    return res


def train(args, dev):
    db = database.parse_database_name(args.scene)
    train_ids, val_ids = database.get_database_split(db, 'val_all')
    t0 = time.perf_counter()
    scene = {'ref_imgs_info': pipeline.build_imgs_info(db, train_ids), 'val_imgs_info': pipeline.build_imgs_info(db, val_ids), 'database': db}
    t_data = time.perf_counter() - t0
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    from neuray_amd.network.renderer import NeuralRayFtRenderer
    cfg = {'use_hierarchical_sampling': True, 'use_self_hit_prob': True, 'render_depth': True, 'use_validation': True,
           'ray_feats_res': [db.h // 4, db.w // 4], 'train_ray_num': args.rays}
    ft = NeuralRayFtRenderer(cfg, scene=scene).train().to(dev)
    opt = torch.optim.Adam(ft.parameters(), lr=args.lr)
    losses = [name2loss['render']({'use_nr_fine_loss': True}), name2loss['consist']({})]
    curve = []
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for step in range(args.steps):
        opt.zero_grad(set_to_none=True)
        out = ft({})
        loss, log = total_loss(losses, out, {}, step)
        loss.backward()
        opt.step()
        if step % max(args.steps // 10, 1) == 0 or step == args.steps - 1:
            curve.append((step, float(log['loss_rgb_nr_fine'].mean())))
    torch.cuda.synchronize(dev)
    t_train = time.perf_counter() - t0
    res = {'scene': args.scene, 'rendered_on': db.rendered_on, 'views_train': len(train_ids), 'views_test': len(val_ids), 'steps': args.steps,
           'rays_per_step': args.rays, 'lr': args.lr, 'data_s': t_data, 'train_s': t_train, 'ms_per_step': 1e3 * t_train / max(args.steps, 1),
           'loss_rgb_nr_fine': curve, 'modes': evaluate(ft, db, val_ids, dev),
           'what': 'one procedurally generated scene, every network trained from scratch for minutes: not the paper\'s checkpoints'}
    if args.export_points:
        res['export_points'] = export_points(ft, db, train_ids, val_ids, dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--time', action='store_true')
    ap.add_argument('--scene', default='procedural/0/white_800')
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--rays', type=int, default=512)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--augment', action='store_true', help='--time: also the augmented stream (the three augmentation entries per batch)')
    ap.add_argument('--export-points', action='store_true', help='fuse the rendered depth of the training views in each render mode')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    if args.time:
        res = kernel_times(dev)
        if args.augment:
            res.update(augment_times(dev))
        res.update(gen_step_times(dev, augment=args.augment))
    else:
        res = train(args, dev)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
