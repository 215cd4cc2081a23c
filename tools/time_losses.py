"""Time a loss call of neuray_amd.loss (csrc/nr_kernels_loss.h, neuray_train_loss[_backward]) on the GPU against an eager PyTorch
composition of the same formulas on the same GPU in the same process (tests/loss_cases.py in float32, with F.grid_sample for the
depth gather as network/loss.py does it).  The reference's own module does not exist on the GPU box; the composition restates it.
  ft    config-4 call: RenderLoss (nr + nr_fine, ray mask) + ConsistencyLoss (coarse + fine), 512 rays, 64 + 64 samples; forward + backward
  gen   config-5 call: RenderLoss (nr + nr_fine) + DepthLoss (coarse + fine, gso), 8 views, 8192 int64 coordinates, 416 x 608 maps,
        depth_mean a strided view; forward + backward
  val   the validation call: RenderLoss (four terms) on 640 000 rays under no_grad; forward only
HIP events around `reps` calls each (alternating ours / eager), median and minimum per call.
    python tools/time_losses.py [--reps 20]
    python tools/time_losses.py --once        # one call of each shape and side, no timing: for `rocprofv3 --kernel-trace --stats`
Kernel names: nr::loss_partials_kernel, nr::loss_finish_kernel, nr::loss_backward_kernel."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import loss_cases as lc                                           # noqa: E402
from neuray_amd import loss as nloss                              # noqa: E402
from neuray_amd.engine import RenderEngine                        # noqa: E402


def shapes(dev, eng):
    """-> {name: (ours, eager, leaves, train)}: closures that return the step's total loss"""
    out = {}
    cfg = {'use_nr_fine_loss': True}
    # ft
    rc = lc.render_inputs(1, 1, 512, suffixes=('nr', 'nr_fine'))
    cc = lc.consist_inputs(2, 1, 512, 64)
    leaves = {k: lc.as_torch(v, device=dev).requires_grad_(True) for k, v in {**rc, **cc}.items()
              if k.startswith('pixel_colors_n') or k.startswith('hit_prob_')}
    data = {**leaves, 'pixel_colors_gt': lc.as_torch(rc['pixel_colors_gt'], device=dev), 'ray_mask': lc.as_torch(rc['ray_mask'], device=dev)}
    losses = [nloss.RenderLoss(cfg, engine=eng), nloss.ConsistencyLoss(cfg, engine=eng)]

    def ft_eager():
        vals = lc.render_terms([data['pixel_colors_nr'], data['pixel_colors_nr_fine']], data['pixel_colors_gt'], data['ray_mask'])
        vals += lc.consist_terms([(data['hit_prob_nr'], data['hit_prob_self']), (data['hit_prob_nr_fine'], data['hit_prob_self_fine'])])
        return sum(torch.mean(v) for v in vals)
    out['ft'] = (lambda: nloss.total_loss(losses, data, {}, 0)[0], ft_eager, [v for k, v in leaves.items() if 'hit_prob_nr' not in k], True)
    # gen
    dc = lc.depth_inputs(3, 8, 8192, 416, 608, True, True)
    data_pr, data_gt, dleaves = lc.depth_data(dc, torch.float32, dev)
    rleaves = {k: lc.as_torch(rc[k], device=dev).requires_grad_(True) for k in ('pixel_colors_nr', 'pixel_colors_nr_fine')}
    gdata = {**data_pr, **rleaves, 'pixel_colors_gt': data['pixel_colors_gt'], 'ray_mask': data['ray_mask']}
    glosses = [nloss.RenderLoss(cfg, engine=eng), nloss.DepthLoss({}, engine=eng)]
    info = data_gt['ref_imgs_info']

    def gen_eager():
        vals = lc.render_terms([gdata['pixel_colors_nr'], gdata['pixel_colors_nr_fine']], gdata['pixel_colors_gt'], gdata['ray_mask'])
        vals += lc.depth_terms([gdata['depth_mean'], gdata['depth_mean_fine']], info['true_depth'], info['depth'], gdata['depth_coords'],
                               info['depth_range'], use_grid_sample=True)
        return sum(torch.mean(v) for v in vals)
    out['gen'] = (lambda: nloss.total_loss(glosses, gdata, data_gt, 0)[0], gen_eager, list(rleaves.values()) + list(dleaves.values()), True)
    # val
    vc = lc.render_inputs(4, 1, 640000)
    vdata = {k: lc.as_torch(v, device=dev) for k, v in vc.items()}
    vloss = nloss.RenderLoss({'use_dr_loss': True, 'use_dr_fine_loss': True, 'use_nr_fine_loss': True}, engine=eng)

    def val_eager():
        vals = lc.render_terms([vdata['pixel_colors_' + s] for s in ('nr', 'dr', 'dr_fine', 'nr_fine')], vdata['pixel_colors_gt'], vdata['ray_mask'])
        return sum(torch.mean(v) for v in vals)
    out['val'] = (lambda: nloss.total_loss([vloss], vdata, {}, 0)[0], val_eager, [], False)
    return out


def one_call(fn, leaves, train):
    if train:
        for v in leaves:
            v.grad = None
        fn().backward()
    else:
        with torch.no_grad():
            fn()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    eng = RenderEngine(dev)
    out = {}
    for name, (ours, eager, leaves, train) in shapes(dev, eng).items():
        if args.once:
            one_call(ours, leaves, train)
            torch.cuda.synchronize()
            one_call(eager, leaves, train)
            torch.cuda.synchronize()
            continue
        with torch.no_grad():
            a, b = float(ours()), float(eager())
        for fn in (ours, eager):                       # warm-up
            for _ in range(3):
                one_call(fn, leaves, train)
        torch.cuda.synchronize()
        ts = {'ours': [], 'eager': []}
        for _ in range(args.reps):
            for side, fn in (('ours', ours), ('eager', eager)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); one_call(fn, leaves, train); e1.record(); torch.cuda.synchronize()
                ts[side].append(e0.elapsed_time(e1))
        out[name] = {'passes': 'forward + backward' if train else 'forward', 'loss_ours': a, 'loss_eager': b,
                     'ours_ms_median': round(float(np.median(ts['ours'])), 4), 'ours_ms_min': round(min(ts['ours']), 4),
                     'eager_ms_median': round(float(np.median(ts['eager'])), 4), 'eager_ms_min': round(min(ts['eager']), 4)}
    if not args.once:
        print(json.dumps(out))


if __name__ == '__main__':
    main()
