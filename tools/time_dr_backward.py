"""Time training through direct rendering (cfg use_dr_loss / use_dr_fine_loss) per pass at the config-4 training shape - 600 x 800
images, 512 rays, 64 + 64 samples, 8 reference views - next to the pass's own per-ray training step (HIP events):
  dr    = autograd.DirectRenderFn forward (the point kernel once more for its per-view record, the dr kernels) + its backward (the two
          dr backward kernels, the decoder rows' re-gather, dist_decoder_rows_backward, interpolate_feats_backward)
  nr    = autograd.RenderPassFn forward + backward (the existing training pass: point / ray kernels and their backward kernels)
    python tools/time_dr_backward.py [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuray_amd import synthetic                                   # noqa: E402
from neuray_amd.network.autograd import DirectRenderFn, PassRun, RenderPassFn      # noqa: E402
from neuray_amd.network.renderer import NeuralRayBaseRenderer      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rays', type=int, default=512)
    ap.add_argument('--hw', type=int, nargs=2, default=[600, 800])
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    cfg = {'use_hierarchical_sampling': True, 'dist_decoder_cfg': {'use_vis': False}, 'use_dr_prediction': True, 'use_dr_loss': True,
           'use_dr_fine_loss': True}
    r = NeuralRayBaseRenderer(cfg).to(dev).train()
    que, ref = synthetic.make_scene(args.hw[0], args.hw[1], 8, seed=0)
    rng = np.random.RandomState(0)
    t = lambda a: torch.from_numpy(a).to(dev)                      # noqa: E731
    tq, tr = {k: t(v) for k, v in que.items() if k != 'Ks_inv'}, {k: t(v) for k, v in ref.items()}
    tr['ray_feats'].requires_grad_(True)
    tr['img_feats'].requires_grad_(True)
    coords = t((rng.rand(args.rays, 2) * np.array([args.hw[1] - 1, args.hw[0] - 1])).astype(np.float32))
    eng = r.engine(dev)
    views, qc = r._views(eng, tr), r._query(eng, tq)
    coarse = eng.sample_coarse_depth(tq['depth_range'], args.rays, 64)
    regs = torch.tensor([0.0] + [0.001] * 3 + [0.005] * 5 + [0.05] * 7, device=dev)      # SphericalHarmonicsSolver(3).regs (sph_solver.py:6-12)
    out = {'rays': args.rays, 'hw': args.hw, 'views': 8}
    for name, is_fine in (('coarse', False), ('fine', True)):
        dist = r.fine_dist_decoder if is_fine else r.dist_decoder
        agg = r.fine_agg_net if is_fine else r.agg_net
        depth = coarse
        if is_fine:                                                     # fine samples on the coarse pass's hit probabilities
            with torch.no_grad():
                hit = eng.render_pass(qc, views, coords, coarse, r._packed_pass(eng, False), use_vis=False)['hit_prob']
            depth = eng.sample_fine_depth(qc, coarse, hit, 64, use_all=True)
        run = PassRun(eng, qc, views, coords, depth.contiguous(), dist, agg, False, dist.cfg['bias_val'], 2, 8, False)
        dparams = [p for _, p in run.dist_params()]
        rn, dn = depth.shape

        def dr_step():
            pix, hitp = DirectRenderFn.apply(run, regs, -15.0, tr['ray_feats'], *dparams)
            torch.autograd.backward([pix, hitp], [torch.ones_like(pix), torch.ones_like(hitp)])

        def nr_step():
            pix, hitp, _, rd = RenderPassFn.apply(run, tr['ray_feats'], tr['img_feats'], *[p for _, p in run.named_params()])
            torch.autograd.backward([pix, hitp], [torch.ones_like(pix), torch.ones_like(hitp)])

        for label, fn in (('dr', dr_step), ('nr', nr_step)):
            fn(); fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            out['%s_%s_ms_median' % (name, label)] = round(float(np.median(ts)), 3)
            out['%s_%s_ms_min' % (name, label)] = round(min(ts), 3)
        out['%s_samples' % name] = dn
        # the dr kernels alone: the two forward kernels (direct_render) and each backward kernel, on the same record
        with torch.no_grad():
            flat, packed, has_vis = run.device_weights()
            rec = eng.render_pass(qc, views, coords, run.depth, packed, use_vis=False, want_dbg=True)['dbg']
            dr = eng.direct_render(qc, views, coords, run.depth, rec, regs)
            gp, gh = torch.ones(rn, 3, device=dev), torch.ones(rn, dn, device=dev)
            for label, fn in (('dr_fwd_kernels', lambda: eng.direct_render(qc, views, coords, run.depth, rec, regs)),
                              ('dr_rays_bwd', lambda: eng.direct_render_rays_backward(dr['alpha'], dr['colors'], gp, gh)),
                              ('dr_points_bwd', lambda: eng.direct_render_points_backward(qc, views, coords, run.depth, rec, regs,
                                                                                         dr['alpha'], dr['colors'], False))):
                fn(); torch.cuda.synchronize()
                ts = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                out['%s_%s_ms_median' % (name, label)] = round(float(np.median(ts)), 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
