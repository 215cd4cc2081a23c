"""What cfg['hip_deterministic'] costs: the backward kernels and the training steps with the mode off (the atomic path,
the baseline) and on, in one process - 3 warm-up steps, the median of 20 by HIP events - and the mode's extra device memory.  Then
whether a WHOLE NeuralRayFtRenderer.train_step + backward (encoders, MIOpen and PyTorch kernels included) repeats bitwise with the mode
on plus torch.use_deterministic_algorithms(True, warn_only=True) and torch.backends.cudnn.deterministic = True: recorded, not gated.

    python tools/bench_deterministic.py [--reps 20] [--no-ft]        -> one JSON line"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuray_amd import synthetic                                   # noqa: E402
from neuray_amd.engine import RenderEngine                         # noqa: E402
from neuray_amd.network import fused_norm                          # noqa: E402
from neuray_amd.network.renderer import NeuralRayBaseRenderer      # noqa: E402

WARMUP = 3


def median_ms(fn, reps):
    for _ in range(WARMUP):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def off_on(make, reps):
    """make(mode) -> (step function, engine) -> {'off_ms', 'on_ms', 'extra_bytes': scratch the mode allocates per step}"""
    res = {}
    for mode in (False, True):
        fn, eng = make(mode)
        res['on_ms' if mode else 'off_ms'] = median_ms(fn, reps)
        before = eng.det_scratch_bytes
        fn()
        if mode:
            res['extra_bytes'] = eng.det_scratch_bytes - before
        else:
            assert eng.det_scratch_bytes == before == 0
    return res


def kernels(dev, reps):
    """the point backward alone (as tools/time_bwd.py) and the ray backward: 512 rays x 64 samples x 8 views, 400 x 600"""
    torch.manual_seed(0)
    r = NeuralRayBaseRenderer({'use_hierarchical_sampling': False, 'dist_decoder_cfg': {'use_vis': False}})
    eng = RenderEngine(dev)
    que, ref = synthetic.make_scene(400, 600, 8, seed=0)
    coords = torch.from_numpy((np.random.RandomState(0).rand(512, 2) * np.array([599, 399])).astype(np.float32)).to(dev)
    t = lambda a: torch.from_numpy(a).to(dev)                      # noqa: E731
    views, qc = eng.prepare_views({k: t(v) for k, v in ref.items()}), eng.prepare_query({k: t(v) for k, v in que.items()})
    depth = eng.sample_coarse_depth(t(que['depth_range']), 512, 64)
    flat, has_vis = eng.flat_pass(dict(r.state_dict()), 'dist_decoder.', 'agg_net.')
    packed = eng.pack_pass_device(flat, has_vis)
    fwd = eng.render_pass(qc, views, coords, depth, packed, use_vis=False, save=True)
    d_rec = torch.randn(512, 64, 20, device=dev) * 1e-2
    d_pix, d_hit = torch.randn(512, 3, device=dev), torch.randn(512, 64, device=dev)
    points = lambda mode: (lambda: eng.render_points_backward(qc, views, coords, depth, flat, has_vis, False, d_rec, packed=packed,      # noqa: E731
                                                              saved=fwd['saved'], deterministic=mode), eng)
    rays = lambda mode: (lambda: eng.render_rays_backward(fwd['point_rec'], depth, packed, d_pix, d_hit, att_saved=fwd['att_saved'],        # noqa: E731
                                                          deterministic=mode), eng)
    return {'point_backward': off_on(points, reps), 'ray_backward': off_on(rays, reps)}


def train_step(dev, reps):
    """the 512-ray step of tools/bench_train.py: render_impl(is_train=True) + backward, 8 views of 400 x 600, 64 + 64 samples"""
    que, ref = synthetic.make_scene(400, 600, 8, seed=0, que_imgs=True)
    que['coords'] = (np.random.RandomState(0).rand(1, 512, 2) * np.array([599, 399])).astype(np.float32)
    tq = {k: torch.from_numpy(v).to(dev) for k, v in que.items()}
    tr = {k: torch.from_numpy(v).to(dev) for k, v in ref.items()}
    for x in (tr['ray_feats'], tr['img_feats'], tq['ray_feats']):
        x.requires_grad_(True)
    tgt = torch.rand(1, 512, 3, device=dev)

    def make(mode):
        torch.manual_seed(0)
        r = NeuralRayBaseRenderer({'use_hierarchical_sampling': True, 'dist_decoder_cfg': {'use_vis': False}, 'depth_sample_num': 64,
                                   'fine_depth_sample_num': 64, 'agg_net_cfg': {'sample_num': 64}, 'fine_agg_net_cfg': {'sample_num': 64},
                                   'use_self_hit_prob': True, 'hip_deterministic': mode}).train().to(dev)

        def step():
            r.zero_grad(set_to_none=True)
            out = r.render_impl(tq, tr, True)
            (((out['pixel_colors_nr'] - tgt) ** 2).mean() + ((out['pixel_colors_nr_fine'] - tgt) ** 2).mean() +
             out['hit_prob_self'].mean() + out['hit_prob_self_fine'].mean()).backward()
        return step, r.engine(dev)
    return off_on(make, reps)


def _ft(dev, mode):
    from neuray_amd import pipeline
    from neuray_amd.network.renderer import NeuralRayFtRenderer
    db = synthetic.MemoryDatabase(24, 800, 800, seed=0)
    scene = {'ref_imgs_info': pipeline.build_imgs_info(db, db.get_img_ids(), -1, True, False, True, True)}
    torch.manual_seed(0)
    ft = NeuralRayFtRenderer({'use_hierarchical_sampling': True, 'dist_decoder_cfg': {'use_vis': False}, 'use_self_hit_prob': True,
                              'use_validation': False, 'train_ray_num': 512, 'hip_deterministic': mode}, scene=scene).train().to(dev)

    def grads():
        ft.zero_grad(set_to_none=True)
        out = ft.train_step()
        (((out['pixel_colors_nr'] - out['pixel_colors_gt']) ** 2).mean() + ((out['pixel_colors_nr_fine'] - out['pixel_colors_gt']) ** 2).mean() +
         out['hit_prob_self'].mean() + out['hit_prob_self_fine'].mean()).backward()
    return ft, grads


def ft_step(dev, reps):
    """the --ft step of tools/bench_train.py: NeuralRayFtRenderer.train_step + backward + Adam on a 24-view 800 x 800 in-memory scene"""
    def make(mode):
        ft, grads = _ft(dev, mode)
        opt = torch.optim.Adam(ft.parameters(), lr=1e-4)

        def step():
            grads()
            opt.step()
        return step, ft.engine(dev)
    return off_on(make, reps)


def whole_step_repeats(dev):
    """three times the same train_step + backward (same seeds, no optimiser step) with the mode on and PyTorch's own switches set:
    are ALL parameter gradients bitwise equal?  Which ops did PyTorch flag as non-deterministic?"""
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.backends.cudnn.deterministic = True
    flagged = set()
    try:
        ft, grads = _ft(dev, True)
        runs = []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            for _ in range(3):
                np.random.seed(7)
                torch.manual_seed(7)
                grads()
                runs.append({k: p.grad.detach().clone() for k, p in ft.named_parameters() if p.grad is not None})
        for w in caught:
            msg = str(w.message)
            if 'deterministic' in msg:
                flagged.add(msg.split(' does not have')[0].split(' is ')[0][:120])
        differ = sorted({k for other in runs[1:] for k in runs[0] if not torch.equal(runs[0][k], other[k])})
        ours = [k for k in differ if k.startswith(('dist_decoder.', 'agg_net.', 'fine_dist_decoder.', 'fine_agg_net.'))]
        return {'gradients': len(runs[0]), 'differ': len(differ), 'differ_in_render_weights': len(ours), 'first_differing': differ[:6],
                'flagged_ops': sorted(flagged)}
    finally:
        torch.use_deterministic_algorithms(False)
        torch.backends.cudnn.deterministic = False
        fused_norm.DETERMINISTIC = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-ft', action='store_true', help='skip the NeuralRayFtRenderer legs (an 800 x 800 scene of 24 views)')
    args = ap.parse_args()
    os.environ.pop('NEURAY_HIP_DETERMINISTIC', None)                 # the tool sets the mode itself
    dev = torch.device('cuda', 0)
    res = {'what': "cfg['hip_deterministic'] off / on, median of %d by HIP events after %d warm-up steps, ms" % (args.reps, WARMUP)}
    res.update(kernels(dev, args.reps))
    res['train_step_512'] = train_step(dev, args.reps)
    if not args.no_ft:
        res['ft_step_512'] = ft_step(dev, args.reps)
        res['whole_ft_step_bitwise'] = whole_step_repeats(dev)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
