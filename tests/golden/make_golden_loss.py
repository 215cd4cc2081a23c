"""Writes tests/golden/case_loss.npz: the reference's own network/loss.py (imported through ref_harness.py; build container only)
on the seeded inputs of tests/loss_cases.py, evaluated twice - in float32 as shipped and with every floating input in float64
(coordinates too: with int64 coordinates interpolate_feats builds a float32 grid and grid_sample refuses the float64 map).

Per case and key:   val.<case>.<key>    float64 loss values
                    grad.<case>.<leaf>  float64 autograd gradient of sum_k mean(v_k) with respect to every prediction
                    dev32v.<case>.<key>, dev32g.<case>.<leaf>  max |float32 result - float64 result|: the reference's own float32 error
                    sha.<case>          sha256 of the inputs (the tests rebuild them from the seeds)

    python tests/golden/make_golden_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import loss_cases as lc  # noqa: E402
import ref_harness  # noqa: E402


def run(loss_obj, data_pr, data_gt, leaves):
    out = loss_obj(data_pr, data_gt, 0)
    total = sum(torch.mean(v) for v in out.values())
    grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    return ({k: v.detach().double().numpy() for k, v in out.items()},
            {k: (g.detach().double().numpy() if g is not None else None) for k, g in zip(leaves, grads)})


def record(store, name, r32, r64, sha):
    (v32, g32), (v64, g64) = r32, r64
    assert list(v32) == list(v64)
    for k in v64:
        store['val.%s.%s' % (name, k)] = v64[k]
        store['dev32v.%s.%s' % (name, k)] = np.float64(np.abs(v32[k] - v64[k]).max())
    for k in g64:
        if g64[k] is None:
            assert g32[k] is None
            continue
        store['grad.%s.%s' % (name, k)] = g64[k]
        store['dev32g.%s.%s' % (name, k)] = np.float64(np.abs(g32[k] - g64[k]).max())
    store['sha.' + name] = np.array(sha)


def main():
    ref_harness.import_reference()
    import network.loss as ref
    from network.ops import interpolate_feats
    store = {}
    full = {'use_dr_loss': True, 'use_dr_fine_loss': True, 'use_nr_fine_loss': True}
    for name, kw in lc.RENDER_CASES.items():
        case = lc.render_inputs(**kw)
        res = []
        for dtype in (torch.float32, torch.float64):
            leaves = {k: lc.as_torch(v, dtype).requires_grad_(True) for k, v in case.items() if k.startswith('pixel_colors_') and k != 'pixel_colors_gt'}
            data_pr = {**leaves, 'pixel_colors_gt': lc.as_torch(case['pixel_colors_gt'], dtype), 'ray_mask': lc.as_torch(case['ray_mask'])}
            res.append(run(ref.RenderLoss({**full, 'use_ray_mask': name == 'render_mask'}), data_pr, {}, leaves))
        record(store, name, res[0], res[1], lc.digest(case))
    for name, kw in lc.CONSIST_CASES.items():
        case = lc.consist_inputs(**kw)
        res = []
        for dtype in (torch.float32, torch.float64):
            leaves = {k: lc.as_torch(v, dtype).requires_grad_(True) for k, v in case.items() if k.startswith('hit_prob_')}
            data_pr = {**leaves, 'ray_mask': lc.as_torch(case['ray_mask'])}
            res.append(run(ref.ConsistencyLoss({}), data_pr, {}, leaves))
        assert res[1][1]['hit_prob_nr'] is None and res[1][1]['hit_prob_nr_fine'] is None       # p0 is detached
        record(store, name, res[0], res[1], lc.digest(case))
    for name, kw in lc.DEPTH_CASES.items():
        case = lc.depth_inputs(**kw)
        res, masks = [], []
        for dtype in (torch.float32, torch.float64):
            data_pr, data_gt, leaves = lc.depth_data(case, dtype, float_coords=dtype == torch.float64)
            loss = ref.DepthLoss({'depth_loss_type': lc.DEPTH_CFG[name]})
            res.append(run(loss, data_pr, data_gt, leaves))
            if kw['gso']:                            # the reference's own mask (loss.py:98-99, 104-110, 120-123), for the flip check
                info = data_gt['ref_imgs_info']
                h, w = info['true_depth'].shape[2:]
                near, far = -1 / info['depth_range'][:, 0:1], -1 / info['depth_range'][:, 1:2]
                proc = lambda m: torch.clamp((-1 / torch.clamp(interpolate_feats(                # noqa: E731
                    m, data_pr['depth_coords'], h, w, padding_mode='border', align_corners=True)[..., 0], min=1e-5) - near) / (far - near), min=0, max=1.0)
                masks.append((torch.abs(proc(info['depth']) - proc(info['true_depth'])) < loss.cfg['depth_correct_thresh']).numpy())
        if kw['gso']:
            assert (masks[0] == masks[1]).all(), '%s: %d mask flips between float32 and float64' % (name, (masks[0] != masks[1]).sum())
            print('%s: mask agrees on all %d points, %.1f %% masked in' % (name, masks[0].size, 100 * masks[0].mean()))
        record(store, name, res[0], res[1], lc.digest(case))
    # without true_depth: zeros([1]), float32, on the predictions' device
    out = ref.DepthLoss({})({'pixel_colors_nr': torch.zeros(1, 4, 3)}, {'ref_imgs_info': {}}, 0)
    store['val.depth_none.loss_depth'] = out['loss_depth'].double().numpy()
    path = os.path.join(HERE, 'case_loss.npz')
    np.savez_compressed(path, **store)
    for k in sorted(store):
        if k.startswith('dev32'):
            ref_key = k.replace('dev32v', 'val').replace('dev32g', 'grad')
            print('%-48s %.3e  (max |ref64| %.3e)' % (k, store[k], np.abs(store[ref_key]).max()))
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
