"""Golden gradients of direct rendering (cfg use_dr_loss / use_dr_fine_loss, network/loss.py:70-76) from the REFERENCE's autograd.

Run in the build container only (needs /root/reference, read-only):

    python tests/golden/make_golden_dr_grads.py

Writes tests/golden/case_dr_grads.npz.  Scene: the cameras of case f_dr (make_golden.py direct_rendering_cases: a camera with
samples behind it, one far away, a wide depth range - masked views and points no view sees reach the `ground` / `insufficient`
branches), 48 x 48 pixels.
Each pass is NeuralRayBaseRenderer.render_by_depth (renderer.py:168-203) on stored depths - the coarse pass on sample_depth's
depths, the fine pass on the reference's own deterministic fine samples - so no chained resampling is involved.  Loss:
sum(lw * pixel_colors_dr) + sum(lw * hit_prob_dr) over both passes; stored: outputs, loss and the gradient of every dist_decoder.* /
fine_dist_decoder.* parameter and of ref.ray_feats, in fp32 and (the same step on the float64 renderer) in float64, for the coarse
decoder with use_vis False ('novis.*') and True ('vis.*').

Size.  The scene is not stored: scene() rebuilds it from its seed (the test does the same and checks 'scene_sha256').  A float64
gradient is stored as its difference from the fp32 one, divided by that difference's largest magnitude and rounded to fp16
('grad64d.*' + 'grad64s.*'): grad64 = grad + grad64s * grad64d, within 2.5e-4 x max |grad64 - grad| - the quantity the float64 check
compares against - instead of 8 bytes per element."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import hashlib  # noqa: E402

import ref_harness  # noqa: E402
from make_golden import build_renderer, coords_for_case, hot_weights  # noqa: E402
from oracle import neuray_oracle as orc  # noqa: E402

RN, DN, FDN, RFN, H, W = 24, 16, 16, 5, 48, 48


def tweak(que, ref):
    ref['poses'][1] = orc.look_at_pose(orc.sphere_pos(2.5, 30.0, 25.0), target=orc.sphere_pos(8.0, 30.0, 25.0))
    ref['poses'][2] = orc.look_at_pose(orc.sphere_pos(9.0, 200.0, -40.0))
    ref['depth_range'][2] = np.array([5.0, 13.0], np.float32)


def scene():
    """-> (que, ref, rng): the f_dr geometry, RN query rays; rng continues with the loss weights"""
    que, ref = orc.make_scene(H, W, RFN, seed=6, depth_range=(0.8, 9.0))
    tweak(que, ref)
    rng = np.random.RandomState(1006)
    que['coords'] = (rng.rand(1, RN, 2) * np.array([W - 1, H - 1])).astype(np.float32)        # make_golden.coords_for_case
    return que, ref, rng


def scene_sha256(que, ref):
    h = hashlib.sha256()
    for pre, d in (('que.', que), ('ref.', ref)):
        for k in sorted(d):
            a = np.ascontiguousarray(d[k])
            h.update((pre + k + str(a.dtype) + str(a.shape)).encode())
            h.update(a.tobytes())
    return h.hexdigest()


def cfg_for(use_vis):
    return {'use_hierarchical_sampling': True, 'dist_decoder_cfg': {'use_vis': use_vis}, 'depth_sample_num': DN,
            'fine_depth_sample_num': FDN, 'agg_net_cfg': {'sample_num': DN}, 'fine_agg_net_cfg': {'sample_num': FDN},
            'use_dr_prediction': True, 'use_dr_loss': True, 'use_dr_fine_loss': True, 'use_self_hit_prob': False}


def one_step(ns, renderer, que, ref, depths, lw, dtype):
    r = renderer.to(dtype)
    tq = {k: torch.from_numpy(v).to(dtype) for k, v in que.items()}
    tr = {k: torch.from_numpy(v).to(dtype) for k, v in ref.items()}
    tr['ray_feats'].requires_grad_(True)
    r.zero_grad()
    loss, outs = 0.0, {}
    for is_fine, depth in enumerate(depths):
        out = r.render_by_depth(torch.from_numpy(depth).to(dtype), tq, tr, True, bool(is_fine))
        sfx = '_fine' if is_fine else ''
        for k in ('pixel_colors_dr', 'hit_prob_dr'):
            outs[k + sfx] = out[k]
            loss = loss + (torch.from_numpy(lw[k + sfx]).to(dtype) * out[k]).sum()
    loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy()
             for k, p in r.named_parameters() if k.startswith(('dist_decoder.', 'fine_dist_decoder.'))}
    grads['ref.ray_feats'] = tr['ray_feats'].grad.detach().numpy().copy()
    return float(loss.detach()), {k: v.detach().numpy().copy() for k, v in outs.items()}, grads


def main():
    ns = ref_harness.import_reference()
    que, ref, rng = scene()
    check = np.random.RandomState(1006)
    assert np.array_equal(que['coords'], coords_for_case(check, H, W, RN, False))
    save = {'scene_sha256': np.array(scene_sha256(que, ref))}
    ro = ns.render_ops
    lw = {k: rng.randn(*shape).astype(np.float32) for k, shape in
          (('pixel_colors_dr', (1, RN, 3)), ('hit_prob_dr', (1, RN, DN)), ('pixel_colors_dr_fine', (1, RN, 3)),
           ('hit_prob_dr_fine', (1, RN, FDN)))}
    for k, v in lw.items():
        save['lw.' + k] = v
    for tag, use_vis in (('novis', False), ('vis', True)):
        cfg = cfg_for(use_vis)
        renderer = build_renderer(ns, cfg, seed=0)
        renderer.train()
        tq = {k: torch.from_numpy(v) for k, v in que.items()}
        tr = {k: torch.from_numpy(v) for k, v in ref.items()}
        with torch.no_grad():           # depths: sample_depth, and the reference's deterministic fine samples on the coarse pass
            coarse, _ = ro.sample_depth(tq['depth_range'], tq['coords'], DN, False)
            cout = renderer.render_by_depth(coarse, tq, tr, False, False)
            fine = ro.sample_fine_depth(coarse, cout['hit_prob_nr'], tq['depth_range'], FDN, False)
            fine = torch.sort(fine, -1)[0]
        depths = (coarse.numpy().astype(np.float32), fine.numpy().astype(np.float32))
        save[tag + '.cfg_json'] = np.array(repr(cfg))
        save[tag + '.depth'], save[tag + '.depth_fine'] = depths
        # the renderer's weights are those of tests/golden/weights_seed0[_vis].npz (conftest.load_weights): not stored again
        stored = np.load(os.path.join(HERE, 'weights_seed0_vis.npz' if use_vis else 'weights_seed0.npz'))
        hot = hot_weights(renderer)
        assert sorted(hot) == sorted(stored.files) and all(np.array_equal(hot[k], stored[k]) for k in hot)
        loss, outs, grads = one_step(ns, renderer, que, ref, depths, lw, torch.float32)
        loss64, _, grads64 = one_step(ns, renderer, que, ref, depths, lw, torch.float64)
        save[tag + '.loss'], save[tag + '.loss64'] = np.array(loss), np.array(loss64)
        for k, v in outs.items():
            save['%s.out.%s' % (tag, k)] = v
        for k, v in grads.items():
            save['%s.grad.%s' % (tag, k)] = v
            diff = grads64[k] - v.astype(np.float64)
            scale = float(np.abs(diff).max())
            save['%s.grad64s.%s' % (tag, k)] = np.array(scale)
            save['%s.grad64d.%s' % (tag, k)] = (diff / scale if scale > 0 else diff).astype(np.float16)
            back = v.astype(np.float64) + scale * save['%s.grad64d.%s' % (tag, k)].astype(np.float64)
            assert np.abs(back - grads64[k]).max() <= 2.5e-4 * scale
        print(tag, 'loss', save[tag + '.loss'], 'loss64', save[tag + '.loss64'])
    path = os.path.join(HERE, 'case_dr_grads.npz')
    np.savez_compressed(path, **save)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
