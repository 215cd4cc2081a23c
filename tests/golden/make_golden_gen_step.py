"""One generalisation training step at BASELINE config 5's structure (configs/train/gen/neuray_gen_cost_volume_train.yaml), produced by
running the REFERENCE ITSELF (CPU, read-only reference tree, imported through ref_harness.py):

    python tests/golden/make_golden_gen_step.py            (build container only; about two minutes)

`NeuralRayGenRenderer` with `CostVolumeInitNet`, both encoders, render + depth loss (the reference's own network/loss.py, summed as
train/trainer.py:124-132 sums them), `loss.backward()`.  Every case runs twice: in float32, and with the trainable part in FLOAT64
(`model.double()`, every float input cast up).  The frozen MVSNet runs once in float32 under no_grad (`construct_project_matrix`
hard-codes float32); its `cost_reg` and `depth` are handed to both runs - and, stored, to the tests - through a patched
`init_net.construct_cost_volume_with_src`.

Written to tests/golden/case_c5_gen_step_{a,b}.npz: the case's arguments, the fp32 `cost_reg` / `depth`, the float64 run's loss terms and
outputs (as float32), a gradient record of every trainable parameter (grad_record below: small tensors whole, large ones as row sums, 512
sampled entries and max |g|), and per top-level module the reference's OWN error `r_m` = float32 run against float64 run under
module_errors - the yardstick of tests/test_gen_train_step.py.

  a   64 x 96, 3 working views + 2 further source views, 48 rays in one ray batch
  b   96 x 64 (portrait), 8 working views (the config's count) + 3, 80 rays at ray_batch_num 32: three render_impl calls, the last partial

The scene (neuray_amd/synthetic.py, pure numpy) is regenerated at test time from the stored arguments, not stored.

The seeds.  The step is not differentiable everywhere: every ReLU (the encoders', the init net's, prob_embed's and IBRNet's in the per-ray
networks) has a kink, and a unit whose pre-activation lies within float32 rounding of zero takes one branch in one float32 evaluation and
the other in the next - each such unit changes the gradients by its whole contribution (g_out * input: 1e-4 ... 1e-2 of a tensor), which
no multiple of a rounding error covers.  The reference's own float32 run differs from its float64 run in 0 - 4 of the 1.4 M (case a) /
3.9 M (case b) ReLU units, depending on the seed; with a flip its r_m is 1e-2, without 2e-5.  A float64 gradient is a yardstick for float32
code only where both sit on the same branches, so case a's seed is chosen FROM THE REFERENCE ALONE (scan of seeds 51, 60, 61, 68 - 70,
72 - 79, 100 - 105 with a forward of both precisions): among the seeds at which the reference's float32 run takes the float64 run's branch
in every unit, the one whose per-ray ReLU units (149 k: they are evaluated by the kernels under test from inputs that already differ by
1e-6) keep the widest distance from the kink in float64 - seed 72, min |x| = 1.95e-5 (seed 51, tried first: 1.8e-6, and both backends
took the other branch in two prob_embed units).  Case b's seeds are the first ones tried; there the reference's float32 run does flip
(r_m 2e-2 / 1e-1 in image_encoder / init_net), which the stored r_m records and the tests' cap of 5e-3 absorbs.

The top half of this file (CASES ... module_errors) is pure numpy and is imported by the tests; only main() needs the reference.
"""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p_ in (HERE, ROOT):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from neuray_amd import synthetic  # noqa: E402

CASES = {
    'a': {'h': 64, 'w': 96, 'rfn': 3, 'extra': 2, 'cost_volume_sn': 8, 'depth_sample_num': 16, 'fine_depth_sample_num': 16, 'rays': 48,
          'depth_loss_coords_num': 96, 'ray_batch_num': 2048, 'seed': 72, 'torch_seed': 73},
    'b': {'h': 96, 'w': 64, 'rfn': 8, 'extra': 3, 'cost_volume_sn': 8, 'depth_sample_num': 16, 'fine_depth_sample_num': 16, 'rays': 80,
          'depth_loss_coords_num': 96, 'ray_batch_num': 32, 'seed': 53, 'torch_seed': 54},
}
# the loss keys of config 5 (the trainer hands its whole cfg to every loss object)
LOSS_CFG = {'use_dr_loss': False, 'use_dr_fine_loss': False, 'use_nr_fine_loss': True}
LOSS_NAMES = ('render', 'depth')
WEIGHT_SCALE = 0.1           # fill_by_name's usual 0.25 blows this step up to a loss of 8.5e4
WHOLE_MAX = 2048             # gradient tensors of at most this many entries are stored whole
N_TOP, N_RANDOM = 256, 256   # sampled entries of the larger ones
FLOOR = 1e-3                 # of the module's largest value: the denominator's floor (tensors whose true gradient is zero)
OUTPUT_KEYS = ('pixel_colors_nr', 'pixel_colors_nr_fine', 'hit_prob_nr', 'hit_prob_nr_fine', 'depth_mean', 'depth_mean_2', 'depth_mean_fine',
               'depth_mean_fine_2', 'pixel_colors_gt')
EXACT_KEYS = ('depth_coords', 'ray_mask', 'ray_mask_fine')


def net_cfg(a):
    """the network cfg of config 5 at the case's sizes"""
    return {'init_net_type': 'cost_volume', 'init_net_cfg': {'cost_volume_sn': int(a['cost_volume_sn'])}, 'use_hierarchical_sampling': True,
            'use_depth_loss': True, 'dist_decoder_cfg': {'use_vis': False}, 'fine_dist_decoder_cfg': {'use_vis': False},
            'ray_batch_num': int(a['ray_batch_num']), 'depth_sample_num': int(a['depth_sample_num']),
            'fine_depth_sample_num': int(a['fine_depth_sample_num']), 'agg_net_cfg': {'sample_num': int(a['depth_sample_num'])},
            'fine_agg_net_cfg': {'sample_num': int(a['fine_depth_sample_num'])}, 'depth_loss_coords_num': int(a['depth_loss_coords_num'])}


def case_inputs(a):
    """-> (que, ref, src): numpy imgs_info dicts of one step, from the case's arguments alone"""
    h, w, rfn = int(a['h']), int(a['w']), int(a['rfn'])
    n = rfn + int(a['extra'])
    que, scene = synthetic.make_scene(h, w, n, seed=int(a['seed']), que_imgs=True, smooth=True)
    src = {k: np.ascontiguousarray(scene[k], np.float32) for k in ('imgs', 'poses', 'Ks', 'depth_range')}
    ref = {k: v[:rfn].copy() for k, v in src.items()}
    ref['nn_ids'] = np.array([[(v + 1) % n, (v + 2) % n, (v + 4) % n] for v in range(rfn)], np.int64)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    ref['true_depth'] = np.stack([3.6 + 0.7 * np.sin(xx / 9.0 + v) * np.cos(yy / 7.0 - v) for v in range(rfn)])[:, None].astype(np.float32)
    que = {k: np.ascontiguousarray(v, np.float32) for k, v in que.items() if k != 'ray_feats'}
    que['coords'] = (np.random.RandomState(int(a['seed'])).rand(1, int(a['rays']), 2) * np.array([w - 1, h - 1])).astype(np.float32)
    return que, ref, src


def module_of(name):
    return name.split('.')[0]


def sample_index(name, g64):
    """flat indices of a large tensor's sampled entries: the N_TOP largest-magnitude entries of the float64 gradient, then N_RANDOM entries
    at indices that depend on the tensor's name only"""
    flat = np.abs(np.asarray(g64).reshape(-1))
    top = np.argsort(-flat, kind='stable')[:N_TOP]
    rnd = np.random.RandomState(zlib.crc32(name.encode())).randint(0, flat.shape[0], N_RANDOM)
    return np.concatenate([top, rnd]).astype(np.int64)


def grad_record(grads, index):
    """grads: name -> array; index: name -> sample_index(...) of the tensors with more than WHOLE_MAX entries.
    -> name -> {kind: float64 array}; kinds: 'whole' | 'sums' (over every dimension but the first), 'vals' (the sampled entries), 'max'"""
    rec = {}
    for name, g in grads.items():
        g = np.asarray(g, np.float64)
        if g.size <= WHOLE_MAX:
            rec[name] = {'whole': g.reshape(-1)}
        else:
            rec[name] = {'sums': g.reshape(g.shape[0], -1).sum(1), 'vals': g.reshape(-1)[index[name]], 'max': np.abs(g).max().reshape(1)}
    return rec


def module_errors(got, ref64):
    """The metric (one function for the reference's own error and for every tested leg).  For every tensor k and every stored quantity q of
    it:  max |got_q - ref64_q| / max(max |ref64_q|, FLOOR * S_m),  S_m = the largest max |ref64_q| of that kind in k's top-level module;
    a tensor's error is the largest over its quantities, a module's the largest over its tensors.  (The floor: ten tensors' true gradient is
    zero - the conv biases directly in front of an InstanceNorm and rgb_fc.4.bias - and both sides hold rounding noise only.)
    -> (module -> error, module -> the tensor that sets it)"""
    scale = {}
    for name, qs in ref64.items():
        for kind, v in qs.items():
            key = (module_of(name), kind)
            scale[key] = max(scale.get(key, 0.0), float(np.abs(v).max()))
    err, worst = {}, {}
    for name, qs in ref64.items():
        m = module_of(name)
        for kind, v in qs.items():
            g = np.asarray(got[name][kind], np.float64)
            assert g.shape == v.shape, (name, kind, g.shape, v.shape)
            e = float(np.abs(g - v).max()) / max(float(np.abs(v).max()), FLOOR * scale[(m, kind)])
            if not np.isfinite(e):
                e = float('inf')
            if e >= err.get(m, -1.0):
                err[m], worst[m] = e, '%s[%s]' % (name, kind)
    return err, worst


KINDS = ('whole', 'sums', 'vals', 'max')


def pack_record(rec, shapes):
    """record -> flat arrays for the npz: one concatenation per kind, tensors in sorted-name order"""
    out = {}
    for kind in KINDS:
        parts = [rec[n][kind] for n in sorted(shapes) if kind in rec[n]]
        out['grad.' + kind] = np.concatenate(parts) if parts else np.zeros(0)
    return out


def unpack_record(z, shapes):
    """inverse of pack_record (z: the loaded npz, shapes: name -> shape) -> (record, index)"""
    rec, index, pos, ipos = {n: {} for n in shapes}, {}, {k: 0 for k in KINDS}, 0
    for n in sorted(shapes):
        size = int(np.prod(shapes[n]))
        lens = {'whole': size} if size <= WHOLE_MAX else {'sums': int(shapes[n][0]), 'vals': N_TOP + N_RANDOM, 'max': 1}
        for kind, ln in lens.items():
            rec[n][kind] = np.asarray(z['grad.' + kind][pos[kind]:pos[kind] + ln], np.float64)
            pos[kind] += ln
        if size > WHOLE_MAX:
            index[n] = np.asarray(z['grad.index'][ipos:ipos + N_TOP + N_RANDOM], np.int64)
            ipos += N_TOP + N_RANDOM
    return rec, index


def load_case(name):
    """-> (args, shapes, record, index, z) of tests/golden/case_c5_gen_step_<name>.npz"""
    z = np.load(os.path.join(HERE, 'case_c5_gen_step_%s.npz' % name), allow_pickle=False)
    args = json.loads(str(z['args_json']))
    shapes = {k: tuple(v) for k, v in json.loads(str(z['shapes_json'])).items()}
    rec, index = unpack_record(z, shapes)
    return args, shapes, rec, index, z


# ---- the reference runs ---------------------------------------------------------------------------------------------------------------
def build_reference_model(ns, a):
    import importlib
    import torch
    from make_golden import fill_buffers_by_name, fill_by_name
    init_net = importlib.import_module('network.init_net')
    real_cuda, real_load = torch.Tensor.cuda, init_net.load_ckpt
    torch.Tensor.cuda = lambda self, *a_, **k_: self
    init_net.load_ckpt = lambda *a_, **k_: None
    try:
        model = ns.renderer.NeuralRayGenRenderer(net_cfg(a))
    finally:
        torch.Tensor.cuda, init_net.load_ckpt = real_cuda, real_load
    fill_by_name(model, scale=WEIGHT_SCALE)
    fill_buffers_by_name(model.init_net.mvsnet)
    return model.train(), init_net


def reference_step(model, init_net, loss_mod, a, inputs, volume, double):
    """one forward + loss + backward of the reference -> (outputs, loss terms, loss, name -> gradient), numpy"""
    import torch
    que, ref, src = inputs
    up = (lambda v: torch.from_numpy(v).double() if v.dtype == np.float32 else torch.from_numpy(v)) if double else torch.from_numpy
    data = {'que_imgs_info': {k: up(v) for k, v in que.items()}, 'ref_imgs_info': {k: up(v) for k, v in ref.items()},
            'src_imgs_info': {k: up(v) for k, v in src.items()}, 'scene_name': 'synthetic'}
    model = model.double() if double else model.float()
    model.zero_grad(set_to_none=True)
    cost_reg, depth = (up(v) for v in volume)
    real_volume, real_coords = init_net.construct_cost_volume_with_src, model.gen_depth_loss_coords
    init_net.construct_cost_volume_with_src = lambda *a_, **k_: (cost_reg, depth)
    if double:      # (grid_sample refuses a float32 grid - which int64 pixel pairs become - on float64 maps)
        model.gen_depth_loss_coords = lambda *a_, **k_: real_coords(*a_, **k_).double()
    try:
        torch.manual_seed(int(a['torch_seed']))
        out = model(data)
        terms = {}
        for name in LOSS_NAMES:                                     # train/trainer.py:124-132
            terms.update(loss_mod.name2loss[name](dict(LOSS_CFG))(out, data, 0))
        loss = 0
        for k, v in terms.items():
            if k.startswith('loss'):
                loss = loss + torch.mean(v)
        loss.backward()
    finally:
        init_net.construct_cost_volume_with_src = real_volume
        if double:
            del model.gen_depth_loss_coords
    grads = {}
    for k, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None, k
            grads[k] = p.grad.detach().double().numpy().copy()
    return ({k: v.detach().numpy() for k, v in out.items()}, {k: v.detach().double().numpy() for k, v in terms.items()},
            float(loss.detach()), grads)


def reference_case(ns, name, volume=None):
    """both runs of one case -> (the dict that is stored, r_m, the tensors that set r_m, the frozen MVSNet's (cost_reg, depth) as computed
    now).  volume: run on this (cost_reg, depth) instead of the one computed now (the stored one: the float64 run is then reproducible to
    float64 rounding whatever order this host's float32 MVSNet sums in)"""
    import importlib
    import torch
    a = CASES[name]
    loss_mod = importlib.import_module('network.loss')
    model, init_net = build_reference_model(ns, a)
    inputs = case_inputs(a)
    que, ref, src = inputs
    with torch.no_grad():
        t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}      # noqa: E731
        cost_reg, depth = init_net.construct_cost_volume_with_src(t(ref), t(src), model.init_net.mvsnet, int(a['cost_volume_sn']),
                                                                  model.init_net.imagenet_mean, model.init_net.imagenet_std, True)
    fresh = (cost_reg.numpy().copy(), depth.numpy().copy())
    volume = fresh if volume is None else volume
    out32, terms32, loss32, g32 = reference_step(model, init_net, loss_mod, a, inputs, volume, False)
    out64, terms64, loss64, g64 = reference_step(model, init_net, loss_mod, a, inputs, volume, True)
    assert out64['pixel_colors_nr_fine'].dtype == np.float64 and all(v.dtype == np.float64 for v in g64.values())
    for k in EXACT_KEYS:
        assert np.array_equal(np.asarray(out32[k], np.int64), np.asarray(out64[k], np.int64)), k      # the two runs took the same branches
    index = {k: sample_index(k, g) for k, g in g64.items() if g.size > WHOLE_MAX}
    rec64, rec32 = grad_record(g64, index), grad_record(g32, index)
    r_m, worst = module_errors(rec32, rec64)
    shapes = {k: list(g.shape) for k, g in g64.items()}
    save = {'args_json': np.array(json.dumps(a)), 'shapes_json': np.array(json.dumps(shapes)), 'cost_reg': volume[0], 'depth': volume[1],
            'loss': np.float64(loss64), 'loss32': np.float64(loss32),
            'grad.index': np.concatenate([index[k] for k in sorted(index)]).astype(np.int32),
            'r_m.names': np.array(sorted(r_m)), 'r_m': np.array([r_m[m] for m in sorted(r_m)], np.float64)}
    save.update(pack_record(rec64, shapes))
    save.update({'term.' + k: v for k, v in terms64.items()})
    save.update({'out.' + k: out64[k].astype(np.float32) for k in OUTPUT_KEYS})
    save.update({'out.' + k: np.asarray(out64[k]).astype(np.int64 if k == 'depth_coords' else np.bool_) for k in EXACT_KEYS})
    save['out32_dev'] = np.array([float(np.abs(out32[k].astype(np.float64) - out64[k]).max()) for k in OUTPUT_KEYS])
    return save, r_m, worst, fresh


def main(only=()):
    import ref_harness
    import torch
    ns = ref_harness.import_reference()
    torch.set_num_threads(8)
    for name in CASES:
        if only and name not in only:
            continue
        save, r_m, worst, _ = reference_case(ns, name)
        path = os.path.join(HERE, 'case_c5_gen_step_%s.npz' % name)
        np.savez_compressed(path, **save)
        print('wrote %s (%d bytes): loss %.8f (fp32 run %.8f), %d gradient tensors' % (
            path, os.path.getsize(path), float(save['loss']), float(save['loss32']), len(json.loads(str(save['shapes_json'])))))
        for m in sorted(r_m):
            print('   r_m %-18s %.2e   (%s)' % (m, r_m[m], worst[m]))


if __name__ == '__main__':
    main(sys.argv[1:])
