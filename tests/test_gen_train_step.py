"""One whole generalisation training step at BASELINE config 5's structure (neuray_gen_cost_volume_train.yaml: NeuralRayGenRenderer with the
cost-volume init net, both encoders, render + depth loss through neuray_amd.loss, backward) against the REFERENCE's own float64 autograd
(tests/golden/case_c5_gen_step_{a,b}.npz, written by tests/golden/make_golden_gen_step.py): every trainable parameter's gradient - the
init net's heads and encoder, image_encoder, vis_encoder, the decoders and aggregation networks of both passes - the depth-loss readout
(interpolate_feature_map -> predict_mean -> its backward -> the map scatter) and the accumulation over several ray batches of one step.

Inputs are identical on both sides: the scene is regenerated from the stored arguments, the weights are fill_by_name(scale 0.1), the
frozen MVSNet's `cost_reg` / `depth` are the stored float32 ones (patched in, as the reference runs were given them), and
torch.manual_seed makes both sides draw the same fine-sampling uniforms and the same depth-loss permutation.

The metric is make_golden_gen_step.module_errors, per top-level module, on the stored gradient record.  The yardstick is `r_m`: the
reference's OWN float32 run against its float64 run under the same metric (stored).  Gates (never from what the code under test gives):
  emulator                                    4 r_m          (the margin tests/test_conv2d_x3.py and test_raycast.py give over a
                                                              reference's own rounding)
  hip, dist_decoder / agg_net / fine_*        4 max_m r_m    (a single decoder's r_m of 1e-6 is summation-order noise: the step's worst
                                                              module is the measure)
  hip, init_net / image_encoder / vis_encoder 4 max(r_m, l_m)   l_m: the same step on the same device through the PyTorch / MIOpen
                                                              library path alone (x3 convolutions, fused norm, fused MVSNet kernels off)
                                                              - a second reference, computed here, not the code under test
every gate capped at the project's whole-step gradient gate of 5e-3.

What the gates can and cannot see.  The step has kinks: every ReLU unit whose pre-activation lies within float32 rounding of zero is on one
branch in one float32 evaluation and on the other in the next, and changes the gradients by its whole contribution.  The float64 run is a
yardstick only where the code under test sits on its branches, so case a's seed was chosen from the reference alone for the distance of
its per-ray ReLU units from the kink (make_golden_gen_step.py, "The seeds"; at the seed tried first the only misses, on both backends,
were two rows of agg_net.prob_embed.0.weight, each equal to g_out * input of ONE unit with a float64 pre-activation of +-1.8e-6, to
1e-9).  In case b the reference's own float32 run leaves the float64 branches in the encoders (r_m 2e-2 / 1e-1), so do the library
path and ours on the MI355X, and every gate of that case is the cap.

Measured (every leg prints its table: pytest -s):
                                     emulator     MI355X    MI355X    MI355X ours           gate
  case a                 r_m         ours         l_m       ours      (deterministic)       emulator / MI355X
  agg_net                1.74e-05    1.27e-05     7.70e-06  1.25e-05  1.25e-05      6.97e-05 / 1.11e-04
  dist_decoder           1.44e-06    2.13e-06     2.61e-06  1.96e-06  2.01e-06      5.77e-06 / 1.11e-04
  fine_agg_net           1.52e-06    1.90e-06     1.11e-06  1.05e-06  1.05e-06      6.08e-06 / 1.11e-04
  fine_dist_decoder      8.90e-07    7.92e-07     1.23e-06  1.69e-06  1.63e-06      3.56e-06 / 1.11e-04
  image_encoder          2.51e-05    1.91e-05     1.75e-05  1.49e-05  1.46e-05      1.00e-04 / 1.00e-04
  init_net               2.78e-05    2.68e-05     2.43e-05  2.34e-05  2.31e-05      1.11e-04 / 1.11e-04
  vis_encoder            1.94e-05    1.03e-05     5.88e-06  6.04e-06  7.56e-06      7.76e-05 / 7.76e-05
  Outputs within 1.5e-6 of the float64 ones on both backends, loss 0.60507977 against
  0.60507984; own cost volume: cost_reg 3.6e-6 / 5.6e-6, depth 1.1e-6 / 1.7e-6 (emulator / MI355X), the same loss.
  case b (MI355X)    r_m         l_m         ours        gate
  agg_net            3.69e-05    6.02e-06    7.88e-06    5e-3
  dist_decoder       2.44e-06    1.68e-06    2.26e-06    5e-3
  fine_agg_net       4.08e-07    1.03e-04    1.03e-04    5e-3      (a prob_embed unit on the other branch, in both paths)
  fine_dist_decoder  7.26e-07    1.55e-04    1.55e-04    5e-3
  image_encoder      2.41e-02    4.37e-04    4.37e-04    5e-3
  init_net           9.90e-02    3.32e-02    2.82e-03    5e-3
  vis_encoder        4.68e-06    3.03e-03    3.03e-03    5e-3
  (two separate runs gave the same figures to three digits.)  Seconds per leg on the MI355X: 6 (the first, with the library's
  kernel selection), 1 - 2 each after that; the emulator's step takes 27 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from emu_util import emu_lib
from test_cost_volume import fill_buffers_by_name
from test_encoders import fill_by_name
from neuray_amd import loss as nloss
from neuray_amd.network import encoders, fused_norm, init_net, mvsnet
from neuray_amd.network import render_ops as ro
from neuray_amd.network import renderer as R

sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import make_golden_gen_step as mg  # noqa: E402  (its top half is pure numpy; only main() imports the reference)
import ref_harness  # noqa: E402

CAP = 5e-3                      # the project's whole-step gradient gate (test_scene_renderers.py, test_loss_reference.py, smoke())
MARGIN = 4
PER_RAY = ('dist_decoder', 'agg_net', 'fine_dist_decoder', 'fine_agg_net')
OUT_TOL = {'cpu': 2e-4, 'cuda:0': 1e-3}           # test_scene_renderers.py's output tolerances
_CASES, _LIBRARY, _STEPS = {}, {}, {}


def case(name):
    if name not in _CASES:
        args, shapes, rec, index, z = mg.load_case(name)
        _CASES[name] = {'args': args, 'shapes': shapes, 'rec': rec, 'index': index, 'z': {k: z[k] for k in z.files},
                        'r_m': dict(zip([str(m) for m in z['r_m.names']], [float(v) for v in z['r_m']])), 'inputs': mg.case_inputs(args)}
    return _CASES[name]


@pytest.fixture
def emu():
    """the kernels on the emulator; the encoders' 3 x 3 layers through PyTorch's CPU convolutions (test_scene_renderers.py's fixture: a
    pass through the emulated MFMA costs minutes, and the kernel has its own emulator tests)"""
    ro._ENGINES.clear()
    ro._TEST_LIB = emu_lib()
    encoders.set_x3_conv(False)
    try:
        yield 'cpu'
    finally:
        encoders.set_x3_conv(True)
        ro._TEST_LIB = None
        ro._ENGINES.clear()


@pytest.fixture
def hip():
    ro._ENGINES.clear()
    ro._TEST_LIB = None
    return 'cuda:0'


def step(name, dev, deterministic=False, own_volume=False, grad=True):
    """our step on the case's inputs -> (outputs, loss, name -> gradient or None, (cost_reg, depth) as computed when own_volume)"""
    c = case(name)
    a, (que, ref, src) = c['args'], c['inputs']
    gen = R.NeuralRayGenRenderer({**mg.net_cfg(a), 'hip_deterministic': deterministic}).train()
    fill_by_name(gen, scale=mg.WEIGHT_SCALE)
    fill_buffers_by_name(gen.init_net.mvsnet)
    if dev == 'cpu':
        gen._engine_test_lib = emu_lib()
    gen = gen.to(dev)
    data = {'que_imgs_info': {k: torch.from_numpy(v).to(dev) for k, v in que.items()},
            'ref_imgs_info': {k: torch.from_numpy(v).to(dev) for k, v in ref.items()},
            'src_imgs_info': {k: torch.from_numpy(v).to(dev) for k, v in src.items()}, 'scene_name': 'synthetic'}
    seen = []
    real = init_net.construct_cost_volume_with_src
    if own_volume:
        init_net.construct_cost_volume_with_src = lambda *a_, **k_: (seen.append(real(*a_, **k_)), seen[-1])[1]
    else:
        stored = (torch.from_numpy(c['z']['cost_reg']).to(dev), torch.from_numpy(c['z']['depth']).to(dev))
        init_net.construct_cost_volume_with_src = lambda *a_, **k_: stored
    eng = ro.engine_for(dev)
    losses = [nloss.name2loss[n](dict(mg.LOSS_CFG), engine=eng) for n in mg.LOSS_NAMES]
    try:
        torch.manual_seed(int(a['torch_seed']))
        with torch.enable_grad() if grad else torch.no_grad():
            out = gen(data)
            loss, _ = nloss.total_loss(losses, out, data, 0)
            if grad:
                loss.backward()
    finally:
        init_net.construct_cost_volume_with_src = real
    grads = None
    if grad:
        grads = {}
        for k, p in gen.named_parameters():
            if p.requires_grad:
                assert p.grad is not None, 'no gradient for ' + k
                grads[k] = p.grad.detach().cpu().double().numpy()
        assert sorted(grads) == sorted(c['shapes']) and all(grads[k].shape == c['shapes'][k] for k in grads)
    return ({k: v.detach().cpu().numpy() for k, v in out.items()}, float(loss.detach()), grads,
            tuple(t.cpu().numpy() for t in seen[0]) if seen else None)


def check_forward(name, dev, out, loss):
    z, tol = case(name)['z'], OUT_TOL[dev]
    for k in mg.EXACT_KEYS:
        assert np.array_equal(out[k], z['out.' + k]), k
    for k in mg.OUTPUT_KEYS:
        d = float(np.abs(out[k].astype(np.float64) - z['out.' + k]).max())
        print('%-22s max |ours - ref64| %.2e' % (k, d))
        assert d <= tol, (k, d, tol)
    print('loss ours %.8f, reference float64 %.8f' % (loss, float(z['loss'])))
    assert abs(loss - float(z['loss'])) <= tol


def errors(name, grads):
    c = case(name)
    return mg.module_errors(mg.grad_record(grads, c['index']), c['rec'])


def library_errors(name, dev):
    """l_m: the same step on the same device with every convolution and norm of the encoders and the init net through PyTorch / MIOpen"""
    if name not in _LIBRARY:
        saved = (fused_norm.X3_CONV, fused_norm.FUSED_NORM, mvsnet.FAST_CONV3D, mvsnet.FUSED_ABN)
        encoders.set_x3_conv(False)
        encoders.set_fused_norm(False)
        mvsnet.FAST_CONV3D = mvsnet.FUSED_ABN = False
        try:
            _LIBRARY[name] = errors(name, step(name, dev)[2])[0]
        finally:
            fused_norm.X3_CONV, fused_norm.FUSED_NORM, mvsnet.FAST_CONV3D, mvsnet.FUSED_ABN = saved
    return _LIBRARY[name]


def check_gradients(name, dev, grads):
    r_m = case(name)['r_m']
    ours, worst = errors(name, grads)
    assert sorted(ours) == sorted(r_m)
    l_m = library_errors(name, dev) if dev != 'cpu' else {}
    gates = {}
    for m in r_m:
        if dev == 'cpu':
            gates[m] = MARGIN * r_m[m]
        elif m in PER_RAY:
            gates[m] = MARGIN * max(r_m.values())
        else:
            gates[m] = MARGIN * max(r_m[m], l_m[m])
        gates[m] = min(gates[m], CAP)
    for m in sorted(r_m):
        print('%-18s r_m %.2e  l_m %s  ours %.2e  gate %.2e  (%s)' % (m, r_m[m], '%.2e' % l_m[m] if m in l_m else '   -    ', ours[m], gates[m],
                                                                       worst[m]))
    bad = {m: (ours[m], gates[m], worst[m]) for m in r_m if not ours[m] <= gates[m]}
    assert not bad, bad


def cached_step(name, dev, deterministic=False):
    """one run of the step per leg, shared by its forward and its gradient test"""
    key = (name, dev, deterministic)
    if key not in _STEPS:
        _STEPS[key] = step(name, dev, deterministic)
    return _STEPS[key]


def test_step_forward_on_the_emulator(emu):
    out, loss, _, _ = cached_step('a', emu)
    check_forward('a', emu, out, loss)


def test_step_gradients_on_the_emulator(emu):
    check_gradients('a', emu, cached_step('a', emu)[2])


@pytest.mark.gpu
@pytest.mark.parametrize('deterministic', [False, True])
def test_step_forward(hip, deterministic):
    out, loss, _, _ = cached_step('a', hip, deterministic)
    check_forward('a', hip, out, loss)


@pytest.mark.gpu
@pytest.mark.parametrize('deterministic', [False, True])
def test_step_gradients(hip, deterministic):
    check_gradients('a', hip, cached_step('a', hip, deterministic)[2])


@pytest.mark.gpu
def test_step_forward_over_three_ray_batches(hip):
    """case b: portrait maps, the config's 8 working views, 80 rays at ray_batch_num 32 - three render_impl calls, the last one partial"""
    out, loss, _, _ = cached_step('b', hip)
    assert out['pixel_colors_nr'].shape == (1, 80, 3)
    check_forward('b', hip, out, loss)


@pytest.mark.gpu
def test_step_gradients_accumulate_over_three_ray_batches(hip):
    check_gradients('b', hip, cached_step('b', hip)[2])


def _own_cost_volume(dev):
    from test_cost_volume import relerr
    z = case('a')['z']
    out, loss, _, (cost_reg, depth) = step('a', dev, own_volume=True, grad=False)
    tol = 2e-4 if dev == 'cpu' else 3e-3                   # test_cost_volume.py's, as it applies them to these two tensors
    e_c, e_d = relerr(cost_reg, z['cost_reg']), relerr(depth, z['depth'])
    print('cost_reg %.2e, depth %.2e (gate %.1e); loss ours %.8f, reference float64 %.8f' % (e_c, e_d, 10 * tol, loss, float(z['loss'])))
    assert cost_reg.shape == z['cost_reg'].shape and depth.shape == z['depth'].shape
    assert e_c <= 10 * tol and e_d <= 10 * tol
    assert abs(loss - float(z['loss'])) <= OUT_TOL[dev]


def test_step_with_its_own_cost_volume_on_the_emulator(emu):
    """nothing patched: our frozen MVSNet's cost volume and regressed depth against the stored ones, and the loss of the step built on them"""
    _own_cost_volume(emu)


@pytest.mark.gpu
def test_step_with_its_own_cost_volume(hip):
    _own_cost_volume(hip)


def test_fixture_is_what_the_reference_computes():
    """case a regenerated from the reference tree (where it exists): the float64 loss and gradient records to float64 rounding, the
    reference's own float32 error r_m to within a factor of two (it is a maximum of float32 rounding noise, whose realisation follows the
    host's summation order: thread count, BLAS build)"""
    if not ref_harness.reference_available():
        pytest.skip('reference tree not present')
    drop = lambda: [sys.modules.pop(k) for k in list(sys.modules) if k == 'network' or k.startswith('network.')]      # noqa: E731
    c = case('a')
    z = c['z']
    drop()
    try:
        save, r_m, _, fresh = mg.reference_case(ref_harness.import_reference(), 'a', volume=(z['cost_reg'], z['depth']))
    finally:
        while ref_harness.REFERENCE_ROOT in sys.path:
            sys.path.remove(ref_harness.REFERENCE_ROOT)
        drop()
    # the frozen MVSNet as this host's float32 sums it (probabilities <= 1, depths of a few units)
    assert np.abs(fresh[0] - z['cost_reg']).max() <= 1e-5 and np.abs(fresh[1] - z['depth']).max() <= 1e-4
    assert str(save['shapes_json']) == str(z['shapes_json']) and np.array_equal(save['grad.index'], z['grad.index'])
    assert abs(float(save['loss']) - float(z['loss'])) <= 1e-10
    for k in ('whole', 'sums', 'vals', 'max'):
        assert np.abs(save['grad.' + k] - z['grad.' + k]).max() <= 1e-9 * np.abs(z['grad.' + k]).max(), k
    for k in mg.EXACT_KEYS:
        assert np.array_equal(save['out.' + k], z['out.' + k]), k
    for m, v in c['r_m'].items():
        print('%-18s r_m stored %.2e, regenerated %.2e' % (m, v, r_m[m]))
        assert 0.5 * v <= r_m[m] <= 2 * v, m
