"""neuray_amd.loss as a drop-in for the reference's network/loss.py:
  * the reference's own module (tests/golden/ref_harness.py) and ours on identical data_pr / data_gt: same keys, shapes, dtypes,
    `.keys` and values within float32 (CPU, kernels on the emulator; skipped where the reference tree is absent);
  * patch_reference(loss=True) makes `network.loss` ours before and after the reference imported it, unpatch_reference() restores
    it; `launch --loss` reaches a script;
  * total_loss() is the trainer's sum (train/trainer.py:124-132);
  * one train step of the mirror's NeuralRayFtRenderer followed by total_loss(...).backward() fills the same parameters' .grad as
    the in-line float32 PyTorch losses, each tensor within 5e-3 of its largest entry (the project's per-tensor gradient gate of
    test_ft_train_step_matches_reference)."""
import os
import sys

import numpy as np
import pytest
import torch

import loss_cases as lc
from conftest import GOLDEN_DIR, ROOT
from emu_util import emu_lib
from neuray_amd import integrate
from neuray_amd import loss as nloss

sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import ref_harness  # noqa: E402

STUB_ROOT = os.path.join(ROOT, 'tests', 'ref_stub')
FULL = {'use_dr_loss': True, 'use_dr_fine_loss': True, 'use_nr_fine_loss': True}


def emu_engine():
    from neuray_amd.engine import RenderEngine
    return RenderEngine('cpu', _test_lib=emu_lib())


def _drop_network_modules():
    for k in [k for k in sys.modules if k == 'network' or k.startswith('network.')]:
        del sys.modules[k]


@pytest.fixture
def reference_loss():
    """the reference's network.loss, imported as its trainer imports it (third-party stubs only)"""
    if not ref_harness.reference_available():
        pytest.skip('reference tree not present')
    _drop_network_modules()
    ref_harness.import_reference()
    import network.loss as ref
    yield ref
    integrate.unpatch_reference()
    while ref_harness.REFERENCE_ROOT in sys.path:
        sys.path.remove(ref_harness.REFERENCE_ROOT)
    _drop_network_modules()


def all_data():
    """one data_pr / data_gt with everything the three losses read"""
    rc, cc = lc.render_inputs(71, 1, 96), lc.consist_inputs(72, 1, 96, 8)
    data_pr, data_gt, _ = lc.depth_data(lc.depth_inputs(73, 3, 200, 40, 30, True, True))
    data_pr = {k: v.detach() for k, v in data_pr.items()}
    data_pr.update({k: lc.as_torch(v) for k, v in {**cc, **rc}.items()})
    return data_pr, data_gt


def test_same_keys_shapes_dtypes_and_values_as_the_reference_module(reference_loss):
    ref = reference_loss
    data_pr, data_gt = all_data()
    eng = emu_engine()
    assert sorted(nloss.name2loss) == sorted(ref.name2loss)
    for name in ref.name2loss:
        for cfg in ({}, {**FULL, 'use_ray_mask': False, 'depth_loss_type': 'smooth_l1'}):
            theirs, ours = ref.name2loss[name](cfg), nloss.name2loss[name](cfg, engine=eng)
            assert ours.keys == theirs.keys and ours.cfg == theirs.cfg
            want, got = theirs(data_pr, data_gt, 0), ours(data_pr, data_gt, 0)
            assert list(got) == list(want), name
            for k in want:
                assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype == torch.float32 and got[k].device == want[k].device, k
                assert torch.allclose(got[k], want[k], rtol=2e-6, atol=0), (k, got[k], want[k])
    # the calls without their inputs
    assert nloss.ConsistencyLoss({}, engine=eng)({}, {}, 0) == ref.ConsistencyLoss({})({}, {}, 0) == {}
    a = nloss.DepthLoss({}, engine=eng)(data_pr, {'ref_imgs_info': {}}, 0)['loss_depth']
    b = ref.DepthLoss({})(data_pr, {'ref_imgs_info': {}}, 0)['loss_depth']
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def test_total_loss_equals_the_trainers_sum_on_the_reference_outputs(reference_loss):
    ref = reference_loss
    data_pr, data_gt = all_data()
    losses = [ref.name2loss[n](FULL) for n in ('render', 'depth', 'consist')]
    log_info = {}                                   # train/trainer.py:122-132
    for loss in losses:
        for k, v in loss(data_pr, data_gt, 0).items():
            log_info[k] = v
    want = 0
    for k, v in log_info.items():
        if k.startswith('loss'):
            want = want + torch.mean(v)
    got, info = nloss.total_loss(losses, data_pr, data_gt, 0)
    assert torch.equal(got, want) and list(info) == list(log_info)


def test_patch_reference_replaces_an_imported_network_loss_in_place(reference_loss):
    ref = reference_loss
    from network.loss import name2loss as held          # what train/trainer.py holds after its import
    saved = {n: getattr(ref, n) for n in nloss.REFERENCE_NAMES}
    saved_table = dict(ref.name2loss)
    integrate.patch_reference(loss=True)
    import network.loss as nl
    for n in ('Loss', 'RenderLoss', 'DepthLoss', 'ConsistencyLoss'):
        assert getattr(nl, n) is getattr(nloss, n), n
    assert nl.name2loss == nloss.name2loss and held == nloss.name2loss and held['render'] is nloss.RenderLoss
    integrate.unpatch_reference()
    for n in nloss.REFERENCE_NAMES:
        assert getattr(sys.modules['network.loss'], n) is saved[n], n
    assert held == saved_table and held['render'] is saved['RenderLoss']


def test_patch_reference_installs_the_module_before_import_and_the_launcher_flag(tmp_path):
    _drop_network_modules()
    while ref_harness.REFERENCE_ROOT in sys.path:
        sys.path.remove(ref_harness.REFERENCE_ROOT)
    sys.path.insert(0, STUB_ROOT)
    try:
        integrate.patch_reference()                     # off by default
        assert 'network.loss' not in sys.modules
        integrate.patch_reference(loss=True)
        from network.loss import RenderLoss, name2loss
        import network
        assert RenderLoss is nloss.RenderLoss and name2loss is nloss.name2loss and network.loss is nloss
        integrate.unpatch_reference()
        assert 'network.loss' not in sys.modules and 'loss' not in network.__dict__
        # the launcher: a two-line script sees the patched module
        from neuray_amd import launch
        script = tmp_path / 'two_lines.py'
        script.write_text("import sys, network.loss\nopen(sys.argv[1], 'w').write(network.loss.__name__ + ' ' + network.loss.name2loss['depth'].__module__)\n")
        launch.main(['--loss', str(script), str(tmp_path / 'seen.txt')])
        assert (tmp_path / 'seen.txt').read_text() == 'neuray_amd.loss neuray_amd.loss'
        integrate.unpatch_reference()
        calls = []
        real = launch.run
        launch.run = lambda *a, **k: calls.append(k)
        try:
            launch.main(['run_training.py'])
        finally:
            launch.run = real
        assert calls[0]['loss'] is False
    finally:
        integrate.unpatch_reference()
        while STUB_ROOT in sys.path:
            sys.path.remove(STUB_ROOT)
        if str(tmp_path) in sys.path:
            sys.path.remove(str(tmp_path))
        _drop_network_modules()


def test_mirror_ft_train_step_with_total_loss_fills_the_same_gradients():
    from test_scene_renderers import make_ft
    from neuray_amd.network import encoders
    from neuray_amd.network import render_ops as ro
    gold = np.load(os.path.join(GOLDEN_DIR, 'case_scene.npz'))
    ro._ENGINES.clear()
    ro._TEST_LIB = emu_lib()
    encoders.set_x3_conv(False)
    try:
        grads = []
        for ours in (True, False):
            ft = make_ft(gold, 'cpu').train()
            np.random.seed(3)
            torch.manual_seed(4)
            t = ft({'index': 0})
            if ours:
                losses = [nloss.name2loss[n]({'use_nr_fine_loss': True}, engine=emu_engine()) for n in ('render', 'consist')]
                total, info = nloss.total_loss(losses, t, {'index': 0}, 0)
                assert sorted(info) == ['loss_prob', 'loss_prob_fine', 'loss_rgb_nr', 'loss_rgb_nr_fine']
            else:
                vals = lc.render_terms([t['pixel_colors_nr'], t['pixel_colors_nr_fine']], t['pixel_colors_gt'], t['ray_mask'])
                vals += lc.consist_terms([(t['hit_prob_nr'], t['hit_prob_self']), (t['hit_prob_nr_fine'], t['hit_prob_self_fine'])])
                total = sum(torch.mean(v) for v in vals)
            total.backward()
            grads.append((float(total.detach()), {n: p.grad.clone() for n, p in ft.named_parameters() if p.grad is not None}))
        (la, ga), (lb, gb) = grads
        assert abs(la - lb) <= 1e-5 * abs(lb)
        assert sorted(ga) == sorted(gb) and len(ga) > 10
        for n in gb:
            top = float(gb[n].abs().max())
            assert float((ga[n] - gb[n]).abs().max()) <= 5e-3 * top, (n, float((ga[n] - gb[n]).abs().max()), top)
    finally:
        encoders.set_x3_conv(True)
        ro._TEST_LIB = None
        ro._ENGINES.clear()
