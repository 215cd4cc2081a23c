"""neuray_amd.metrics as a drop-in for the reference's network/metrics.py, and the eval.py protocol (neuray_amd.evaluate):
  * the reference's own module (tests/golden/ref_harness.py; its skimage structural_similarity set to the float64 oracle of
    test_metrics.py) and ours on identical data_pr: same keys, shapes, dtypes and values (CPU, kernels on the emulator; skipped
    where the reference tree is absent);
  * patch_reference(metrics=True) makes `network.metrics` ours, unpatch_reference() restores it (reference tree, or the stand-in
    tests/ref_stub where it is absent);
  * VisualizeImage writes the reference's file with the kernel's quantised pixels;
  * evaluate_dirs on PIL-written images against the oracle; on the MI355X the CLI once in a subprocess."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from emu_util import emu_lib
from test_metrics import quantise, smooth_noise, ssim_box11, ssim_gauss11
from neuray_amd import integrate, metrics

sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import ref_harness  # noqa: E402

STUB_ROOT = os.path.join(ROOT, 'tests', 'ref_stub')


def emu_engine():
    from neuray_amd.engine import RenderEngine
    return RenderEngine('cpu', _test_lib=emu_lib())


def _drop_network_modules():
    for k in [k for k in sys.modules if k == 'network' or k.startswith('network.')]:
        del sys.modules[k]


def skimage_ssim_oracle(im1, im2, win_size=11, multichannel=True, data_range=255):
    assert win_size == 11 and multichannel and data_range == 255
    return ssim_box11(im1, im2)


@pytest.fixture
def reference_metrics():
    """the reference's network.metrics, imported as its trainer imports it (third-party stubs only)"""
    if not ref_harness.reference_available():
        pytest.skip('reference tree not present')
    _drop_network_modules()
    ref_harness.import_reference()
    import network.metrics as ref
    ref.structural_similarity = skimage_ssim_oracle        # (the module bound skimage's name at import)
    yield ref
    integrate.unpatch_reference()
    while ref_harness.REFERENCE_ROOT in sys.path:
        sys.path.remove(ref_harness.REFERENCE_ROOT)
    _drop_network_modules()


def data_pr(h, w, seed=0, suffixes=('nr', 'dr', 'nr_fine', 'dr_fine')):
    rng = np.random.RandomState(seed)
    gt = smooth_noise(rng, 1, h, w)
    d = {'pixel_colors_gt': torch.from_numpy(gt), 'que_imgs_info': {'imgs': torch.zeros(1, 3, h, w)}}
    for i, s in enumerate(suffixes):
        d['pixel_colors_%s' % s] = torch.from_numpy(np.clip(gt + (0.03 + 0.04 * i) * rng.randn(1, h * w, 3).astype(np.float32), -0.1, 1.1))
    return d


def test_psnr_ssim_matches_the_reference_module(reference_metrics):
    ref = reference_metrics
    h, w = 26, 45
    d = data_pr(h, w)
    want = ref.PSNR_SSIM({})(d, {}, 0)
    got = metrics.PSNR_SSIM({}, engine=emu_engine())(d, {}, 0)
    assert list(got) == list(want) == ['psnr_nr', 'ssim_nr', 'psnr_dr', 'ssim_dr', 'psnr_nr_fine', 'ssim_nr_fine', 'psnr_dr_fine', 'ssim_dr_fine']
    for k in want:
        assert got[k].dtype == want[k].dtype == torch.float32 and got[k].shape == want[k].shape == (1,), k
        assert got[k].device.type == 'cpu'
        tol = 1e-4 if k.startswith('psnr') else 1e-7           # the reference's PSNR sums in float32; SSIM: the same float64 value, cast
        assert abs(float(got[k]) - float(want[k])) <= tol, (k, float(got[k]), float(want[k]))
    # only the outputs present: nr alone
    d2 = data_pr(h, w, 1, ('nr', 'nr_fine'))
    assert list(metrics.PSNR_SSIM({}, engine=emu_engine())(d2, {}, 0)) == list(ref.PSNR_SSIM({})(d2, {}, 0))
    # compute_psnr / structural_similarity on uint8 images, and the key metrics on a results dict
    g, p = quantise(d['pixel_colors_gt'].numpy()).reshape(h, w, 3), quantise(d['pixel_colors_dr'].numpy()).reshape(h, w, 3)
    eng = emu_engine()
    assert abs(metrics.compute_psnr(g, p, engine=eng) - float(ref.compute_psnr(g, p))) <= 1e-4
    mask = np.ones((h, w), np.float32) * 2
    mask[: h // 2] = 0
    assert abs(metrics.compute_psnr(g, p, True, mask, engine=eng) - float(ref.compute_psnr(g, p, True, mask))) <= 1e-4   # (the quirk)
    assert abs(metrics.structural_similarity(g, p, win_size=11, multichannel=True, data_range=255, engine=eng) - ssim_box11(g, p)) <= 1e-9
    results = {'psnr_nr': [20.5, 21.25], 'psnr_nr_fine': [22.0, 23.5, 24.0]}
    for name in ('psnr_nr', 'psnr_nr_fine'):
        assert metrics.name2key_metrics[name](results) == ref.name2key_metrics[name](results)
    assert sorted(metrics.name2metrics) == sorted(ref.name2metrics)


def test_structural_similarity_refuses_other_call_shapes():
    g = np.zeros((12, 12, 3), np.uint8)
    for kw in ({'win_size': 7}, {'gaussian_weights': True}, {'data_range': 1.0}, {'multichannel': False}):
        with pytest.raises(NotImplementedError, match='win_size=11, multichannel=True, data_range=255'):
            metrics.structural_similarity(g, g, **kw)


def test_patch_reference_installs_and_restores_network_metrics(reference_metrics):
    """the reference's module is already imported: its public names are replaced in place, then restored"""
    ref = reference_metrics
    saved = {n: getattr(ref, n) for n in metrics.__all__}
    integrate.patch_reference(metrics=True)
    import network.metrics as nm
    for n in metrics.__all__:
        assert getattr(nm, n) is getattr(metrics, n), n
    integrate.unpatch_reference()
    for n in metrics.__all__:
        assert getattr(sys.modules['network.metrics'], n) is saved[n], n


def test_patch_reference_installs_the_module_before_import():
    """network.metrics not imported yet (the reference's needs skimage; here the stand-in tree has none): sys.modules gets ours"""
    _drop_network_modules()
    while ref_harness.REFERENCE_ROOT in sys.path:
        sys.path.remove(ref_harness.REFERENCE_ROOT)
    sys.path.insert(0, STUB_ROOT)
    try:
        integrate.patch_reference(metrics=True)
        from network.metrics import PSNR_SSIM, name2metrics
        import network
        assert PSNR_SSIM is metrics.PSNR_SSIM and name2metrics is metrics.name2metrics and network.metrics is metrics
        integrate.unpatch_reference()
        assert 'network.metrics' not in sys.modules and 'metrics' not in network.__dict__
        # the launcher's flag reaches patch_reference; off by default
        from neuray_amd import launch
        calls = []
        real = launch.run
        launch.run = lambda *a, **k: calls.append(k)
        try:
            launch.main(['--metrics', 'run_training.py', '--cfg', 'x.yaml'])
            launch.main(['run_training.py'])
        finally:
            launch.run = real
        assert calls[0]['metrics'] is True and calls[1]['metrics'] is False
    finally:
        integrate.unpatch_reference()
        sys.path.remove(STUB_ROOT)
        _drop_network_modules()


def test_visualize_image_writes_the_reference_file(tmp_path, monkeypatch):
    from neuray_amd import database
    monkeypatch.chdir(tmp_path)
    h, w = 20, 31
    d = data_pr(h, w, 2, ('nr', 'dr', 'nr_fine'))
    out = metrics.VisualizeImage({}, engine=emu_engine())(d, {}, 1200, data_index=3, model_name='m')
    assert out == {}
    path = tmp_path / 'data' / 'vis_val' / 'm' / 'step-1200-index-3.png'
    got = database.imread(str(path))
    want = np.concatenate([quantise(d[k].numpy()).reshape(h, w, 3) for k in
                           ('pixel_colors_gt', 'pixel_colors_nr', 'pixel_colors_dr', 'pixel_colors_nr_fine')], 1)
    np.testing.assert_array_equal(got, want)
    # the reference's concatenation: shorter images zero-padded at the bottom
    a, b = np.full((3, 2, 3), 7, np.uint8), np.full((5, 1, 3), 9, np.uint8)
    c = metrics.concat_images_list(a, b)
    assert c.shape == (5, 3, 3) and (c[3:, :2] == 0).all() and (c[:3, :2] == 7).all() and (c[:, 2] == 9).all()


def write_eval_dirs(root, sizes, seed=0):
    """eval.py's layout: {dir_gt}/{k}.jpg and {dir_pr}/{k}-nr_fine.jpg (PNG-coded: lossless; PIL decodes by content)"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    dg, dp = root / 'gt', root / 'pr'
    dg.mkdir()
    dp.mkdir()
    pairs = []
    for k, (h, w) in enumerate(sizes):
        g = quantise(smooth_noise(rng, 1, h, w)).reshape(h, w, 3)
        p = np.clip(g.astype(int) + rng.randint(-20, 21, g.shape), 0, 255).astype(np.uint8)
        Image.fromarray(g).save(str(dg / ('%d.jpg' % k)), format='PNG')
        Image.fromarray(p).save(str(dp / ('%d-nr_fine.jpg' % k)), format='PNG')
        pairs.append((g, p))
    return str(dg), str(dp), pairs


def test_evaluate_dirs_matches_the_oracle(tmp_path):
    from neuray_amd.evaluate import evaluate_dirs
    dg, dp, pairs = write_eval_dirs(tmp_path, [(24, 33), (24, 33), (19, 40), (24, 33)])
    eng = emu_engine()
    for variant, oracle in (('gauss11', ssim_gauss11), ('box11', ssim_box11)):
        res = evaluate_dirs(dg, dp, ssim=variant, engine=eng)
        assert res['lpips'] is None and res['ssim_variant'] == variant and len(res['images']) == 4
        for k, (g, p) in enumerate(pairs):
            mse = ((g.astype(np.float64) - p) ** 2).mean()
            assert abs(res['images'][k]['psnr'] - 10 * np.log10(255.0 ** 2 / mse)) <= 1e-9
            assert abs(res['images'][k]['ssim'] - oracle(g, p)) <= 1e-9
        assert abs(res['ssim'] - np.mean([oracle(g, p) for g, p in pairs])) <= 1e-9


@pytest.mark.gpu
def test_evaluate_cli_on_the_gpu(tmp_path):
    dg, dp, pairs = write_eval_dirs(tmp_path, [(64, 80), (64, 80), (50, 72)])
    out = str(tmp_path / 'res.json')
    p = subprocess.run([sys.executable, '-m', 'neuray_amd.evaluate', '--dir_gt', dg, '--dir_pr', dp, '--json', out], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.load(open(out))
    want_ssim = np.mean([ssim_gauss11(g, pr) for g, pr in pairs])
    want_psnr = np.mean([10 * np.log10(255.0 ** 2 / ((g.astype(np.float64) - pr) ** 2).mean()) for g, pr in pairs])
    assert abs(res['ssim'] - want_ssim) <= 1e-9 and abs(res['psnr'] - want_psnr) <= 1e-9
    assert p.stdout.strip().splitlines()[-1] == 'psnr %.4f ssim %.4f lpips not computed' % (res['psnr'], res['ssim'])
