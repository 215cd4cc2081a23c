"""python -m neuray_amd.evaluate with LPIPS (neuray_amd/lpips.py): evaluate_dirs on PIL-written images with a thin network (seeded random
weights, kernels on the emulator) against the float64 oracle and the accuracy gate of tests/test_lpips.py; the result and the printed
line without weights, unchanged; on the MI355X the CLI once in a fresh child process with --lpips-weights naming an .npz of
save_weights()."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT
from test_lpips import THIN, engine, oracle, random_weights, smooth_u8, to_f32

NOISE = 0.05            # every prediction: the ground truth + uniform noise of 5 % of full scale
FLOOR = 2e-5            # (the gate of tests/test_lpips.py for noise >= 0.05)


def write_eval_dirs(root, sizes, seed=5):
    rng = np.random.RandomState(seed)
    dg, dp = root / 'gt', root / 'pr'
    dg.mkdir()
    dp.mkdir()
    pairs = []
    for k, (h, w) in enumerate(sizes):
        g = smooth_u8(rng, h, w)
        p = np.clip(g.astype(int) + rng.randint(-int(NOISE * 255), int(NOISE * 255) + 1, g.shape), 0, 255).astype(np.uint8)
        Image.fromarray(g).save(str(dg / ('%d.jpg' % k)), format='PNG')           # (lossless: the decoded pixels are these)
        Image.fromarray(p).save(str(dp / ('%d-nr_fine.jpg' % k)), format='PNG')
        pairs.append((g, p))
    return str(dg), str(dp), pairs


def check_images(res, W, pairs):
    for k, (g, p) in enumerate(pairs):
        f64 = oracle(W, to_f32(p[None]), to_f32(g[None]), torch.float64).sum()
        f32 = oracle(W, to_f32(p[None]), to_f32(g[None]), torch.float32).sum()
        err = abs(res['images'][k]['lpips'] - f64)
        print('image %d: lpips %.6f, err %.1e (eager32 %.1e)' % (k, f64, err / f64, abs(f32 - f64) / f64))
        assert err <= max(4 * abs(f32 - f64), FLOOR * abs(f64))
    assert res['lpips'] == float(np.mean([r['lpips'] for r in res['images']]))


def test_evaluate_dirs_with_lpips_matches_the_oracle(tmp_path, capsys):
    from neuray_amd import evaluate
    from neuray_amd.lpips import LPIPS
    dg, dp, pairs = write_eval_dirs(tmp_path, [(20, 26), (20, 26), (17, 30)])
    eng = engine('emu')
    W = random_weights(THIN, 200)
    res = evaluate.evaluate_dirs(dg, dp, engine=eng, lpips=LPIPS(W, engine=eng))
    assert len(res['images']) == 3 and sorted(res['images'][0]) == ['index', 'lpips', 'psnr', 'ssim']
    check_images(res, W, pairs)
    bare = evaluate.evaluate_dirs(dg, dp, engine=eng)
    assert bare['lpips'] is None and all(sorted(r) == ['index', 'psnr', 'ssim'] for r in bare['images'])
    assert bare['psnr'] == res['psnr'] and bare['ssim'] == res['ssim']


def test_printed_lines_with_and_without_weights(tmp_path, capsys, monkeypatch):
    """main() with evaluate_dirs on the emulator engine: `psnr X ssim Y lpips Z` with weights (flag or environment variable), today's
    `... lpips not computed` without"""
    from neuray_amd import evaluate, lpips
    dg, dp, _ = write_eval_dirs(tmp_path, [(16, 20)])
    eng = engine('emu')
    npz = str(tmp_path / 'thin.npz')
    lpips.save_weights(npz, random_weights(THIN, 201))
    real = evaluate.evaluate_dirs
    seen = []

    def on_emulator(dir_gt, dir_pr, ssim='gauss11', lpips=None):
        seen.append(lpips)
        return real(dir_gt, dir_pr, ssim=ssim, engine=eng, lpips=lpips)
    monkeypatch.setattr(evaluate, 'evaluate_dirs', on_emulator)
    monkeypatch.delenv('NEURAY_LPIPS_WEIGHTS', raising=False)
    res = evaluate.main(['--dir_gt', dg, '--dir_pr', dp])
    assert res['lpips'] is None and seen[-1] is None
    assert capsys.readouterr().out.strip().splitlines()[-1] == 'psnr %.4f ssim %.4f lpips not computed' % (res['psnr'], res['ssim'])
    res = evaluate.main(['--dir_gt', dg, '--dir_pr', dp, '--lpips-weights', npz])
    assert seen[-1] == [npz] and res['lpips'] > 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line == 'psnr %.4f ssim %.4f lpips %.4f' % (res['psnr'], res['ssim'], res['lpips'])
    monkeypatch.setenv('NEURAY_LPIPS_WEIGHTS', npz)
    env = evaluate.main(['--dir_gt', dg, '--dir_pr', dp])
    assert seen[-1] == [npz] and env['lpips'] == res['lpips']


@pytest.mark.gpu
def test_evaluate_cli_with_lpips_on_the_gpu(tmp_path):
    from neuray_amd import lpips
    dg, dp, pairs = write_eval_dirs(tmp_path, [(64, 80), (64, 80), (50, 72)])
    W = random_weights(THIN, 202)
    npz, out = str(tmp_path / 'thin.npz'), str(tmp_path / 'res.json')
    lpips.save_weights(npz, W)
    p = subprocess.run([sys.executable, '-m', 'neuray_amd.evaluate', '--dir_gt', dg, '--dir_pr', dp, '--lpips-weights', npz, '--json', out],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.load(open(out))
    check_images(res, W, pairs)
    assert p.stdout.strip().splitlines()[-1] == 'psnr %.4f ssim %.4f lpips %.4f' % (res['psnr'], res['ssim'], res['lpips'])
