"""eval.py's protocol on the HIP metrics kernels (neuray_image_metrics, and neuray_amd.lpips for the third number):

    python -m neuray_amd.evaluate --dir_gt D --dir_pr D [--ssim gauss11|box11] [--lpips-weights PATH [PATH ...]] [--json out.json]

pairs {dir_gt}/{k}.jpg with {dir_pr}/{k}-nr_fine.jpg for k in range(number of files in dir_gt), decoded with PIL
(database.imread), and prints `psnr X ssim Y` (means over the images, 4 decimals).  PSNR = 10 log10(255^2 / MSE) of the decoded
uint8 images (tf.image.psnr); SSIM gauss11 = tf.image.ssim (the default, eval.py's), box11 = skimage's structural_similarity of
the validation metric.  Consecutive images of one size go through one kernel launch.  LPIPS (eval.py: lpips.LPIPS(net='vgg') on
the images scaled to [-1, 1]) is computed when its weights are named - --lpips-weights, or the environment variable
NEURAY_LPIPS_WEIGHTS (paths joined by os.pathsep): a full LPIPS state_dict, torchvision's vgg16 state_dict + the lpips package's
vgg.pth, or an .npz of neuray_amd.lpips.save_weights - and the line becomes `psnr X ssim Y lpips Z`.  The VGG and linear layer
weights are not part of this project and are never downloaded; without them the output says `lpips not computed`.
"""
import argparse
import json
import os

import numpy as np
import torch

from . import database

BATCH = 16          # images per launch (a batch of same-sized neighbours)


def _decode(path):
    img = database.imread(path)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError('neuray_amd.evaluate: %s is not an 8-bit RGB image (%s %s)' % (path, img.dtype, img.shape))
    return img


def evaluate_dirs(dir_gt, dir_pr, ssim='gauss11', engine=None, device=None, lpips=None):
    """-> {'psnr': mean, 'ssim': mean, 'ssim_variant', 'lpips': None, 'images': [{'index', 'psnr', 'ssim'}, ...]}
    lpips: a neuray_amd.lpips.LPIPS object, or the path(s) of its weights: every image record gains 'lpips' and the result's 'lpips' is
    the mean."""
    from .metrics import _engine
    eng = _engine(device if device is not None else 'cuda', engine)
    if lpips is not None and not callable(lpips):
        from .lpips import LPIPS
        lpips = LPIPS(lpips, engine=eng)
    num = len(os.listdir(dir_gt))
    pairs = [(_decode(f'{dir_gt}/{k}.jpg'), _decode(f'{dir_pr}/{k}-nr_fine.jpg')) for k in range(num)]
    for k, (gt, pr) in enumerate(pairs):
        if gt.shape != pr.shape:
            raise ValueError('neuray_amd.evaluate: image %d: ground truth %s and prediction %s differ in size' % (k, gt.shape, pr.shape))
    psnr, val, lp = [], [], []
    k = 0
    while k < num:
        e = k + 1
        while e < num and e - k < BATCH and pairs[e][0].shape == pairs[k][0].shape:
            e += 1
        h, w = pairs[k][0].shape[:2]
        gt = torch.from_numpy(np.stack([p[0] for p in pairs[k:e]]))
        pr = torch.from_numpy(np.stack([p[1] for p in pairs[k:e]]))
        r = eng.image_metrics(pr, gt, h, w, ssim=ssim)
        out = torch.stack([r['psnr'], r['ssim']]).cpu().numpy()
        psnr += out[0].tolist()
        val += out[1].tolist()
        if lpips is not None:
            lp += lpips(pr, gt).cpu().numpy().tolist()          # (the same batch, in the metric's own memory chunks)
        k = e
    images = [{'index': i, 'psnr': p, 'ssim': s} for i, (p, s) in enumerate(zip(psnr, val))]
    for rec, v in zip(images, lp):
        rec['lpips'] = v
    return {'psnr': float(np.mean(psnr)) if num else float('nan'), 'ssim': float(np.mean(val)) if num else float('nan'),
            'ssim_variant': ssim, 'lpips': (float(np.mean(lp)) if num else float('nan')) if lpips is not None else None,
            'images': images}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--dir_gt', type=str, default='data/render/fern/gt')
    ap.add_argument('--dir_pr', type=str, default='data/render/fern/neuray_gen_depth-pretrain-eval')
    ap.add_argument('--ssim', choices=('gauss11', 'box11'), default='gauss11')
    env = os.environ.get('NEURAY_LPIPS_WEIGHTS')
    ap.add_argument('--lpips-weights', type=str, nargs='+', default=env.split(os.pathsep) if env else None, metavar='PATH',
                    help='LPIPS weights: a full LPIPS state_dict, vgg16 state_dict + vgg.pth, or an .npz of neuray_amd.lpips.save_weights '
                         '(default: $NEURAY_LPIPS_WEIGHTS)')
    ap.add_argument('--json', type=str, default=None, help='write the per-image values here')
    args = ap.parse_args(argv)
    res = evaluate_dirs(args.dir_gt, args.dir_pr, ssim=args.ssim, lpips=args.lpips_weights)
    if res['lpips'] is None:
        print(f"psnr {res['psnr']:.4f} ssim {res['ssim']:.4f} lpips not computed")
    else:
        print(f"psnr {res['psnr']:.4f} ssim {res['ssim']:.4f} lpips {res['lpips']:.4f}")
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == '__main__':
    main()
