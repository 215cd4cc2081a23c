"""Drop-in for the reference's network/metrics.py: validation metrics (cfg val_metric [psnr_ssim, vis_img], checkpoint selection by
key_metric_name psnr_nr / psnr_nr_fine) on the HIP kernels of neuray_image_metrics (RenderEngine.image_metrics).

Same names, arguments and return types as the reference module; every class and function takes an optional `engine=` (a
RenderEngine; default: the product engine of the tensors' device, which must be the GPU - there is no host fallback).

Deliberate differences:
  * PSNR_SSIM with eval_margin_ratio < 1: the reference crops only the ground truth and pixel_colors_nr and then fails on the shape
    mismatch for dr / nr_fine / dr_fine; here every output is cropped like the ground truth.  No shipped config sets the ratio.
  * compute_psnr / structural_similarity / VisualizeImage take images of at least 11 x 11 pixels (one SSIM window; the kernels
    measure both metrics in one pass).
"""
from pathlib import Path

import numpy as np
import torch

from . import database

__all__ = ['compute_psnr', 'structural_similarity', 'PSNR_SSIM', 'VisualizeImage', 'name2metrics', 'psnr_nr', 'psnr_nr_fine',
           'name2key_metrics']

PRED_SUFFIXES = ('nr', 'dr', 'nr_fine', 'dr_fine')      # network/metrics.py:63-76: nr, then compute_psnr_prefix's order
_ENGINES = {}


def _engine(device, engine=None):
    if engine is not None:
        return engine
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if device not in _ENGINES:
        from .engine import RenderEngine
        _ENGINES[device] = RenderEngine(device)          # (raises on a CPU device: the metrics run on the HIP kernels)
    return _ENGINES[device]


def _default_device():
    return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')


def _u8_image(img, name):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError('neuray_amd.metrics: %s must be a uint8 [h, w, 3] image (got %s %s)' % (name, img.dtype, img.shape))
    return img


def _pair_metrics(img_gt, img_pr, ssim, engine):
    gt, pr = _u8_image(img_gt, 'img_gt'), _u8_image(img_pr, 'img_pr')
    if gt.shape != pr.shape:
        raise ValueError('neuray_amd.metrics: image shapes differ: %s vs %s' % (gt.shape, pr.shape))
    eng = _engine(_default_device(), engine)
    h, w = gt.shape[:2]
    r = eng.image_metrics(torch.from_numpy(np.ascontiguousarray(pr))[None], torch.from_numpy(np.ascontiguousarray(gt))[None], h, w,
                          ssim=ssim)
    return torch.stack([r['psnr'], r['ssim']]).cpu().numpy()[:, 0]


def compute_psnr(img_gt, img_pr, use_vis_scores=False, vis_scores=None, vis_scores_thresh=1.5, engine=None):
    """network/metrics.py:14-28: PSNR of two uint8 [h, w, 3] images, 10 log10(255^2 / mean squared difference), as a float.
    The reference's quirk is kept: its use_vis_scores branch computes a masked mean squared error that the unconditional code
    after it overwrites - but the branch has already replaced img_gt / img_pr by their pixels with vis_scores >= vis_scores_thresh,
    so the value returned is the PSNR over those pixels (nan if there are none), not over the whole image.  Here the other pixels
    are zeroed in both images before the kernel's exact SSE, and the mean is taken over the selected ones."""
    if not use_vis_scores:
        return float(_pair_metrics(img_gt, img_pr, 'box11', engine)[0])
    gt, pr = _u8_image(img_gt, 'img_gt'), _u8_image(img_pr, 'img_pr')
    keep = (np.asarray(vis_scores) >= vis_scores_thresh).reshape(-1)
    gt, pr = gt.reshape(-1, 3).copy(), pr.reshape(-1, 3).copy()
    gt[~keep] = 0
    pr[~keep] = 0
    eng = _engine(_default_device(), engine)
    r = eng.image_metrics(torch.from_numpy(pr)[None], torch.from_numpy(gt)[None], img_gt.shape[0], img_gt.shape[1])
    sse = float(r['sse'].cpu()[0])
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(10 * np.log10(255.0 * 255.0 * 3 * int(keep.sum()) / np.float64(sse)))


def structural_similarity(im1, im2, win_size=11, multichannel=True, data_range=255, engine=None, **kwargs):
    """The one call of skimage.metrics.structural_similarity the reference makes (network/metrics.py:56,71):
    structural_similarity(gt, pr, win_size=11, multichannel=True, data_range=255) on uint8 [h, w, 3] images - 11 x 11 uniform
    window, sample covariance, mean over the valid positions, channel mean."""
    if win_size != 11 or multichannel is not True or data_range != 255 or kwargs:
        raise NotImplementedError('neuray_amd.metrics.structural_similarity supports only the reference call '
                                  'structural_similarity(im1, im2, win_size=11, multichannel=True, data_range=255)')
    return float(_pair_metrics(im1, im2, 'box11', engine)[1])


def _query_hw(data_pr, data_gt):
    info = data_gt['que_imgs_info'] if 'que_imgs_info' in data_gt else data_pr['que_imgs_info']
    h, w = info['imgs'].shape[2:]
    return int(h), int(w)


def _stack(data_pr, keys, h, w, device):
    return torch.stack([data_pr[k].detach().reshape(h * w, 3).to(device=device, dtype=torch.float32) for k in keys])


class PSNR_SSIM:
    """network/metrics.py:31-79: psnr_* / ssim_* (float32 CPU tensors of shape [1]) of pixel_colors_nr and, where present, _dr,
    _nr_fine, _dr_fine against pixel_colors_gt - one neuray_image_metrics launch for all of them against the broadcast ground truth
    (box11: skimage's structural_similarity), one device -> host read of the results."""
    default_cfg = {
        'eval_margin_ratio': 1.0,
    }

    def __init__(self, cfg, engine=None):
        self.keys = []
        self.cfg = {**self.default_cfg, **cfg}
        self.engine = engine

    def __call__(self, data_pr, data_gt, step, **kwargs):
        h, w = _query_hw(data_pr, data_gt)
        suffixes = ['nr'] + [s for s in PRED_SUFFIXES[1:] if f'pixel_colors_{s}' in data_pr]
        gt = data_pr['pixel_colors_gt']
        eng = _engine(gt.device, self.engine)
        preds = _stack(data_pr, ['pixel_colors_%s' % s for s in suffixes], h, w, eng.device)
        gt = gt.detach().reshape(1, h * w, 3).to(device=eng.device, dtype=torch.float32)
        h_margin = int(h * (1 - self.cfg['eval_margin_ratio'])) // 2
        w_margin = int(w * (1 - self.cfg['eval_margin_ratio'])) // 2
        r = eng.image_metrics(preds, gt, h, w, ssim='box11', roi=(h_margin, h - h_margin, w_margin, w - w_margin))
        vals = torch.stack([r['psnr'], r['ssim']]).cpu()
        outputs = {}
        for i, s in enumerate(suffixes):
            outputs[f'psnr_{s}'] = vals[0, i:i + 1].to(torch.float32)
            outputs[f'ssim_{s}'] = vals[1, i:i + 1].to(torch.float32)
        return outputs


def concat_images_list(*imgs):
    """utils/draw_utils.py:149-169 (horizontal): side by side, shorter images zero-padded at the bottom"""
    hmax = max(im.shape[0] for im in imgs)
    padded = [im if im.shape[0] == hmax else np.concatenate([im, np.zeros((hmax - im.shape[0],) + im.shape[1:], im.dtype)], 0)
              for im in imgs]
    return np.concatenate(padded, axis=1)


class VisualizeImage:
    """network/metrics.py:81-109: data/vis_val/{model_name}/step-{step}-index-{data_index}.png (h, w <= 64) or .jpg - pixel_colors_gt,
    _nr[, _dr, _nr_fine, _dr_fine] quantised by the metrics kernel (color_map_backward) and concatenated horizontally."""

    def __init__(self, cfg, engine=None):
        self.keys = []
        self.engine = engine

    def __call__(self, data_pr, data_gt, step, **kwargs):
        h, w = _query_hw(data_pr, data_gt)
        keys = ['pixel_colors_gt', 'pixel_colors_nr'] + ['pixel_colors_%s' % s for s in PRED_SUFFIXES[1:] if f'pixel_colors_{s}' in data_pr]
        eng = _engine(data_pr['pixel_colors_gt'].device, self.engine)
        imgs = _stack(data_pr, keys, h, w, eng.device)
        quant = torch.empty(len(keys), h, w, 3, dtype=torch.uint8, device=eng.device)
        eng.image_metrics(imgs, imgs[:1], h, w, quantised_out=quant)
        quant = quant.cpu().numpy()
        data_index = kwargs['data_index']
        model_name = kwargs['model_name']
        Path(f'data/vis_val/{model_name}').mkdir(exist_ok=True, parents=True)
        ext = 'png' if h <= 64 and w <= 64 else 'jpg'
        database.imsave(f'data/vis_val/{model_name}/step-{step}-index-{data_index}.{ext}', concat_images_list(*quant))
        return {}


name2metrics = {
    'psnr_ssim': PSNR_SSIM,
    'vis_img': VisualizeImage,
}


def psnr_nr(results):
    return np.mean(results['psnr_nr'])


def psnr_nr_fine(results):
    return np.mean(results['psnr_nr_fine'])


name2key_metrics = {
    'psnr_nr': psnr_nr,
    'psnr_nr_fine': psnr_nr_fine,
}
