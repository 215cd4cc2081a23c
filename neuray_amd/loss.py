"""Drop-in for the reference's network/loss.py: the training losses (cfg loss [render, depth] / [render, consist]) on the HIP
kernels of neuray_train_loss (csrc/nr_kernels_loss.h) - every term of one loss object in one forward and one backward launch.

Same names, `.keys`, call signature `(data_pr, data_gt, step, **kwargs)` and returned keys / shapes / dtype / device as the reference
module; every class takes an optional `engine=` (a RenderEngine; default: the product engine of the tensors' device, which must be
the GPU - there is no host fallback).  The reference's quirks are kept: ConsistencyLoss reads `use_ray_mask` and never applies the
mask, returns {} without `hit_prob_self`, and sends no gradient to hit_prob_nr[_fine]; RenderLoss multiplies a masked-out ray by 0 (a
non-finite colour under a zero mask still gives NaN); DepthLoss takes the int64 (row, col) depth_coords as (x, y) and returns
zeros([1]) without `true_depth`.

Differences: inputs must be float32 (TypeError otherwise); a ground truth, depth map or depth range that requires grad raises
NotImplementedError (the kernels differentiate the predictions only); the losses are once differentiable.

total_loss() restates the trainer's reduction (train/trainer.py:124-132) so that the mirror package and parallel.train_step have a
ready loss_fn.
"""
import torch

from .metrics import _engine
from .network.autograd import loss_call

__all__ = ['Loss', 'ConsistencyLoss', 'RenderLoss', 'DepthLoss', 'name2loss', 'total_loss']
REFERENCE_NAMES = ('Loss', 'ConsistencyLoss', 'RenderLoss', 'DepthLoss', 'name2loss')     # what network/loss.py defines


class Loss:
    def __init__(self, keys):
        """keys: the output keys of the dict (the reference's multi-GPU DummyLoss reads them)"""
        self.keys = keys

    def __call__(self, data_pr, data_gt, step, **kwargs):
        pass


class ConsistencyLoss(Loss):
    """network/loss.py:18-44: loss_prob[, loss_prob_fine], float32 [qn]"""
    default_cfg = {
        'use_ray_mask': False,
        'use_dr_loss': False,
        'use_dr_fine_loss': False,
        'use_nr_fine_loss': False,
    }

    def __init__(self, cfg, engine=None):
        self.cfg = {**self.default_cfg, **cfg}
        self.engine = engine
        super().__init__(['loss_prob', 'loss_prob_fine'])

    def __call__(self, data_pr, data_gt, step, **kwargs):
        if 'hit_prob_self' not in data_pr:
            return {}
        if self.cfg['use_ray_mask']:
            data_pr['ray_mask']                      # (read and never applied, as in the reference: loss.py:33-36)
        names = ['loss_prob']
        terms = [('consist', {}, data_pr['hit_prob_self'], data_pr['hit_prob_nr'], None, None, None)]
        if 'hit_prob_nr_fine' in data_pr:
            names.append('loss_prob_fine')
            terms.append(('consist', {}, data_pr['hit_prob_self_fine'], data_pr['hit_prob_nr_fine'], None, None, None))
        eng = _engine(data_pr['hit_prob_self'].device, self.engine)
        return dict(zip(names, loss_call(eng, terms)))


class RenderLoss(Loss):
    """network/loss.py:46-77: loss_rgb_nr[, _dr, _dr_fine, _nr_fine], float32 [b]"""
    default_cfg = {
        'use_ray_mask': True,
        'use_dr_loss': False,
        'use_dr_fine_loss': False,
        'use_nr_fine_loss': False,
    }

    def __init__(self, cfg, engine=None):
        self.cfg = {**self.default_cfg, **cfg}
        self.engine = engine
        super().__init__(['loss_rgb'])

    def __call__(self, data_pr, data_gt, step, **kwargs):
        rgb_gt = data_pr['pixel_colors_gt']          # b,rn,3
        mask = data_pr['ray_mask'] if self.cfg['use_ray_mask'] else None     # b,rn (bool: read as it is)
        suffixes = ['nr'] + [s for s in ('dr', 'dr_fine', 'nr_fine') if self.cfg[f'use_{s}_loss']]
        terms = [('render', {}, data_pr[f'pixel_colors_{s}'], rgb_gt, mask, None, None) for s in suffixes]
        eng = _engine(rgb_gt.device, self.engine)
        return dict(zip([f'loss_rgb_{s}' for s in suffixes], loss_call(eng, terms)))


class DepthLoss(Loss):
    """network/loss.py:79-132: loss_depth[, loss_depth_fine], float32 [rfn]; zeros([1]) without true_depth (no launch)"""
    default_cfg = {
        'depth_correct_thresh': 0.02,
        'depth_loss_type': 'l2',
        'depth_loss_l1_beta': 0.05,
    }

    def __init__(self, cfg, engine=None):
        super().__init__(['loss_depth'])
        self.cfg = {**self.default_cfg, **cfg}
        self.engine = engine
        if self.cfg['depth_loss_type'] not in ('l2', 'smooth_l1'):
            raise ValueError("neuray_amd.loss.DepthLoss: depth_loss_type %r (l2 or smooth_l1)" % (self.cfg['depth_loss_type'],))

    def __call__(self, data_pr, data_gt, step, **kwargs):
        info = data_gt['ref_imgs_info']
        if 'true_depth' not in info:
            return {'loss_depth': torch.zeros([1], dtype=torch.float32, device=data_pr['pixel_colors_nr'].device)}
        noisy = info['depth'] if data_gt['scene_name'].startswith('gso') else None
        opts = {'smooth_l1': self.cfg['depth_loss_type'] == 'smooth_l1', 'beta': self.cfg['depth_loss_l1_beta'],
                'thresh': self.cfg['depth_correct_thresh']}
        names = ['loss_depth'] + (['loss_depth_fine'] if 'depth_mean_fine' in data_pr else [])
        terms = [('depth', opts, data_pr['depth_mean' + n[len('loss_depth'):]], info['true_depth'], noisy, data_pr['depth_coords'],
                  info['depth_range']) for n in names]
        eng = _engine(data_pr['depth_mean'].device, self.engine)
        return dict(zip(names, loss_call(eng, terms)))


name2loss = {
    'render': RenderLoss,
    'depth': DepthLoss,
    'consist': ConsistencyLoss,
}


def total_loss(losses, data_pr, data_gt, step, **kwargs):
    """train/trainer.py:124-132: every loss object is called, and the step's loss is the sum over the keys that start with 'loss' of
    the key's mean.  -> (loss, log_info): log_info holds every returned key (the trainer logs them all)."""
    log_info = {}
    for loss in losses:
        log_info.update(loss(data_pr, data_gt, step, **kwargs))
    loss = 0
    for k, v in log_info.items():
        if k.startswith('loss'):
            loss = loss + torch.mean(v)
    return loss, log_info
