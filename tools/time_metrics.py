"""Time the image-metrics kernels (csrc/nr_kernels_metrics.h, neuray_image_metrics) on the GPU (HIP events):
  psnr_ssim      neuray_amd.metrics.PSNR_SSIM at 800 x 800 with four predictions (nr, dr, nr_fine, dr_fine) + the ground truth:
                 the whole call (stacking the predictions, the two kernels, the one device -> host read), and the launch alone
  gauss11_u8     RenderEngine.image_metrics(ssim='gauss11') on a batch of 8 uint8 800 x 800 images (eval.py's variant)
  host stand-in  the float64 scipy oracle of tests/test_metrics.py (box11) on the four predictions + the device -> host copies of the
                 five images (wall clock; skimage itself is not installed, so this only stands in for the reference's host path)
The kernels' names are printed for `rocprofv3 --kernel-trace --stats`.
    python tools/time_metrics.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from neuray_amd import metrics                                    # noqa: E402
from neuray_amd.engine import RenderEngine                        # noqa: E402

KERNELS = ('nr::image_metrics_tile_kernel<false>  (box11)', 'nr::image_metrics_tile_kernel<true>  (gauss11)',
           'nr::image_metrics_reduce_kernel')


def event_ms(fn, reps):
    fn(); fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(float(np.median(ts)), 4), round(min(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--hw', type=int, nargs=2, default=[800, 800])
    args = ap.parse_args()
    h, w = args.hw
    dev = torch.device('cuda', 0)
    eng = RenderEngine(dev)
    g = torch.Generator(device='cpu').manual_seed(0)
    gt = torch.rand(1, h * w, 3, generator=g)
    data = {'pixel_colors_gt': gt.to(dev), 'que_imgs_info': {'imgs': torch.zeros(1, 3, h, w, device=dev)}}
    for i, s in enumerate(('nr', 'dr', 'nr_fine', 'dr_fine')):
        data['pixel_colors_%s' % s] = (gt + 0.05 * (i + 1) * torch.randn(1, h * w, 3, generator=g)).to(dev)
    out = {'hw': [h, w], 'kernels': KERNELS}
    ps = metrics.PSNR_SSIM({}, engine=eng)
    out['psnr_ssim_call_ms_median'], out['psnr_ssim_call_ms_min'] = event_ms(lambda: ps(data, {}, 0), args.reps)
    preds = torch.cat([data['pixel_colors_%s' % s] for s in ('nr', 'dr', 'nr_fine', 'dr_fine')])
    out['psnr_ssim_launch_ms_median'], out['psnr_ssim_launch_ms_min'] = event_ms(
        lambda: eng.image_metrics(preds, data['pixel_colors_gt'], h, w, ssim='box11'), args.reps)
    u8 = torch.randint(0, 256, (8, h, w, 3), dtype=torch.uint8, generator=g).to(dev)
    u8gt = torch.randint(0, 256, (8, h, w, 3), dtype=torch.uint8, generator=g).to(dev)
    out['gauss11_u8x8_ms_median'], out['gauss11_u8x8_ms_min'] = event_ms(
        lambda: eng.image_metrics(u8, u8gt, h, w, ssim='gauss11'), args.reps)
    out['box11_u8x8_ms_median'], out['box11_u8x8_ms_min'] = event_ms(
        lambda: eng.image_metrics(u8, u8gt, h, w, ssim='box11'), args.reps)

    # host stand-in: the float64 oracle of the tests on the four predictions, after copying the five images to the host
    from test_metrics import quantise, ssim_box11
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = [data[k].cpu().numpy().reshape(h, w, 3) for k in ('pixel_colors_gt', 'pixel_colors_nr', 'pixel_colors_dr',
                                                             'pixel_colors_nr_fine', 'pixel_colors_dr_fine')]
    q = [quantise(x) for x in host]
    for p in q[1:]:
        ssim_box11(q[0], p)
        ((q[0].astype(np.int64) - p) ** 2).sum()
    out['host_oracle_standin_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
