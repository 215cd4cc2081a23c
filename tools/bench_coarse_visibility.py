"""What cfg['hip_coarse_pass'] = 'visibility' buys on the bench workload.

    python tools/bench_coarse_visibility.py [--reps 20] [--warmup 3]

bench.py's image (synthetic.make_scene, 800 x 800, 8 reference views, 64 coarse + 32 fine samples, 65 536-ray launches), rendered in one
process in 'network' mode (the parent code path: the aggregation network on the coarse and on the fine samples) and in 'visibility' mode
(the visibility kernels place the fine samples, the network runs on them only), for cfg['hip_arith'] = 'x3' and 'f32'.  Per mode and
arithmetic: the whole image (HIP events around render(), median of --reps after --warmup) and the coarse pass alone (the kernel durations
of the coarse launches of an image - point + ray kernel against vis_points + vis_rays - summed per image, median of --reps images).  The PSNR
between the two modes' images is printed as information only: seeded random weights carry no meaningful visibility.  One JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuray_amd import synthetic  # noqa: E402
from neuray_amd.network.renderer import NeuralRayBaseRenderer  # noqa: E402

H = W = 800
RFN, DN_COARSE, DN_FINE, RAY_BATCH = 8, 64, 32, 65536
COARSE_KERNELS = {'network': ('points', 'rays'), 'visibility': ('vis_points', 'vis_rays')}


def build(device, arith, mode):
    cfg = {'use_hierarchical_sampling': True, 'dist_decoder_cfg': {'use_vis': False}, 'depth_sample_num': DN_COARSE,
           'fine_depth_sample_num': DN_FINE, 'agg_net_cfg': {'sample_num': DN_COARSE}, 'fine_agg_net_cfg': {'sample_num': DN_FINE},
           'ray_batch_num': RAY_BATCH, 'hip_arith': arith, 'hip_coarse_pass': mode}
    torch.manual_seed(0)
    return NeuralRayBaseRenderer(cfg).eval().to(device)


def render(renderer, tq, tr):
    with torch.no_grad():        # fresh dicts: the per-image constants and relayouts are part of the image, as in bench.py
        return renderer.render(dict(tq), {k: v for k, v in tr.items() if not k.startswith('_')}, False)


def measure(renderer, mode, tq, tr, device, warmup, reps):
    for _ in range(warmup):
        out = render(renderer, tq, tr)
    torch.cuda.synchronize(device)
    image_ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(device))
        out = render(renderer, tq, tr)
        e1.record(torch.cuda.current_stream(device))
        e1.synchronize()
        image_ms.append(e0.elapsed_time(e1))
    # the coarse launches of an image: the kernels whose launch covers rays x DN_COARSE sample points
    eng = renderer.engine(device)
    coarse_ms, parts = [], {k: [] for k in COARSE_KERNELS[mode]}
    for _ in range(reps):
        eng.timing = []
        render(renderer, tq, tr)
        torch.cuda.synchronize(device)
        timing, eng.timing = eng.timing, None
        rays = H * W
        sizes = {min(RAY_BATCH, rays - b) * DN_COARSE for b in range(0, rays, RAY_BATCH)}
        per = {k: sum(e0.elapsed_time(e1) for name, e0, e1, n in timing if name == k and n in sizes) for k in COARSE_KERNELS[mode]}
        assert all(sum(1 for name, _, _, n in timing if name == k and n in sizes) == -(-rays // RAY_BATCH) for k in per), 'coarse launches'
        coarse_ms.append(sum(per.values()))
        for k, v in per.items():
            parts[k].append(v)
    med = statistics.median(image_ms)
    return {'image_ms': med, 'image_ms_min': min(image_ms), 'rays_per_s': H * W / (med * 1e-3),
            'coarse_pass_ms': statistics.median(coarse_ms),
            'coarse_kernels_ms': {k: statistics.median(v) for k, v in parts.items()}}, out['pixel_colors_nr_fine']


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float('inf') if mse == 0.0 else -10.0 * math.log10(mse)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    os.environ.pop('NEURAY_HIP_COARSE', None)
    os.environ.pop('NEURAY_HIP_ARITH', None)
    device = torch.device('cuda:0')
    que, ref = synthetic.make_scene(H, W, RFN, seed=0)
    que['coords'] = synthetic.meshgrid_coords(H, W)
    tq = {k: torch.from_numpy(v).to(device) for k, v in que.items()}
    tr = {k: torch.from_numpy(v).to(device) for k, v in ref.items()}
    line = {'workload': '%dx%d, %d views, %d + %d samples, %d-ray launches' % (H, W, RFN, DN_COARSE, DN_FINE, RAY_BATCH),
            'policy': 'one process, %d warm-up images, median of %d by HIP events' % (args.warmup, args.reps),
            'device': torch.cuda.get_device_name(device)}
    for arith in ('x3', 'f32'):
        res, imgs = {}, {}
        for mode in ('network', 'visibility'):
            res[mode], imgs[mode] = measure(build(device, arith, mode), mode, tq, tr, device, args.warmup, args.reps)
        res['image_speedup'] = res['network']['image_ms'] / res['visibility']['image_ms']
        res['coarse_pass_speedup'] = res['network']['coarse_pass_ms'] / res['visibility']['coarse_pass_ms']
        res['psnr_between_modes_db_informational'] = psnr(imgs['network'], imgs['visibility'])
        line[arith] = res
    print(json.dumps(line))


if __name__ == '__main__':
    main()
