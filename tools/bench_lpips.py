"""Time LPIPS on the HIP kernels (neuray_amd/lpips.py) next to an eager PyTorch fp32 composition of the same network on the same GPU,
in the same process: full VGG16 widths, seeded random weights, 800 x 800 and 756 x 1008, one pair and one ground truth against four
predictions.  HIP events, the median of --reps runs after two warm-up runs.  Reports the end-to-end time of both, the time per layer
of both (every launch between its own pair of events, in a run of its own), and the difference of the two scores.
The kernels' names for `rocprofv3 --kernel-trace --stats`: nr::lpips_stem_kernel, nr::conv2d_x3_kernel<4, 2, *, true>,
nr::maxpool2x2_kernel, nr::lpips_head_tile_kernel, nr::lpips_head_reduce_kernel.
    python tools/bench_lpips.py [--reps 20] [--sizes 800x800 756x1008] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuray_amd.engine import RenderEngine                        # noqa: E402
from neuray_amd.lpips import BLOCKS, LPIPS, Weights               # noqa: E402

VGG = (64, 128, 256, 512, 512)


def random_weights(widths, seed):
    g = torch.Generator().manual_seed(seed)
    convs, cin = [], 3
    for width, count in zip(widths, BLOCKS):
        for _ in range(count):
            convs.append((torch.randn(width, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5, torch.randn(width, generator=g) * 0.05))
            cin = width
    return Weights(convs, [torch.rand(width, generator=g) * 0.1 for width in widths])


class Timer:
    """per-layer events: every step of a run between its own pair"""

    def __init__(self):
        self.rows = []

    def __call__(self, name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        self.rows.append((name, e0, e1))
        return r

    def ms(self):
        torch.cuda.synchronize()
        return [(n, a.elapsed_time(b)) for n, a, b in self.rows]


def layer_names():
    names = ['stem (scale + conv1_1)']
    for blk, count in enumerate(BLOCKS):
        if blk:
            names.append('pool%d' % blk)
        names += ['conv%d_%d' % (blk + 1, k + 1) for k in range(count) if (blk, k) != (0, 0)]
        names.append('head%d' % (blk + 1))
    return names


def ours_layers(m, img0, img1, timer):
    """the body of LPIPS.__call__ for one chunk, step by step"""
    eng, p = m.engine, img0.shape[0]
    a, b = m._buffers((p + img1.shape[0]) * m.weights.widths[0] * img0.shape[1] * img0.shape[2])
    batch = torch.cat([img0, img1]).contiguous()
    layers = eng.empty(p, 5, dtype=torch.float64)
    x = timer('stem (scale + conv1_1)', lambda: eng.lpips_stem(batch, m.weights.shift, m.weights.scale, m.stem_w, m.stem_b, out=a))
    other, cur, i = b, a, 0
    for blk, count in enumerate(BLOCKS):
        if blk:
            x = timer('pool%d' % blk, lambda: eng.maxpool2x2(x, out=other))
            cur, other = other, cur
        for k in range(count):
            if (blk, k) == (0, 0):
                continue
            x = timer('conv%d_%d' % (blk + 1, k + 1), lambda: eng.conv3x3_x3_relu(x, m.packs[i], m.biases[i], m.couts[i], pad=1, out=other))
            cur, other = other, cur
            i += 1
        timer('head%d' % (blk + 1), lambda: eng.lpips_head(x[:p], x[p:], m.lins[blk], out=layers, column=blk))
    return layers.sum(1)


class Eager:
    """the same network as eager PyTorch fp32 ops on the device"""

    def __init__(self, W, dev):
        self.convs = [(w.to(dev), b.to(dev)) for w, b in W.convs]
        self.lins = [l.to(dev).view(1, -1, 1, 1) for l in W.lins]
        self.shift = torch.tensor(W.shift, device=dev).view(1, 3, 1, 1)
        self.scale = torch.tensor(W.scale, device=dev).view(1, 3, 1, 1)

    def __call__(self, img0, img1, timer=None):
        t = timer if timer is not None else (lambda name, fn: fn())
        p = img0.shape[0]

        def stem():
            x = torch.cat([img0, img1]).to(torch.float32) / 255.0
            x = ((x * 2.0 - 1.0).permute(0, 3, 1, 2) - self.shift) / self.scale
            return F.relu(F.conv2d(x, *self.convs[0], padding=1))
        x = t('stem (scale + conv1_1)', stem)
        total, i = 0.0, 1
        for blk, count in enumerate(BLOCKS):
            if blk:
                x = t('pool%d' % blk, lambda: F.max_pool2d(x, 2, 2))
            for k in range(count):
                if (blk, k) == (0, 0):
                    continue
                x = t('conv%d_%d' % (blk + 1, k + 1), lambda: F.relu(F.conv2d(x, *self.convs[i], padding=1)))
                i += 1

            def head():
                f0, f1 = x[:p], x[p:]
                n0 = f0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10)
                n1 = f1 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + 1e-10)
                return (self.lins[blk] * (n0 - n1) ** 2).sum(1).mean((1, 2))
            total = total + t('head%d' % (blk + 1), head)
        return total


def event_ms(fn, reps):
    fn(); fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(float(np.median(ts)), 3), round(min(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', type=str, nargs='+', default=['800x800', '756x1008'])
    ap.add_argument('--json', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_lpips.py measures on the GPU; none is present')
    dev = torch.device('cuda', 0)
    eng = RenderEngine(dev)
    W = random_weights(VGG, 0)
    ours, eager = LPIPS(W, engine=eng), Eager(W, dev)
    out = {'widths': VGG, 'reps': args.reps, 'cases': []}
    g = torch.Generator().manual_seed(1)
    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        gt = torch.randint(0, 256, (1, h, w, 3), dtype=torch.uint8, generator=g)
        for n in (1, 4):
            noise = torch.randint(-12, 13, (n, h, w, 3), generator=g)
            pr = (gt.to(torch.int64) + noise).clamp(0, 255).to(torch.uint8).to(dev)
            gtd = gt.to(dev)
            case = {'hw': [h, w], 'predictions': n}
            case['ours_ms_median'], case['ours_ms_min'] = event_ms(lambda: ours(pr, gtd), args.reps)
            case['eager_ms_median'], case['eager_ms_min'] = event_ms(lambda: eager(pr, gtd), args.reps)
            a, b = ours(pr, gtd).cpu().numpy(), eager(pr, gtd).double().cpu().numpy()
            case['score_ours'], case['score_eager'] = a.tolist(), b.tolist()
            case['score_rel_diff_max'] = float(np.max(np.abs(a - b) / np.abs(a)))
            per = {}
            for name, fn in (('ours', lambda t: ours_layers(ours, pr, gtd, t)), ('eager', lambda t: eager(pr, gtd, t))):
                runs = []
                for _ in range(args.reps):
                    t = Timer()
                    fn(t)
                    runs.append(t.ms())
                per[name] = {nm: round(float(np.median([r[j][1] for r in runs])), 3) for j, (nm, _) in enumerate(runs[0])}
            case['layers_ms'] = [{'layer': nm, 'ours': per['ours'][nm], 'eager': per['eager'][nm]} for nm in layer_names()]
            out['cases'].append(case)
            print('%d x %d, %d prediction(s): ours %.2f ms, eager %.2f ms, scores differ by %.1e (relative)'
                  % (h, w, n, case['ours_ms_median'], case['eager_ms_median'], case['score_rel_diff_max']))
            for row in case['layers_ms']:
                print('    %-24s ours %8.3f ms   eager %8.3f ms' % (row['layer'], row['ours'], row['eager']))
            del pr
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != 'cases'}))


if __name__ == '__main__':
    main()
