"""LPIPS, the third number of eval.py (eval.py:16,24-27: lpips.LPIPS(net='vgg') on images scaled to [-1, 1]), on the HIP kernels:
neuray_lpips_stem (scaling layer + conv1_1), neuray_conv3x3_x3_relu (the other twelve convolutions, split-operand bf16 MFMA at fp32
grade), neuray_maxpool2x2 and neuray_lpips_head.  Inference only.  There is no host fallback and no other convolution library behind
it: one arithmetic everywhere, as in neuray_amd.metrics.

    from neuray_amd.lpips import LPIPS
    metric = LPIPS(('vgg16.pth', 'vgg.pth'))          # or a Weights object, or one path
    d = metric(img0, img1)                            # float64 device tensor [N]

The network is written from the published formula: five blocks of 2, 2, 3, 3, 3 convolutions (3 x 3, padding 1, ReLU), a 2 x 2 max
pool in front of blocks 2 to 5, a tap behind every block; per tap both feature maps are normalised over the channels, the squared
difference is weighted by `lin`, summed over the channels and averaged over the pixels; the score is the sum of the five terms.
The widths are read from the weights (VGG16: 64, 128, 256, 512, 512; any multiples of 32 work).

Weights are NOT part of this project and are never downloaded: load_weights() reads files the user names, in one of three layouts
  1. the full state_dict of lpips.LPIPS(net='vgg')                                   (one torch file)
  2. torchvision's vgg16 state_dict + the lpips package's weights/v0.1/vgg.pth        (two torch files, either order)
  3. the .npz that save_weights() writes                                              (one file)
The key names of layouts 1 and 2 are written down from the public packages AS REMEMBERED: neither package is available where this
project is developed, so they could not be checked against the real files.  The loader therefore matches keys by the small explicit
tables below and does not guess: on any missing or unexpected key it raises a KeyError that lists what it found and what it wanted.
If a real file is refused, that message shows which table entry to correct.

Memory: the pairs go through the network in chunks; the activations live in two ping-pong buffers sized for the first block (the
largest), a tap is handed to the head kernel as soon as it is complete and its buffer is reused by the next block.  Every tensor
handed to the convolution stays below its 2^31-byte limit.  A single ground truth compared with n predictions runs through the
network once per chunk (once in all when the n + 1 images fit one chunk - up to 5 predictions at 800 x 800).
"""
import os

import numpy as np
import torch

__all__ = ['LPIPS', 'Weights', 'load_weights', 'save_weights', 'BLOCKS', 'MIN_SIZE']

BLOCKS = (2, 2, 3, 3, 3)                       # convolutions per block
MIN_SIZE = 16                                  # four pools: the last tap is at least 1 x 1
SHIFT = (-.030, -.088, -.188)                  # the published scaling-layer constants
SCALE = (.458, .448, .450)
TV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # the convolutions inside torchvision's vgg16().features
_BLOCK_OF = tuple(b for b, k in enumerate(BLOCKS) for _ in range(k))

# ---- the explicit key tables (canonical name -> key in the file) ------------------------------------------------------------------
_CONV = ['conv%d.%s' % (i, p) for i in range(13) for p in ('weight', 'bias')]
_LIN = ['lin%d' % i for i in range(5)]
# 1. lpips.LPIPS(net='vgg').state_dict(): the features are re-wrapped as net.slice1 .. net.slice5, keeping torchvision's indices
FULL_REQUIRED = dict([('conv%d.%s' % (i, p), 'net.slice%d.%d.%s' % (_BLOCK_OF[i] + 1, TV_INDEX[i], p)) for i in range(13) for p in ('weight', 'bias')]
                     + [('lin%d' % i, 'lin%d.model.1.weight' % i) for i in range(5)])
FULL_OPTIONAL = dict([('shift', 'scaling_layer.shift'), ('scale', 'scaling_layer.scale')]
                     + [('lin%d.copy' % i, 'lins.%d.model.1.weight' % i) for i in range(5)])     # (newer releases also register the list)
# 2a. torchvision.models.vgg16().state_dict(); the classifier is not used
TV_REQUIRED = dict(('conv%d.%s' % (i, p), 'features.%d.%s' % (TV_INDEX[i], p)) for i in range(13) for p in ('weight', 'bias'))
TV_IGNORED = tuple('classifier.%d.%s' % (i, p) for i in (0, 3, 6) for p in ('weight', 'bias'))
# 2b. lpips/weights/v0.1/vgg.pth
LIN_REQUIRED = dict(('lin%d' % i, 'lin%d.model.1.weight' % i) for i in range(5))
# 3. save_weights(): the canonical names themselves
NPZ_REQUIRED = dict((k, k) for k in _CONV + _LIN + ['shift', 'scale'])


class Weights:
    """The network's parameters in canonical form: convs [(weight [co, ci, 3, 3], bias [co])] * 13, lins [[c]] * 5 (float32 CPU
    tensors), shift / scale (tuples of three floats)."""

    def __init__(self, convs, lins, shift=SHIFT, scale=SCALE, names=None):
        names = names or {}

        def name(k):
            return names.get(k, k)
        if len(convs) != 13 or len(lins) != 5:
            raise ValueError('neuray_amd.lpips: %d convolutions and %d linear layers (13 and 5)' % (len(convs), len(lins)))
        self.convs, self.lins = [], []
        cin, widths = 3, []
        for i, (w, b) in enumerate(convs):
            w, b = _f32(w, name('conv%d.weight' % i)), _f32(b, name('conv%d.bias' % i))
            first = i == 0 or _BLOCK_OF[i] != _BLOCK_OF[i - 1]
            if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[1] != cin or (not first and w.shape[0] != cin) or w.shape[0] % 32 or w.shape[0] < 32:
                raise ValueError('neuray_amd.lpips: %s has shape %s; wanted [%s, %d, 3, 3]'
                                 % (name('conv%d.weight' % i), tuple(w.shape), 'a multiple of 32' if first else str(cin), cin))
            if tuple(b.shape) != (w.shape[0],):
                raise ValueError('neuray_amd.lpips: %s has shape %s; wanted [%d]' % (name('conv%d.bias' % i), tuple(b.shape), w.shape[0]))
            cin = w.shape[0]
            if first:
                widths.append(cin)
            self.convs.append((w, b))
        for i, l in enumerate(lins):
            l = _f32(l, name('lin%d' % i))
            if l.numel() != widths[i] or tuple(l.shape) not in ((widths[i],), (1, widths[i], 1, 1)):
                raise ValueError('neuray_amd.lpips: %s has shape %s; wanted [1, %d, 1, 1]' % (name('lin%d' % i), tuple(l.shape), widths[i]))
            self.lins.append(l.reshape(-1).contiguous())
        self.widths = tuple(widths)
        self.shift, self.scale = _three(shift, name('shift')), _three(scale, name('scale'))
        if any(s == 0.0 for s in self.scale):
            raise ValueError('neuray_amd.lpips: %s has a zero entry' % name('scale'))


def _f32(x, name):
    x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).detach().cpu()
    if x.dtype != torch.float32:
        raise ValueError('neuray_amd.lpips: %s is %s; wanted float32' % (name, x.dtype))
    return x.contiguous()


def _three(x, name):
    v = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).reshape(-1)
    if v.size != 3:
        raise ValueError('neuray_amd.lpips: %s has %d entries; wanted 3' % (name, v.size))
    return tuple(float(np.float32(t)) for t in v)


def _select(found, required, optional=(), ignored=(), what=''):
    """-> {canonical: value} for the required and the present optional keys; KeyError unless `found` is exactly required + some of
    optional / ignored"""
    optional = dict(optional)
    missing = sorted(k for k in required.values() if k not in found)
    extra = sorted(k for k in found if k not in set(required.values()) | set(optional.values()) | set(ignored))
    if missing or extra:
        raise KeyError('neuray_amd.lpips: %s: missing keys %s, unexpected keys %s.  Found %s; wanted %s%s'
                       % (what, missing, extra, sorted(found), sorted(required.values()),
                          (' and optionally %s' % sorted(list(optional.values()) + list(ignored))) if optional or ignored else ''))
    out = {c: found[k] for c, k in required.items()}
    out.update({c: found[k] for c, k in optional.items() if k in found})
    return out


def _build(sel, names):
    for i in range(5):                               # the duplicate registration must say the same
        if 'lin%d.copy' % i in sel and not torch.equal(torch.as_tensor(sel['lin%d.copy' % i]), torch.as_tensor(sel['lin%d' % i])):
            raise ValueError('neuray_amd.lpips: %s and %s differ' % (names['lin%d.copy' % i], names['lin%d' % i]))
    return Weights([(sel['conv%d.weight' % i], sel['conv%d.bias' % i]) for i in range(13)], [sel['lin%d' % i] for i in range(5)],
                   sel.get('shift', SHIFT), sel.get('scale', SCALE), names)


def load_weights(*paths):
    """-> Weights from one of the three layouts of the module docstring.  torch files are read with
    torch.load(map_location='cpu', weights_only=True), .npz files with np.load(allow_pickle=False)."""
    if len(paths) == 1 and not isinstance(paths[0], (str, os.PathLike)):
        paths = tuple(paths[0])
    if not 1 <= len(paths) <= 2:
        raise ValueError('neuray_amd.lpips.load_weights: one file (a full LPIPS state_dict or an .npz) or two (vgg16 + the linear layers), got %d' % len(paths))
    files = []
    for p in paths:
        p = os.fspath(p)
        if p.endswith('.npz'):
            with np.load(p, allow_pickle=False) as z:
                files.append((p, 'npz', {k: z[k] for k in z.files}))
        else:
            sd = torch.load(p, map_location='cpu', weights_only=True)
            if not isinstance(sd, dict):
                raise ValueError('neuray_amd.lpips.load_weights: %s does not hold a state_dict' % p)
            kind = 'tv' if any(k.startswith('features.') for k in sd) else 'full' if any(k.startswith('net.') for k in sd) else 'lin'
            files.append((p, kind, dict(sd)))
    kinds = sorted(k for _, k, _ in files)
    if kinds == ['npz']:
        p, _, found = files[0]
        return _build(_select(found, NPZ_REQUIRED, what=p), {})
    if kinds == ['full']:
        p, _, found = files[0]
        return _build(_select(found, FULL_REQUIRED, FULL_OPTIONAL, what=p), {**FULL_REQUIRED, **FULL_OPTIONAL})
    if kinds == ['lin', 'tv']:
        by = {k: (p, found) for p, k, found in files}
        sel = _select(by['tv'][1], TV_REQUIRED, ignored=TV_IGNORED, what=by['tv'][0])
        sel.update(_select(by['lin'][1], LIN_REQUIRED, what=by['lin'][0]))
        return _build(sel, {**TV_REQUIRED, **LIN_REQUIRED})
    raise KeyError('neuray_amd.lpips.load_weights: %s are not one of the three layouts (a full LPIPS state_dict with net.slice*/lin* keys; '
                   'a vgg16 state_dict with features.* keys + the lin*.model.1.weight file; an .npz of save_weights).  Found: %s'
                   % (list(map(os.fspath, paths)), {p: sorted(f)[:6] for p, _, f in files}))


def save_weights(path, weights):
    """Layout 3: an .npz of conv{0..12}.weight / .bias, lin{0..4} [c], shift [3], scale [3] (float32)"""
    path = os.fspath(path)
    if not path.endswith('.npz'):
        raise ValueError('neuray_amd.lpips.save_weights: %s: the file name must end in .npz' % path)
    arrays = {}
    for i, (w, b) in enumerate(weights.convs):
        arrays['conv%d.weight' % i], arrays['conv%d.bias' % i] = w.numpy(), b.numpy()
    for i, l in enumerate(weights.lins):
        arrays['lin%d' % i] = l.numpy()
    arrays['shift'], arrays['scale'] = np.asarray(weights.shift, np.float32), np.asarray(weights.scale, np.float32)
    np.savez(path, **arrays)


CHUNK_BYTES = 1 << 30        # size of one activation buffer (below the convolution's 2^31-byte limit)


class LPIPS:
    """weights: a Weights object, a path or a sequence of paths (load_weights).  engine: a RenderEngine (default: the product engine
    of the GPU).  The weight packs of the convolutions are made once, here."""

    def __init__(self, weights, engine=None, device=None, chunk_bytes=CHUNK_BYTES):
        from .metrics import _engine
        if not isinstance(weights, Weights):
            weights = load_weights(weights) if isinstance(weights, (str, os.PathLike)) else load_weights(*weights)
        self.weights = weights
        self.engine = eng = _engine(device if device is not None else 'cuda', engine)
        self.chunk_bytes = int(chunk_bytes)
        if not 0 < self.chunk_bytes < (1 << 31) - 256:
            raise ValueError('neuray_amd.lpips: chunk_bytes must stay below 2^31')
        dev = eng.device
        self.stem_w, self.stem_b = (t.to(dev) for t in weights.convs[0])
        self.packs = [eng.conv3x3_x3_pack(w.to(dev)) for w, _ in weights.convs[1:]]
        self.biases = [b.to(dev) for _, b in weights.convs[1:]]
        self.couts = [w.shape[0] for w, _ in weights.convs[1:]]
        self.lins = [l.to(dev) for l in weights.lins]
        self._buf = None

    def _buffers(self, floats):
        if self._buf is None or self._buf[0].numel() < floats:
            self._buf = None                                     # (released before the larger pair is made)
            self._buf = (self.engine.empty(floats), self.engine.empty(floats))
        return self._buf

    def _images(self, img, name):
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.ascontiguousarray(img))
        if not torch.is_tensor(img) or img.dtype not in (torch.float32, torch.uint8):
            raise TypeError('neuray_amd.lpips: %s must be a float32 [N, 3, H, W] or uint8 [N, H, W, 3] tensor (got %s)'
                            % (name, img.dtype if hasattr(img, 'dtype') else type(img)))
        ok = img.dim() == 4 and img.shape[0] >= 1 and img.shape[3 if img.dtype == torch.uint8 else 1] == 3
        if not ok:
            raise ValueError('neuray_amd.lpips: %s has shape %s; wanted %s' % (name, tuple(img.shape), '[N, H, W, 3]' if img.dtype == torch.uint8 else '[N, 3, H, W]'))
        return img.detach()

    def __call__(self, img0, img1, return_layers=False):
        """img0, img1: float32 [N, 3, H, W] in [-1, 1] or uint8 [N, H, W, 3], both of one dtype and size; either may have batch 1 (one
        ground truth against N images).  -> float64 device tensor [N]; with return_layers also the five per-tap terms [N, 5]."""
        eng = self.engine
        img0, img1 = self._images(img0, 'img0'), self._images(img1, 'img1')
        if img0.dtype != img1.dtype:
            raise TypeError('neuray_amd.lpips: img0 is %s, img1 %s' % (img0.dtype, img1.dtype))
        if img0.shape[0] == 1 and img1.shape[0] > 1:
            img0, img1 = img1, img0                              # (the value is symmetric, bit for bit)
        if tuple(img0.shape[1:]) != tuple(img1.shape[1:]) or img1.shape[0] not in (1, img0.shape[0]):
            raise ValueError('neuray_amd.lpips: image shapes differ: %s vs %s' % (tuple(img0.shape), tuple(img1.shape)))
        u8 = img0.dtype == torch.uint8
        n = img0.shape[0]
        h, w = (img0.shape[1], img0.shape[2]) if u8 else (img0.shape[2], img0.shape[3])
        if h < MIN_SIZE or w < MIN_SIZE:
            raise ValueError('neuray_amd.lpips: images of %d x %d; the smallest size is %d x %d' % (h, w, MIN_SIZE, MIN_SIZE))
        shared = img1.shape[0] == 1 and n > 1
        per_image = self.weights.widths[0] * h * w * 4
        room = self.chunk_bytes // per_image                      # images per buffer
        if room < 2:
            raise ValueError('neuray_amd.lpips: a pair of %d x %d images does not fit the activation buffers (%d bytes each)' % (h, w, self.chunk_bytes))
        step = min(n, room - 1 if shared else room // 2)
        a, b = self._buffers((step + (1 if shared else step)) * per_image // 4)
        img0, img1 = img0.to(eng.device), img1.to(eng.device)
        layers = eng.empty(n, 5, dtype=torch.float64)
        for k in range(0, n, step):
            e = min(n, k + step)
            p = e - k
            x = eng.lpips_stem(torch.cat([img0[k:e], img1 if shared else img1[k:e]]).contiguous(), self.weights.shift, self.weights.scale,
                               self.stem_w, self.stem_b, out=a)
            cur, other = a, b
            i = 0                                                # index into the twelve packed convolutions
            for blk, count in enumerate(BLOCKS):
                if blk:
                    x = eng.maxpool2x2(x, out=other)
                    cur, other = other, cur
                for _ in range(count - (blk == 0)):
                    x = eng.conv3x3_x3_relu(x, self.packs[i], self.biases[i], self.couts[i], pad=1, out=other)
                    cur, other = other, cur
                    i += 1
                eng.lpips_head(x[:p], x[p:], self.lins[blk], out=layers[k:e], column=blk)      # (the tap's buffer is free after this)
        score = layers[:, 0]
        for t in range(1, 5):
            score = score + layers[:, t]                         # tap order
        return (score, layers) if return_layers else score
