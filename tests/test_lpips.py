"""LPIPS on the HIP kernels (csrc/nr_kernels_lpips.h + the ReLU instantiation of csrc/nr_kernels_conv2d.h; neuray_amd/lpips.py) against a
float64 PyTorch composition of the published formula on the CPU: F.conv2d(padding=1), relu, max_pool2d(2, 2), normalise over the
channels, squared difference, weight by lin, sum over the channels, mean over the pixels; the score is the sum of the five taps.
Weights are seeded random ones (He-scaled convolutions, small biases, lin = rand * 0.1; one case with a few negative lin entries) -
no real weight file exists in this project.  Inputs are smooth colour fields quantised to uint8; the second image of a pair is the
first plus uniform noise of 0.3, 0.05, 0.01 or 0.004 of full scale, quantised again.

Accuracy gate.  The kernels claim fp32 grade, so the yardstick is the distance of an fp32 eager composition of the same network from
the float64 one on the same inputs, computed here next to it: per tap term and for the total
    |ours - f64| <= max(4 |eager32 - f64|, floor |f64|)
with the factor 4 of tests/test_conv2d_x3.py and floor = 2e-5 for noise >= 0.05, 1e-4 for noise < 0.05 (seven / five times the worst
fp32-eager error measured on the CPU for those noise levels; the error grows as the images approach each other because the head
differences two nearly equal normalised vectors).  Stem alone: 3e-6 of the largest output (the gate of test_conv2d_x3).  Head alone:
1e-9 relative - its channel sums are fp64.

The emulator runs the thin network (widths 32, 32, 64, 64, 64) at 32 x 32, 37 x 50, 48 x 33, 33 x 47 and 16 x 16; the MI355X the same
and the full VGG16 widths at 96 x 128, 75 x 101 and one 400 x 600 pair.  Every case prints the errors it saw before it asserts.
The emulator leg of this file takes about six minutes on 16 CPU threads (the thin network at these sizes is what it can afford)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from emu_util import emu_lib

BACKENDS = ['emu', pytest.param('hip', marks=pytest.mark.gpu)]
HIP_ONLY = [pytest.param('hip', marks=pytest.mark.gpu)]
THIN, VGG = (32, 32, 64, 64, 64), (64, 128, 256, 512, 512)
NOISES = (0.3, 0.05, 0.01, 0.004)
THIN_SIZES = [(32, 32), (37, 50), (48, 33), (33, 47), (16, 16)]


def engine(backend):
    from neuray_amd.engine import RenderEngine
    return RenderEngine('cpu', _test_lib=emu_lib()) if backend == 'emu' else RenderEngine('cuda:0')


# ---- seeded weights and inputs -------------------------------------------------------------------------------------------------
def random_weights(widths, seed, negative_lin=False):
    from neuray_amd.lpips import BLOCKS, Weights
    g = torch.Generator().manual_seed(seed)
    convs, cin = [], 3
    for width, count in zip(widths, BLOCKS):
        for _ in range(count):
            w = torch.randn(width, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5          # He
            convs.append((w, torch.randn(width, generator=g) * 0.05))
            cin = width
    lins = [torch.rand(width, generator=g) * 0.1 for width in widths]
    if negative_lin:
        for l in lins:
            l[::11] *= -0.5
    return Weights(convs, lins)


def smooth_u8(rng, h, w):
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
    f = rng.rand(3, 3)
    img = np.stack([0.5 + 0.45 * np.sin(2 * np.pi * (1.5 * f[c, 0] * xx + 1.5 * f[c, 1] * yy) + 6 * f[c, 2]) for c in range(3)], -1)
    return np.clip(np.rint(img * 255), 0, 255).astype(np.uint8)


def noisy_u8(rng, img, level):
    return np.clip(np.rint(img.astype(np.float64) + (rng.rand(*img.shape) * 2 - 1) * level * 255), 0, 255).astype(np.uint8)


def to_f32(u8):
    """eval.py's arithmetic in fp32: u8 / 255, then * 2 - 1; NHWC -> NCHW"""
    x = torch.from_numpy(np.ascontiguousarray(u8)).to(torch.float32) / 255.0
    return (x * 2.0 - 1.0).permute(0, 3, 1, 2).contiguous()


# ---- oracle ---------------------------------------------------------------------------------------------------------------------
def features(W, x, dtype):
    from neuray_amd.lpips import BLOCKS
    x = x.to(dtype)
    x = (x - torch.tensor(W.shift, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(W.scale, dtype=dtype).view(1, 3, 1, 1)
    taps, i = [], 0
    for blk, count in enumerate(BLOCKS):
        if blk:
            x = F.max_pool2d(x, 2, 2)
        for _ in range(count):
            w, b = W.convs[i]
            x = F.relu(F.conv2d(x, w.to(dtype), b.to(dtype), padding=1))
            i += 1
        taps.append(x)
    return taps


def head(f0, f1, lin):
    n0 = f0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + 1e-10)
    return (lin.to(f0.dtype).view(1, -1, 1, 1) * (n0 - n1) ** 2).sum(1).mean((1, 2))


def oracle(W, x0, x1, dtype):
    """x0 [n, 3, h, w], x1 [1 or n, 3, h, w] fp32 in [-1, 1] -> layers [n, 5] (float64 numpy)"""
    t0, t1 = features(W, x0, dtype), features(W, x1, dtype)
    return torch.stack([head(a, b, l) for a, b, l in zip(t0, t1, W.lins)], 1).double().numpy()


def check_accuracy(tag, got_layers, got_score, W, x0, x1, noises):
    f64, f32 = oracle(W, x0, x1, torch.float64), oracle(W, x0, x1, torch.float32)
    got_layers, got_score = got_layers.cpu().numpy(), got_score.cpu().numpy()
    ours = np.concatenate([got_layers, got_score[:, None]], 1)
    want = np.concatenate([f64, f64.sum(1, keepdims=True)], 1)
    eager = np.concatenate([f32, f32.sum(1, keepdims=True)], 1)
    bad = []
    for i, noise in enumerate(noises):
        floor = 2e-5 if noise >= 0.05 else 1e-4
        err, ref = np.abs(ours[i] - want[i]), np.abs(eager[i] - want[i])
        gate = np.maximum(4 * ref, floor * np.abs(want[i]))
        print('%s noise %.3f  score %.6f  rel err ours %s | eager32 %s' % (
            tag, noise, want[i, 5], ' '.join('%.1e' % v for v in err / np.abs(want[i])), ' '.join('%.1e' % v for v in ref / np.abs(want[i]))))
        if (err > gate).any():
            bad.append((noise, err.tolist(), gate.tolist()))
    assert not bad, bad


def pairs(seed, h, w):
    rng = np.random.RandomState(seed)
    a = smooth_u8(rng, h, w)
    return a[None], np.stack([noisy_u8(rng, a, lv) for lv in NOISES])


# ---- the whole metric -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', THIN_SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('backend', BACKENDS)
def test_thin_network_against_float64(backend, size):
    from neuray_amd.lpips import LPIPS
    h, w = size
    W = random_weights(THIN, 10 + h, negative_lin=(size == (37, 50)))
    gt, pr = pairs(h * 100 + w, h, w)
    m = LPIPS(W, engine=engine(backend))
    score, layers = m(torch.from_numpy(pr), torch.from_numpy(gt), return_layers=True)
    assert score.dtype == torch.float64 and tuple(score.shape) == (4,) and tuple(layers.shape) == (4, 5)
    check_accuracy('thin %dx%d %s' % (h, w, backend), layers, score, W, to_f32(pr), to_f32(gt), NOISES)


@pytest.mark.parametrize('size', [(96, 128), (75, 101)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('backend', HIP_ONLY)
def test_vgg16_widths_against_float64(backend, size):
    from neuray_amd.lpips import LPIPS
    h, w = size
    W = random_weights(VGG, 20 + h)
    gt, pr = pairs(h * 100 + w, h, w)
    m = LPIPS(W, engine=engine(backend))
    score, layers = m(torch.from_numpy(pr), torch.from_numpy(gt), return_layers=True)
    check_accuracy('vgg16 %dx%d %s' % (h, w, backend), layers, score, W, to_f32(pr), to_f32(gt), NOISES)


@pytest.mark.parametrize('backend', HIP_ONLY)
def test_vgg16_widths_at_400x600(backend):
    from neuray_amd.lpips import LPIPS
    W = random_weights(VGG, 31)
    rng = np.random.RandomState(32)
    a = smooth_u8(rng, 400, 600)
    b = noisy_u8(rng, a, 0.05)
    score, layers = LPIPS(W, engine=engine(backend))(torch.from_numpy(a[None]), torch.from_numpy(b[None]), return_layers=True)
    check_accuracy('vgg16 400x600 %s' % backend, layers, score, W, to_f32(a[None]), to_f32(b[None]), (0.05,))


# ---- the kernels alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_stem_against_float64(backend):
    eng = engine(backend)
    W = random_weights(THIN if backend == 'emu' else VGG, 40)
    rng = np.random.RandomState(41)
    u8 = np.stack([smooth_u8(rng, 21, 35), rng.randint(0, 256, (21, 35, 3)).astype(np.uint8)])
    w, b = W.convs[0]
    x = to_f32(u8).double()
    x = (x - torch.tensor(W.shift, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(W.scale, dtype=torch.float64).view(1, 3, 1, 1)
    want = F.relu(F.conv2d(x, w.double(), b.double(), padding=1))
    for inp in (torch.from_numpy(u8), to_f32(u8)):
        got = eng.lpips_stem(inp.to(eng.device), W.shift, W.scale, w.to(eng.device), b.to(eng.device)).cpu()
        err = float((got.double() - want).abs().max() / want.abs().max())
        print('stem %s %s: max err / max output %.2e' % (backend, inp.dtype, err))
        assert tuple(got.shape) == tuple(want.shape) and err <= 3e-6


@pytest.mark.parametrize('backend', BACKENDS)
def test_head_against_float64(backend):
    """several tiles and a partial one (37 x 29 = 1073 pixels), pixels whose features are all zero, negative lin entries, a shared f1"""
    eng = engine(backend)
    g = torch.Generator().manual_seed(50)
    f0 = F.relu(torch.randn(3, 64, 37, 29, generator=g))
    f1 = F.relu(f0 + 0.02 * torch.randn(3, 64, 37, 29, generator=g))
    f0[:, :, 5, 7] = 0
    f1[:, :, 5, 7] = 0
    f1[1, :, 9, 9] = 0
    lin = torch.rand(64, generator=g) * 0.1
    lin[::9] *= -0.5
    for other in (f1, f1[:1].contiguous()):
        got = eng.lpips_head(f0.to(eng.device), other.to(eng.device), lin.to(eng.device)).cpu().numpy()
        want = head(f0.double(), other.double(), lin).numpy()
        err = np.abs(got - want) / np.abs(want)
        print('head %s: relative errors %s' % (backend, err))
        assert (err <= 1e-9).all()
    out = torch.full((3, 5), -1.0, dtype=torch.float64, device=eng.device)
    eng.lpips_head(f0.to(eng.device), f1.to(eng.device), lin.to(eng.device), out=out, column=3)
    assert (out[:, [0, 1, 2, 4]] == -1).all() and out[:, 3].cpu().numpy().tobytes() == eng.lpips_head(
        f0.to(eng.device), f1.to(eng.device), lin.to(eng.device)).cpu().numpy().tobytes()


@pytest.mark.parametrize('backend', BACKENDS)
def test_maxpool_and_relu_epilogue_are_exact(backend):
    eng = engine(backend)
    g = torch.Generator().manual_seed(60)
    for h, w in ((16, 16), (21, 35), (2, 3)):
        x = torch.randn(2, 5, h, w, generator=g)
        got = eng.maxpool2x2(x.to(eng.device)).cpu()
        assert torch.equal(got, F.max_pool2d(x, 2, 2))
    x = torch.randn(2, 32, 13, 19, generator=g).to(eng.device)
    wgt, bias = torch.randn(64, 32, 3, 3, generator=g).to(eng.device) * 0.1, torch.randn(64, generator=g).to(eng.device)
    pack = eng.conv3x3_x3_pack(wgt)
    plain = eng.conv3x3_x3(x, pack, bias, 64, pad=1)
    assert torch.equal(eng.conv3x3_x3_relu(x, pack, bias, 64, pad=1), torch.relu(plain)) and bool((plain < 0).any())
    ws = torch.empty(2 * 64 * 13 * 19 + 7, device=eng.device)
    assert torch.equal(eng.conv3x3_x3_relu(x, pack, bias, 64, pad=1, out=ws), torch.relu(plain))


# ---- bitwise properties ---------------------------------------------------------------------------------------------------------
def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize('backend', BACKENDS)
def test_uint8_input_equals_the_fp32_input_of_eval_py(backend):
    from neuray_amd.lpips import LPIPS
    m = LPIPS(random_weights(THIN, 70), engine=engine(backend))
    gt, pr = pairs(71, 20, 27)
    a, la = m(torch.from_numpy(pr[:2]), torch.from_numpy(gt), return_layers=True)
    b, lb = m(to_f32(pr[:2]), to_f32(gt), return_layers=True)
    assert _bytes(a) == _bytes(b) and _bytes(la) == _bytes(lb)


@pytest.mark.parametrize('backend', BACKENDS)
def test_batching_chunking_and_repetition_do_not_change_a_bit(backend):
    """one ground truth against n predictions = n separate calls; a pair inside a batch of 3 = the pair alone; a second run = the first;
    small activation buffers (several chunks) = one chunk"""
    from neuray_amd.lpips import LPIPS
    eng = engine(backend)
    W = random_weights(THIN, 80)
    m = LPIPS(W, engine=eng)
    gt, pr = pairs(81, 19, 24)
    pr, gt3 = torch.from_numpy(pr[:3]), torch.from_numpy(np.stack([gt[0], pr[3], pr[0]]))
    shared, ls = m(pr, torch.from_numpy(gt), return_layers=True)
    assert _bytes(m(pr, torch.from_numpy(gt))) == _bytes(shared)
    for i in range(3):
        one, lo = m(pr[i:i + 1], torch.from_numpy(gt), return_layers=True)
        assert _bytes(one) == _bytes(shared[i:i + 1]) and _bytes(lo) == _bytes(ls[i:i + 1])
    batch = m(pr, gt3)
    assert _bytes(m(pr[1:2], gt3[1:2])) == _bytes(batch[1:2])
    assert _bytes(batch[:1]) == _bytes(shared[:1])
    small = LPIPS(W, engine=eng, chunk_bytes=2 * 32 * 19 * 24 * 4)         # two images per buffer: one pair per chunk
    assert _bytes(small(pr, torch.from_numpy(gt))) == _bytes(shared) and _bytes(small(pr, gt3)) == _bytes(batch)


@pytest.mark.parametrize('backend', BACKENDS)
def test_identical_images_score_zero_and_the_metric_is_symmetric(backend):
    from neuray_amd.lpips import LPIPS
    m = LPIPS(random_weights(THIN, 90, negative_lin=True), engine=engine(backend))
    gt, pr = pairs(91, 17, 22)
    a, b = torch.from_numpy(np.repeat(gt, 2, 0)), torch.from_numpy(pr[2:4])
    zero, lz = m(a, a.clone(), return_layers=True)
    assert (zero == 0.0).all() and (lz == 0.0).all()
    ab, lab = m(a, b, return_layers=True)
    ba, lba = m(b, a, return_layers=True)
    assert _bytes(ab) == _bytes(ba) and _bytes(lab) == _bytes(lba) and (ab != 0).all()


# ---- weights --------------------------------------------------------------------------------------------------------------------
def _layouts(W, tmp_path):
    """the three layouts of one weight set as files -> {name: paths}, and the two torch dicts"""
    from neuray_amd import lpips
    full, tv, lin = {}, {}, {}
    for i, (w, b) in enumerate(W.convs):
        for name, t in (('weight', w), ('bias', b)):
            full[lpips.FULL_REQUIRED['conv%d.%s' % (i, name)]] = t.clone()
            tv[lpips.TV_REQUIRED['conv%d.%s' % (i, name)]] = t.clone()
    for i, l in enumerate(W.lins):
        full['lin%d.model.1.weight' % i] = l.clone().view(1, -1, 1, 1)
        lin['lin%d.model.1.weight' % i] = l.clone().view(1, -1, 1, 1)
    full['scaling_layer.shift'] = torch.tensor(W.shift).view(1, 3, 1, 1)
    full['scaling_layer.scale'] = torch.tensor(W.scale).view(1, 3, 1, 1)
    tv['classifier.0.weight'] = torch.zeros(4, 4)
    paths = {k: str(tmp_path / ('%s.pth' % k)) for k in ('full', 'tv', 'lin')}
    for k, d in (('full', full), ('tv', tv), ('lin', lin)):
        torch.save(d, paths[k])
    paths['npz'] = str(tmp_path / 'w.npz')
    lpips.save_weights(paths['npz'], W)
    return paths, full, tv, lin


def test_layout_tables_name_the_published_keys():
    from neuray_amd import lpips
    assert [lpips.TV_REQUIRED['conv%d.weight' % i] for i in range(13)] == [
        'features.%d.weight' % k for k in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)]
    assert lpips.FULL_REQUIRED['conv0.weight'] == 'net.slice1.0.weight' and lpips.FULL_REQUIRED['conv12.bias'] == 'net.slice5.28.bias'
    assert lpips.FULL_REQUIRED['conv4.weight'] == 'net.slice3.10.weight' and lpips.LIN_REQUIRED['lin4'] == 'lin4.model.1.weight'
    assert lpips.SHIFT == (-.030, -.088, -.188) and lpips.SCALE == (.458, .448, .450)


@pytest.mark.parametrize('backend', BACKENDS)
def test_three_weight_layouts_give_equal_packs_and_scores(backend, tmp_path):
    from neuray_amd.lpips import LPIPS, load_weights
    eng = engine(backend)
    W = random_weights(THIN, 100)
    paths, _, _, _ = _layouts(W, tmp_path)
    gt, pr = pairs(101, 16, 18)
    ref = LPIPS(W, engine=eng)
    want = _bytes(ref(torch.from_numpy(pr[:2]), torch.from_numpy(gt)))
    for src in ((paths['full'],), (paths['tv'], paths['lin']), (paths['lin'], paths['tv']), (paths['npz'],)):
        loaded = load_weights(*src)
        assert loaded.widths == THIN and loaded.shift == W.shift and loaded.scale == W.scale
        m = LPIPS(src if len(src) > 1 else src[0], engine=eng)
        assert all(_bytes(a) == _bytes(b) for a, b in zip(m.packs, ref.packs)) and len(m.packs) == 12
        assert _bytes(m.stem_w) == _bytes(ref.stem_w) and all(_bytes(a) == _bytes(b) for a, b in zip(m.lins, ref.lins))
        assert _bytes(m(torch.from_numpy(pr[:2]), torch.from_numpy(gt))) == want


def test_loader_refuses_missing_extra_and_misshapen_keys(tmp_path):
    from neuray_amd.lpips import load_weights
    W = random_weights(THIN, 110)
    paths, full, tv, lin = _layouts(W, tmp_path)
    bad = str(tmp_path / 'bad.pth')

    def saved(d):
        torch.save(d, bad)
        return bad
    d = dict(full)
    del d['net.slice3.12.bias']
    with pytest.raises(KeyError, match=r'net\.slice3\.12\.bias'):
        load_weights(saved(d))
    with pytest.raises(KeyError, match=r'net\.slice9\.1\.weight'):
        load_weights(saved(dict(full, **{'net.slice9.1.weight': torch.zeros(1)})))
    d = dict(tv)
    del d['features.28.weight']
    with pytest.raises(KeyError, match=r'features\.28\.weight'):
        load_weights(saved(d), paths['lin'])
    with pytest.raises(KeyError, match=r'lin5\.model\.1\.weight'):
        load_weights(paths['tv'], saved(dict(lin, **{'lin5.model.1.weight': torch.zeros(1, 64, 1, 1)})))
    with pytest.raises(ValueError, match=r'net\.slice2\.7\.weight'):
        load_weights(saved(dict(full, **{'net.slice2.7.weight': torch.zeros(32, 16, 3, 3)})))
    with pytest.raises(ValueError, match=r'lin2\.model\.1\.weight'):
        load_weights(paths['tv'], saved(dict(lin, **{'lin2.model.1.weight': torch.zeros(1, 32, 1, 1)})))
    with pytest.raises((KeyError, ValueError)):
        load_weights(paths['tv'])                                  # the linear layers are missing
    with pytest.raises((KeyError, ValueError)):
        load_weights(paths['tv'], paths['full'])
    z = dict(np.load(paths['npz']))
    del z['lin3']
    np.savez(str(tmp_path / 'bad.npz'), **z)
    with pytest.raises(KeyError, match='lin3'):
        load_weights(str(tmp_path / 'bad.npz'))
    d = dict(full)
    del d['scaling_layer.shift'], d['scaling_layer.scale']       # optional: the published constants are the default
    assert load_weights(saved(d)).shift == tuple(float(np.float32(v)) for v in (-.030, -.088, -.188))


@pytest.mark.parametrize('backend', BACKENDS)
def test_bad_inputs_raise(backend):
    from neuray_amd.lpips import LPIPS
    m = LPIPS(random_weights(THIN, 120), engine=engine(backend))
    u8 = lambda n, h, w: torch.zeros(n, h, w, 3, dtype=torch.uint8)      # noqa: E731
    with pytest.raises(ValueError, match='smallest size'):
        m(u8(1, 15, 40), u8(1, 15, 40))
    with pytest.raises(ValueError, match='smallest size'):
        m(torch.zeros(1, 3, 16, 12), torch.zeros(1, 3, 16, 12))
    with pytest.raises(ValueError, match='shapes differ'):
        m(u8(1, 16, 17), u8(1, 17, 16))
    with pytest.raises(ValueError, match='shapes differ'):
        m(u8(3, 16, 16), u8(2, 16, 16))
    with pytest.raises(TypeError):
        m(torch.zeros(1, 3, 16, 16, dtype=torch.float64), torch.zeros(1, 3, 16, 16, dtype=torch.float64))
    with pytest.raises(TypeError):
        m(u8(1, 16, 16), torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, 3))          # fp32 must be NCHW
    with pytest.raises(ValueError, match='does not fit'):
        LPIPS(m.weights, engine=m.engine, chunk_bytes=32 * 16 * 16 * 4)(u8(1, 16, 16), u8(1, 16, 16))


def test_lpips_without_an_engine_needs_the_gpu():
    """no host fallback: on a CPU device the metric asks for the HIP engine, which refuses it"""
    from neuray_amd.lpips import LPIPS
    with pytest.raises(RuntimeError, match='HIP device'):
        LPIPS(random_weights(THIN, 130), device='cpu')
