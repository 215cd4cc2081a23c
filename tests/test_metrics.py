"""Image metrics on the HIP kernels (csrc/nr_kernels_metrics.h, neuray_image_metrics, RenderEngine.image_metrics) against a float64
numpy / scipy oracle written from the definitions (network/metrics.py: color_map_backward + skimage structural_similarity(win_size=11,
data_range=255); eval.py: tf.image.ssim):
  box11   scipy.ndimage.uniform_filter(size=11), sample covariance (121 / 120), 5 pixels cropped from each side, channel mean
  gauss11 an explicit separable VALID correlation with the normalised 1-D Gaussian (sigma 1.5), biased moments, luminance x cs
SSE must equal the int64 numpy SSE exactly, SSIM the oracle within 1e-9.  Emulator on small shapes, the MI355X at 800 x 800."""
import numpy as np
import pytest
import torch
from scipy.ndimage import uniform_filter

from emu_util import emu_lib

BACKENDS = ['emu', pytest.param('hip', marks=pytest.mark.gpu)]
VARIANTS = ['box11', 'gauss11']
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


# ---- oracle ---------------------------------------------------------------------------------------------------------------------
def quantise(x):
    """utils/base_utils.py:496-499 color_map_backward on float32"""
    with np.errstate(invalid='ignore', over='ignore'):
        return np.clip(np.asarray(x, np.float32) * np.float32(255), 0, 255).astype(np.uint8)


def ssim_box11(gt, pr):
    vals = []
    for c in range(3):
        x, y = gt[..., c].astype(np.float64), pr[..., c].astype(np.float64)
        f = lambda a: uniform_filter(a, size=11)       # noqa: E731
        ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
        cov = 121.0 / 120.0
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        s = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        vals.append(s[5:-5, 5:-5].mean())
    return float(np.mean(vals))


def gauss_taps():
    d = np.arange(11) - 5.0
    g = np.exp(-0.5 * d * d / 1.5 ** 2)
    return g / g.sum()


def ssim_gauss11(gt, pr):
    g = gauss_taps()

    def filt(a):
        h, w = a.shape
        r = sum(g[k] * a[:, k:w - 10 + k] for k in range(11))
        return sum(g[k] * r[k:h - 10 + k] for k in range(11))
    vals = []
    for c in range(3):
        x, y = gt[..., c].astype(np.float64), pr[..., c].astype(np.float64)
        mx, my, mxx, myy, mxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
        num0, den0 = mx * my * 2, mx * mx + my * my
        lum = (num0 + C1) / (den0 + C1)
        cs = (mxy * 2 - num0 + C2) / (mxx + myy - den0 + C2)
        vals.append((lum * cs).mean())
    return float(np.mean(vals))


ORACLE = {'box11': ssim_box11, 'gauss11': ssim_gauss11}


def sse(gt, pr):
    return int(((gt.astype(np.int64) - pr.astype(np.int64)) ** 2).sum())


def psnr(s, pixels):
    with np.errstate(divide='ignore'):
        return 10 * np.log10(255.0 ** 2 * 3 * pixels / np.float64(s))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def smooth_noise(rng, n, h, w):
    """float32 [n, h*w, 3]: smooth colour fields + noise, saturated and negative values, a sprinkle of +-inf and NaN"""
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
    out = []
    for _ in range(n):
        f = rng.rand(3, 3)
        base = np.stack([0.5 + 0.6 * np.sin(2 * np.pi * (f[c, 0] * xx + f[c, 1] * yy) + 6 * f[c, 2]) for c in range(3)], -1)
        img = (base + 0.05 * rng.randn(h, w, 3)).astype(np.float32)
        spots = rng.rand(h, w, 3)
        img[spots < 0.003] = np.inf
        img[(spots >= 0.003) & (spots < 0.006)] = -np.inf
        img[(spots >= 0.006) & (spots < 0.009)] = np.nan
        out.append(img.reshape(h * w, 3))
    return np.stack(out)


def engine(backend):
    from neuray_amd.engine import RenderEngine
    return RenderEngine('cpu', _test_lib=emu_lib()) if backend == 'emu' else RenderEngine('cuda:0')


def run(eng, pred, gt, h, w, **kw):
    r = eng.image_metrics(torch.from_numpy(np.ascontiguousarray(pred)), torch.from_numpy(np.ascontiguousarray(gt)), h, w, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def check(r, gts, prs, variant, pixels):
    """gts / prs: uint8 [n, h, w, 3] (the ROI)"""
    for i in range(len(prs)):
        s = sse(gts[i], prs[i])
        assert int(r['sse'][i]) == s, i
        want = psnr(s, pixels)
        assert (np.isinf(want) and np.isinf(r['psnr'][i])) or abs(r['psnr'][i] - want) <= 1e-12 * abs(want), (i, r['psnr'][i], want)
        o = ORACLE[variant](gts[i], prs[i])
        assert abs(r['ssim'][i] - o) <= 1e-9, (i, variant, r['ssim'][i], o)


SHAPE = {'emu': (37, 90), 'hip': (800, 800)}


# ---- tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('backend', BACKENDS)
def test_float_predictions_against_a_broadcast_ground_truth(backend, variant):
    """PSNR_SSIM's shape: four float predictions (with saturated / negative / +-inf / NaN entries) against one ground truth"""
    h, w = SHAPE[backend]
    rng = np.random.RandomState(1)
    gt = smooth_noise(rng, 1, h, w)
    pred = np.clip(gt + 0.08 * rng.randn(4, h * w, 3).astype(np.float32), -0.2, 1.2)
    pred[1, : h * w // 3] = gt[0, : h * w // 3]                     # partly identical
    pred[3] = smooth_noise(rng, 1, h, w)[0]
    r = run(engine(backend), pred, gt, h, w, ssim=variant)
    g = quantise(gt).reshape(1, h, w, 3)
    check(r, np.repeat(g, 4, 0), quantise(pred).reshape(4, h, w, 3), variant, h * w)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('backend', BACKENDS)
def test_small_constant_and_identical_images(backend, variant):
    """one window (11 x 11), one window row (11 x 300), constant images, identical inputs (SSIM 1, PSNR inf)"""
    eng = engine(backend)
    rng = np.random.RandomState(2)
    for h, w in ((11, 11), (11, 300), (300, 11) if backend == 'hip' else (23, 11)):
        gt = rng.randint(0, 256, (1, h, w, 3)).astype(np.uint8)
        prs = np.stack([gt[0], np.full((h, w, 3), 77, np.uint8), np.clip(gt[0].astype(int) + rng.randint(-9, 10, (h, w, 3)), 0, 255),
                        np.full((h, w, 3), 255, np.uint8)]).astype(np.uint8)
        r = run(eng, prs, gt, h, w, ssim=variant)
        check(r, np.repeat(gt, 4, 0), prs, variant, h * w)
        if variant == 'box11':
            assert r['ssim'][0] == 1.0
        else:
            assert abs(r['ssim'][0] - 1.0) <= 1e-15
        assert np.isinf(r['psnr'][0]) and r['sse'][0] == 0
        const = np.full((2, h, w, 3), 200, np.uint8)
        const[1] = 13
        rc = run(eng, const, const, h, w, ssim=variant)
        check(rc, const, const, variant, h * w)
        assert (rc['sse'] == 0).all()
        rc = run(eng, const[1:], const[:1], h, w, ssim=variant)       # two different constants: luminance only
        check(rc, const[:1], const[1:], variant, h * w)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('backend', BACKENDS)
def test_region_of_interest_from_eval_margin_ratio(backend, variant):
    """PSNR_SSIM's crop (eval_margin_ratio 0.8): valid windows and SSE pixels are counted inside the ROI only"""
    h, w = SHAPE[backend] if backend == 'hip' else (41, 67)
    rng = np.random.RandomState(3)
    gt = smooth_noise(rng, 1, h, w)
    pred = smooth_noise(rng, 2, h, w)
    hm, wm = int(h * (1 - 0.8)) // 2, int(w * (1 - 0.8)) // 2
    r = run(engine(backend), pred, gt, h, w, ssim=variant, roi=(hm, h - hm, wm, w - wm))
    g = quantise(gt).reshape(1, h, w, 3)[:, hm:h - hm, wm:w - wm]
    p = quantise(pred).reshape(2, h, w, 3)[:, hm:h - hm, wm:w - wm]
    check(r, np.repeat(g, 2, 0), p, variant, (h - 2 * hm) * (w - 2 * wm))


@pytest.mark.parametrize('backend', BACKENDS)
def test_quantised_output_is_color_map_backward(backend):
    """the fused load quantises exactly as np.clip(x * np.float32(255), 0, 255).astype(np.uint8): 1 ulp either side of k / 255,
    negatives, values above 1, +-inf, NaN"""
    k = np.arange(256, dtype=np.float32)
    q = k / np.float32(255)
    vals = np.concatenate([q, np.nextafter(q, np.float32(np.inf)), np.nextafter(q, np.float32(-np.inf)),
                           np.array([-0.0, -1e-30, -0.5, -1e30, 1.0000001, 1.5, 3e38, np.inf, -np.inf, np.nan, 1e-45, 0.99999994],
                                    np.float32)]).astype(np.float32)
    h, w = 16, 40
    rng = np.random.RandomState(4)
    pad = rng.rand(3 * h * w - vals.size).astype(np.float32)
    x = np.concatenate([vals, pad]).reshape(1, h * w, 3)
    y = rng.permutation(x.reshape(-1)).reshape(1, h * w, 3)
    pred = np.concatenate([x, y])
    eng = engine(backend)
    out = torch.zeros(2, h, w, 3, dtype=torch.uint8, device=eng.device)
    r = run(eng, pred, x, h, w, quantised_out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), quantise(pred).reshape(2, h, w, 3))
    check(r, np.repeat(quantise(x).reshape(1, h, w, 3), 2, 0), quantise(pred).reshape(2, h, w, 3), 'box11', h * w)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('backend', BACKENDS)
def test_bitwise_deterministic_and_independent_of_the_batch(backend, variant):
    h, w = (37, 90) if backend == 'emu' else (800, 800)
    rng = np.random.RandomState(5)
    gt = smooth_noise(rng, 1, h, w)
    pred = smooth_noise(rng, 5, h, w)
    eng = engine(backend)
    a = run(eng, pred, gt, h, w, ssim=variant)
    b = run(eng, pred, gt, h, w, ssim=variant)
    for key in ('sse', 'ssim', 'psnr'):
        assert a[key].tobytes() == b[key].tobytes(), key
    for i in (0, 3):
        one = run(eng, pred[i:i + 1], gt, h, w, ssim=variant)
        for key in ('sse', 'ssim', 'psnr'):
            assert one[key].tobytes() == a[key][i:i + 1].tobytes(), (i, key)
    copies = run(eng, pred, np.repeat(gt, 5, 0), h, w, ssim=variant)       # explicit ground truth per pair (stride 1)
    for key in ('sse', 'ssim', 'psnr'):
        assert copies[key].tobytes() == a[key].tobytes(), key


@pytest.mark.parametrize('backend', BACKENDS)
def test_float_and_uint8_inputs_agree_and_small_regions_raise(backend):
    h, w = 30, 52
    rng = np.random.RandomState(6)
    gt, pred = smooth_noise(rng, 1, h, w), smooth_noise(rng, 2, h, w)
    eng = engine(backend)
    for variant in VARIANTS:
        f = run(eng, pred, gt, h, w, ssim=variant)
        u = run(eng, quantise(pred).reshape(2, h, w, 3), quantise(gt).reshape(1, h, w, 3), h, w, ssim=variant)
        for key in ('sse', 'ssim', 'psnr'):
            assert f[key].tobytes() == u[key].tobytes(), (variant, key)
    with pytest.raises(RuntimeError, match='smaller than the 11 x 11'):
        run(eng, pred, gt, h, w, roi=(0, 10, 0, w))
    with pytest.raises(RuntimeError, match='smaller than the 11 x 11'):
        run(eng, pred, gt, h, w, roi=(3, h, 20, 30))
    small = np.zeros((1, 10 * 40, 3), np.float32)
    with pytest.raises(RuntimeError, match='smaller than the 11 x 11'):
        run(eng, small, small, 10, 40)
    with pytest.raises(RuntimeError, match='not inside'):
        run(eng, pred, gt, h, w, roi=(0, h + 1, 0, w))
    with pytest.raises(TypeError):
        run(eng, pred.astype(np.float64), gt.astype(np.float64), h, w)


def test_metrics_without_an_engine_need_the_gpu():
    """no host fallback: on a CPU tensor the drop-in asks for the HIP engine, which refuses a CPU device"""
    from neuray_amd import metrics
    data = {'pixel_colors_gt': torch.zeros(1, 400, 3), 'pixel_colors_nr': torch.zeros(1, 400, 3),
            'que_imgs_info': {'imgs': torch.zeros(1, 3, 20, 20)}}
    with pytest.raises(RuntimeError, match='HIP device'):
        metrics.PSNR_SSIM({})(data, {}, 0)
