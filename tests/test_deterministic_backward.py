"""The deterministic training backward (cfg['hip_deterministic']): the backward kernels without float atomics.

  1. neuray_reduce_partials adds the workgroups' rows in ascending order: bit for bit a NumPy float32 loop;
  2. the deterministic map scatter (interpolate_feats_backward(deterministic=True)) adds every texel's contributions in ascending
     (point, tap 00, 10, 01, 11) order: bit for bit a NumPy float32 loop, and within 1e-6 of the largest entry of a float64 index_add_;
  3. the gradients are still right: the gates of test_backward.py / test_direct_rendering_backward.py with the mode on;
  4. the same step three times gives bitwise the same gradients (a toy with every map texel contended, and the training shape);
  5. (tests/test_deterministic_norm.py: the fused norm's statistics)
  6. the switch: environment over cfg, 'auto', the grafted reference class, refusals, and nothing of the mode when it is off."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, load_weights
from emu_util import emu_lib, emu_lib_bf16x3
from oracle import torch_eager_port as tep
from test_backward import BACKENDS, _pass_case
from neuray_amd import _lib, synthetic
from neuray_amd.engine import RenderEngine
from neuray_amd.network import fused_norm
from neuray_amd.network.renderer import NeuralRayBaseRenderer


def _dev(backend):
    return 'cpu' if backend == 'emu' else 'cuda:0'


def _engine(backend):
    return RenderEngine(_dev(backend), _test_lib=emu_lib() if backend == 'emu' else None)


@pytest.fixture(autouse=True)
def _switch_off(monkeypatch):
    """every test starts and ends with the mode's process-wide switches off"""
    monkeypatch.delenv('NEURAY_HIP_DETERMINISTIC', raising=False)
    fused_norm.DETERMINISTIC = fused_norm.RENDERER_DETERMINISTIC = False
    yield
    fused_norm.DETERMINISTIC = fused_norm.RENDERER_DETERMINISTIC = False


# ---- 1. the order contract of the reduction -------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('g', [1, 7, 256])
@pytest.mark.parametrize('n', [1, 1000, 'FLAT_PASS_FLOATS'])
def test_reduce_partials_adds_the_rows_in_ascending_order(g, n, backend):
    eng = _engine(backend)
    n = int(eng.lib.neuray_flat_pass_floats()) if n == 'FLAT_PASS_FLOATS' else n
    rng = np.random.RandomState(1000 * g + n % 997)
    # normals scaled over six decades: a float32 sum in any other order differs in the last bits
    part = (rng.randn(g, n) * 10.0 ** rng.uniform(-3, 3, size=(g, n))).astype(np.float32)
    out0 = rng.randn(n).astype(np.float32)
    want = part[0].copy()
    for r in range(1, g):
        want = want + part[r]                       # float32 adds, row after row
    want = out0 + want
    if g >= 7 and n >= 1000:                        # (the inputs do tell orders apart)
        assert not np.array_equal(want, out0 + part[::-1].sum(0, dtype=np.float32))
    out = torch.from_numpy(out0.copy()).to(_dev(backend))
    eng.reduce_partials(torch.from_numpy(part).to(_dev(backend)), out)
    assert np.array_equal(out.cpu().numpy(), want)


# ---- 2. the order contract of the scatter -----------------------------------------------------------------------------------------
def _texel_coord_align(p, size):
    """nr_device.h texel_coord with align_corners on a full-resolution map, in float32 step by step"""
    f = np.float32
    n = f(f(f(p) / f(f(size) - f(1))) * f(2)) - f(1)
    ix = f(f(f(n + f(1)) / f(2)) * f(f(size) - f(1)))
    return min(f(f(size) - f(1)), max(ix, f(0)))


def _taps(ix, iy, mw, mh):
    """nr_device.h taps_from -> [(texel, weight)] in the order 00, 10, 01, 11"""
    f = np.float32
    x0f, y0f = np.floor(ix), np.floor(iy)
    x0, y0 = int(x0f), int(y0f)
    x1, yb = min(x0 + 1, mw - 1), min(y0 + 1, mh - 1)
    wx1, wy1 = f(ix - x0f), f(iy - y0f)
    wx0, wy0 = f(f(x0f + f(1)) - ix), f(f(y0f + f(1)) - iy)
    w = [f(wx0 * wy0), f(wx1 * wy0), f(wx0 * wy1), f(wx1 * wy1)]
    if x0 + 1 > mw - 1:
        w[1] = w[3] = f(0)
    if y0 + 1 > mh - 1:
        w[2] = w[3] = f(0)
    return list(zip([y0 * mw + x0, y0 * mw + x1, yb * mw + x0, yb * mw + x1], w))


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('c', [32, 3])
def test_deterministic_scatter_adds_in_point_then_tap_order(c, with_mask, backend):
    b, fh, fw, n = 2, 5, 7, 300
    rng = np.random.RandomState(10 * c + with_mask)
    # multiples of 0.25 inside the map and on its borders (the last row / column: coinciding taps, weight 0)
    pts = np.stack([rng.randint(0, 4 * (fw - 1) + 1, size=(b, n)), rng.randint(0, 4 * (fh - 1) + 1, size=(b, n))], -1).astype(np.float32) * 0.25
    pts[:, :8] = [[fw - 1, fh - 1], [0, 0], [fw - 1, 0.25], [0.5, fh - 1], [fw - 1, fh - 1], [3.0, 2.0], [fw - 1.25, fh - 1], [0, fh - 1]]
    d_out = (rng.randn(b, n, c) * 10.0 ** rng.uniform(-2, 2, size=(b, n, c))).astype(np.float32)
    mask = (rng.rand(b, n) > 0.25).astype(np.float32) if with_mask else None
    base = rng.randn(b, c, fh, fw).astype(np.float32)              # the call ADDS into its output

    want = np.zeros((b, fh * fw, c), np.float32)
    want64 = torch.zeros(b, fh * fw, c, dtype=torch.float64)
    touched = np.zeros((b, fh * fw), bool)
    runs = np.zeros((b, fh * fw), int)
    for bi in range(b):
        for i in range(n):
            mk = np.float32(1.0) if mask is None else mask[bi, i]
            if mk == 0.0:
                continue
            g = d_out[bi, i] * mk                                                   # float32
            taps = _taps(_texel_coord_align(pts[bi, i, 0], fw), _texel_coord_align(pts[bi, i, 1], fh), fw, fh)
            for tex, w in taps:
                if w != 0.0:
                    want[bi, tex] = want[bi, tex] + w * g                             # float32: one product, one add
                    want64[bi].index_add_(0, torch.tensor([tex]), torch.from_numpy((np.float64(w) * g.astype(np.float64)))[None])
                    touched[bi, tex] = True
                    runs[bi, tex] += 1
    assert runs.max() >= 20 and touched.all()
    want = np.where(touched[..., None], base.reshape(b, c, -1).transpose(0, 2, 1) + want, base.reshape(b, c, -1).transpose(0, 2, 1))

    eng, dev = _engine(backend), _dev(backend)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)            # noqa: E731
    before = eng.det_scratch_bytes
    got = eng.interpolate_feats_backward(t(d_out), (b, c, fh, fw), t(pts), fh, fw, align_corners=True, mask=t(mask) if with_mask else None,
                                         out=t(base.copy()), deterministic=True)
    assert eng.det_scratch_bytes > before
    got = got.cpu().numpy().reshape(b, c, -1).transpose(0, 2, 1)
    assert np.array_equal(got, want)
    ref64 = want64.numpy() + base.reshape(b, c, -1).transpose(0, 2, 1).astype(np.float64)
    err = float(np.abs(got - ref64).max())
    print('deterministic scatter against float64 index_add_ [c=%d, mask=%s, %s]: %.3e of %.3e' % (c, with_mask, backend, err, np.abs(ref64).max()))
    assert err <= 1e-6 * float(np.abs(ref64).max())
    # and the atomic path computes the same function
    plain = eng.interpolate_feats_backward(t(d_out), (b, c, fh, fw), t(pts), fh, fw, align_corners=True, mask=t(mask) if with_mask else None,
                                           out=t(base.copy()))
    assert float(np.abs(plain.cpu().numpy().reshape(b, c, -1).transpose(0, 2, 1) - ref64).max()) <= 1e-5 * float(np.abs(ref64).max())


# ---- 3. the gradients are still right ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('rfn,rn,dn,vis_head', [(3, 5, 8, False), (8, 3, 6, True), (2, 4, 5, False), (1, 3, 5, False),
                                                  (7, 2, 4, True), (5, 7, 9, True)])
def test_deterministic_pass_backward_matches_autograd(rfn, rn, dn, vis_head, backend):
    """test_backward.test_pass_backward_matches_autograd with deterministic=True, at that test's gate: 2e-3 of the largest entry against
    autograd of the eager port"""
    from oracle import neuray_oracle as orc
    dev, eng = _dev(backend), _engine(backend)
    que, ref, weights, rng = _pass_case(rfn, rn, dn, vis_head, seed=40 + rfn)
    lw_pix = rng.randn(rn, 3).astype(np.float32)
    lw_hit = rng.randn(rn, dn).astype(np.float32)
    depth = orc.sample_depth(que['depth_range'], rn, dn)
    depth = (depth * (1.0 + 0.02 * rng.rand(1, rn, dn))).astype(np.float32)
    depth.sort(-1)

    w = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in weights.items() if k.startswith(('dist_decoder.', 'agg_net.'))}
    tq = {k: torch.from_numpy(v) for k, v in que.items()}
    tr = {k: torch.from_numpy(v.copy()) for k, v in ref.items()}
    tr['ray_feats'].requires_grad_(True)
    tr['img_feats'].requires_grad_(True)
    out = tep.render_pass(w, {'coarse_use_vis': vis_head, 'fine_use_vis': True}, torch.from_numpy(depth), tq, tr, False)
    ((out['pixel_colors_nr'][0] * torch.from_numpy(lw_pix)).sum() + (out['hit_prob_nr'][0] * torch.from_numpy(lw_hit)).sum()).backward()

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)            # noqa: E731
    views = eng.prepare_views({k: t(v) for k, v in ref.items()})
    qc = eng.prepare_query({k: t(v) for k, v in que.items()})
    packed = eng.pack_pass(weights, 'dist_decoder.', 'agg_net.')
    fwd = eng.render_pass(qc, views, t(que['coords'][0]), t(depth[0]), packed, use_vis=vis_head)
    d_rec, g_ray = eng.render_rays_backward(fwd['point_rec'], t(depth[0]), packed, t(lw_pix), t(lw_hit), deterministic=True)
    flat, has_vis = eng.flat_pass(weights, 'dist_decoder.', 'agg_net.')
    d_flat, d_rf, d_if = eng.render_points_backward(qc, views, t(que['coords'][0]), t(depth[0]), flat, has_vis, vis_head, d_rec,
                                                    deterministic=True)
    grads = eng.unflatten_pass_grads(d_flat, weights, 'dist_decoder.', 'agg_net.')
    for name, g in g_ray.items():
        grads['agg_net.agg_impl.' + name] = g

    def close(got, want, name, rel=2e-3):
        want = want.detach().numpy() if torch.is_tensor(want) else want
        got = got.detach().cpu().numpy()
        tol = rel * max(1e-3, float(np.abs(want).max()))
        assert got.shape == want.shape, name
        assert np.abs(got - want).max() <= tol, (name, float(np.abs(got - want).max()), float(np.abs(want).max()))

    for k, p_ in w.items():
        close(grads[k], p_.grad if p_.grad is not None else torch.zeros_like(p_), k)
    close(d_rf.permute(0, 3, 1, 2), tr['ray_feats'].grad, 'ray_feats')
    close(d_if.permute(0, 3, 1, 2), tr['img_feats'].grad, 'img_feats')


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('variant', ['fp32', 'bf16x3'])
def test_deterministic_training_gradients_match_reference_autograd(variant, backend):
    """tests/golden/case_g_grads.npz (the reference's own autograd of render_impl(is_train=True)) through a renderer with
    cfg['hip_deterministic'] = True, at the golden's own gate of test_backward.test_training_gradients_match_reference_autograd: 5e-3.
    'bf16x3': the split library carries the same backward kernels (test_bf16x3_variant's gate is the same 5e-3): the mode runs there too."""
    z = np.load(os.path.join(GOLDEN_DIR, 'case_g_grads.npz'))
    cfg = ast.literal_eval(str(z['cfg_json']))
    dev = _dev(backend)
    r = NeuralRayBaseRenderer({**cfg, 'hip_deterministic': True, 'hip_variant': variant})
    r.load_state_dict({k: torch.from_numpy(v) for k, v in load_weights(False).items()}, strict=True)
    r.train()
    if backend == 'emu':
        r._engine_test_lib = emu_lib() if variant == 'fp32' else emu_lib_bf16x3()
    r = r.to(dev)
    assert r.engine(dev).variant == variant
    que = {k[4:]: torch.from_numpy(z[k]).to(dev) for k in z.files if k.startswith('que.') and k != 'que.Ks_inv'}
    ref = {k[4:]: torch.from_numpy(z[k]).to(dev) for k in z.files if k.startswith('ref.')}
    for t_ in (ref['ray_feats'], ref['img_feats'], que['ray_feats']):
        t_.requires_grad_(True)
    torch.manual_seed(4321)
    out = r.render_impl(que, ref, True)
    assert r.engine(dev).det_scratch_bytes == 0                       # (the forward is the forward)
    keys = ('pixel_colors_nr', 'pixel_colors_nr_fine', 'hit_prob_self', 'hit_prob_self_fine')
    loss = sum((torch.from_numpy(z['lw.' + k]).to(dev) * out[k]).sum() for k in keys)
    assert abs(float(loss.detach()) - float(z["loss"])) <= 5e-3
    loss.backward()
    assert r.engine(dev).det_scratch_bytes > 0

    def close(got, want, name, rel=5e-3):
        scale = max(1e-3, float(np.abs(want).max()))
        err = float(np.max(np.abs(got - want)))
        assert err <= rel * scale, (name, err, scale)

    for k, p_ in r.named_parameters():
        close(p_.grad.cpu().numpy() if p_.grad is not None else np.zeros(tuple(p_.shape), np.float32), z['grad.' + k], k)
    close(ref['ray_feats'].grad.cpu().numpy(), z['grad.ref.ray_feats'], 'ref.ray_feats')
    close(ref['img_feats'].grad.cpu().numpy(), z['grad.ref.img_feats'], 'ref.img_feats')
    close(que['ray_feats'].grad.cpu().numpy(), z['grad.que.ray_feats'], 'que.ray_feats')


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('tag', ['novis', 'vis'])
def test_deterministic_dr_loss_gradients_match_reference_autograd(tag, backend):
    """test_direct_rendering_backward.test_dr_loss_gradients_match_reference_autograd (tests/golden/case_dr_grads.npz) with the mode on, at
    its gates: 5e-3 of the tensor's max against the fp32 reference, and no further from the float64 one than 2x the fp32 one + 1e-3"""
    import test_direct_rendering_backward as drb
    z = drb._golden()
    r = drb._renderer(z, tag, backend, {'hip_deterministic': True})
    que, ref = drb._inputs(z, backend)
    dev = _dev(backend)
    loss = 0.0
    for is_fine, key in enumerate(('depth', 'depth_fine')):
        out = r.render_by_depth(torch.from_numpy(z['%s.%s' % (tag, key)]).to(dev), que, ref, True, bool(is_fine))
        sfx = '_fine' if is_fine else ''
        for k in ('pixel_colors_dr', 'hit_prob_dr'):
            assert out[k].grad_fn is not None
            loss = loss + (torch.from_numpy(z['lw.' + k + sfx]).to(dev) * out[k]).sum()
    assert abs(float(loss.detach()) - float(z[tag + '.loss'])) <= 5e-3
    loss.backward()
    assert r.engine(dev).det_scratch_bytes > 0
    params = dict(r.named_parameters())
    keys = [k[len(tag) + 6:] for k in z.files if k.startswith(tag + '.grad.')]
    assert 'ref.ray_feats' in keys
    for k in keys:
        got = (ref['ray_feats'].grad if k == 'ref.ray_feats' else params[k].grad)
        got = got.cpu().numpy() if got is not None else np.zeros_like(z['%s.grad.%s' % (tag, k)])
        want32 = z['%s.grad.%s' % (tag, k)]
        want64 = want32.astype(np.float64) + float(z['%s.grad64s.%s' % (tag, k)]) * z['%s.grad64d.%s' % (tag, k)].astype(np.float64)
        scale = max(1e-3, float(np.abs(want32).max()))
        e32 = float(np.abs(got - want32).max())
        e64, r64 = float(np.abs(got - want64).max()), float(np.abs(want32 - want64).max())
        assert e32 <= 5e-3 * scale, (k, e32, scale)
        assert e64 <= 2.0 * r64 + 1e-3 * scale, (k, e64, r64, scale)


# ---- 4. repeatability ---------------------------------------------------------------------------------------------------------------
def _self_pass_step(r, que, ref, depth, lw, dev):
    """one forward + backward of RenderPassSelfFn through render_by_depth, from fresh gradient buffers -> {name: gradient}"""
    for p_ in r.parameters():
        p_.grad = None
    q = {k: v.detach().clone() for k, v in que.items()}
    f = {k: v.detach().clone() for k, v in ref.items()}
    for t_ in (f['ray_feats'], f['img_feats'], q['ray_feats']):
        t_.requires_grad_(True)
    out = r.render_by_depth(depth, q, f, True, False)
    assert type(out['hit_prob_self'].grad_fn.next_functions[0][0]).__name__.startswith('RenderPassSelfFn')      # (behind the [None])
    sum((lw[k] * out[k]).sum() for k in lw).backward()
    g = {k: p_.grad.detach().clone() for k, p_ in r.named_parameters() if p_.grad is not None}
    assert any(k.startswith('dist_decoder.vis_decoder') for k in g) and any(k.startswith('agg_net.') for k in g)
    g['ref.ray_feats'], g['ref.img_feats'], g['que.ray_feats'] = f['ray_feats'].grad, f['img_feats'].grad, q['ray_feats'].grad
    return g


def _repeatability(backend, rfn, rn, dn, h, w):
    dev = _dev(backend)
    cfg = {'use_hierarchical_sampling': False, 'dist_decoder_cfg': {'use_vis': True}, 'use_self_hit_prob': True, 'depth_sample_num': dn,
           'agg_net_cfg': {'sample_num': dn}}
    que, ref = synthetic.make_scene(h, w, rfn, seed=17, que_imgs=True)
    rng = np.random.RandomState(5)
    que['coords'] = (rng.rand(1, rn, 2) * np.array([w - 1, h - 1])).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)            # noqa: E731
    que, ref = {k: t(v) for k, v in que.items()}, {k: t(v) for k, v in ref.items()}
    lw = {'pixel_colors_nr': t(rng.randn(1, rn, 3).astype(np.float32)), 'hit_prob_nr': t(rng.randn(1, rn, dn).astype(np.float32)),
          'hit_prob_self': t(rng.randn(1, rn, dn).astype(np.float32))}
    runs = {}
    for mode in (True, False) if backend == 'hip' else (True,):
        torch.manual_seed(3)
        r = NeuralRayBaseRenderer({**cfg, 'hip_deterministic': mode}).train()
        if backend == 'emu':
            r._engine_test_lib = emu_lib()
        r = r.to(dev)
        depth = r.engine(dev).sample_coarse_depth(que['depth_range'], rn, dn)[None]
        runs[mode] = [_self_pass_step(r, que, ref, depth, lw, dev) for _ in range(3 if mode else 2)]
    a = runs[True][0]
    assert float(a['ref.ray_feats'].abs().max()) > 0 and float(a['que.ray_feats'].abs().max()) > 0
    for other in runs[True][1:]:
        assert set(other) == set(a)
        for k in a:
            assert torch.equal(a[k], other[k]), k
    if False in runs:        # information only: whether the atomic mode happened to differ between two runs here (never asserted)
        diff = [k for k in runs[False][0] if not torch.equal(runs[False][0][k], runs[False][1][k])]
        print('default (atomic) mode, two runs [%d rays x %d samples x %d views]: %d of %d gradients differ bitwise'
              % (rn, dn, rfn, len(diff), len(runs[False][0])))


@pytest.mark.parametrize('backend', BACKENDS)
def test_repeatable_gradients_with_every_texel_contended(backend):
    """3 views, 37 rays x 9 samples on 12 x 16 feature maps (a 48 x 64 scene), a vis-head decoder, use_self_hit_prob"""
    _repeatability(backend, 3, 37, 9, 48, 64)


@pytest.mark.parametrize('backend', [pytest.param('hip', marks=pytest.mark.gpu)])
def test_repeatable_gradients_at_the_training_shape(backend):
    """512 rays x 64 samples x 8 views at 600 x 800: 2048 tiles on the persistent grid's 256 workgroups - every workgroup owns several.
    On the GPU only: the CPU emulator runs workgroups one after the other, so it cannot tell the orders apart, and this shape takes it
    ten minutes (the toy above covers the code path there)."""
    _repeatability(backend, 8, 512, 64, 600, 800)


# ---- 6. plumbing ------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """an engine whose backward methods record the `deterministic` keyword they receive, then run"""
    NAMES = ('render_points_backward', 'render_rays_backward', 'self_hit_prob_backward', 'interpolate_feats_backward')

    def __init__(self, eng):
        self.seen = {}
        for name in self.NAMES:
            setattr(eng, name, self._wrap(name, getattr(eng, name)))

    def _wrap(self, name, fn):
        def call(*a, **k):
            self.seen.setdefault(name, []).append(k.get('deterministic', 'absent'))
            return fn(*a, **k)
        return call


def _toy_step(cfg_extra, cls=NeuralRayBaseRenderer):
    cfg = {'use_hierarchical_sampling': False, 'dist_decoder_cfg': {'use_vis': True}, 'use_self_hit_prob': True, 'depth_sample_num': 5,
           'agg_net_cfg': {'sample_num': 5}, **cfg_extra}
    que, ref = synthetic.make_scene(16, 24, 2, seed=1, que_imgs=True)
    que['coords'] = (np.random.RandomState(0).rand(1, 3, 2) * np.array([23, 15])).astype(np.float32)
    que, ref = {k: torch.from_numpy(v) for k, v in que.items()}, {k: torch.from_numpy(v) for k, v in ref.items()}
    ref['ray_feats'].requires_grad_(True)
    que['ray_feats'].requires_grad_(True)
    torch.manual_seed(0)
    r = cls(cfg).train()
    r._engine_test_lib = emu_lib()
    rec = _Recorder(r.engine('cpu'))
    out = r.render_impl(que, ref, True)
    (out['pixel_colors_nr'].sum() + out['hit_prob_self'].sum()).backward()
    assert set(rec.seen) == set(_Recorder.NAMES)
    modes = {m for v in rec.seen.values() for m in v}
    assert len(modes) == 1
    return modes.pop(), r.engine('cpu').det_scratch_bytes


def test_mode_is_off_by_default_and_allocates_nothing():
    assert NeuralRayBaseRenderer({}).cfg['hip_deterministic'] is False
    mode, scratch = _toy_step({})
    assert mode is False and scratch == 0
    mode, scratch = _toy_step({'hip_deterministic': True})
    assert mode is True and scratch > 0


def test_environment_beats_the_cfg(monkeypatch):
    monkeypatch.setenv('NEURAY_HIP_DETERMINISTIC', '1')
    assert _toy_step({'hip_deterministic': False})[0] is True
    monkeypatch.setenv('NEURAY_HIP_DETERMINISTIC', '0')
    mode, scratch = _toy_step({'hip_deterministic': True})
    assert mode is False and scratch == 0
    monkeypatch.setenv('NEURAY_HIP_DETERMINISTIC', 'yes')
    with pytest.raises(ValueError, match='NEURAY_HIP_DETERMINISTIC'):
        _toy_step({})


def test_auto_follows_torch_deterministic_algorithms():
    before = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        r = NeuralRayBaseRenderer({'hip_deterministic': 'auto'})
        assert r._deterministic_mode() is False and fused_norm.deterministic() is False
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert r._deterministic_mode() is True and fused_norm.deterministic() is True
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
    with pytest.raises(ValueError, match='hip_deterministic'):
        NeuralRayBaseRenderer({'hip_deterministic': 'on'})


def test_a_renderer_leaves_the_users_module_flag_alone():
    """fused_norm.DETERMINISTIC is the user's; a renderer writes its cfg into its own slot, and either one turns the switch on"""
    fused_norm.DETERMINISTIC = True
    r = NeuralRayBaseRenderer({})
    r._deterministic_mode()
    assert fused_norm.DETERMINISTIC is True and fused_norm.RENDERER_DETERMINISTIC is False and fused_norm.deterministic() is True
    fused_norm.DETERMINISTIC = False
    assert fused_norm.deterministic() is False
    NeuralRayBaseRenderer({'hip_deterministic': True})
    assert fused_norm.DETERMINISTIC is False and fused_norm.deterministic() is True
    NeuralRayBaseRenderer({})
    assert fused_norm.deterministic() is False


class _Seen:
    """records the `deterministic` keyword that the named engine methods receive"""

    def __init__(self, eng, names):
        self.seen = {}
        for name in names:
            setattr(eng, name, self._wrap(name, getattr(eng, name)))

    def _wrap(self, name, fn):
        def call(*a, **k):
            self.seen.setdefault(name, []).append(k.get('deterministic', 'absent'))
            return fn(*a, **k)
        return call


@pytest.mark.parametrize('backend', BACKENDS)
def test_depth_loss_path_follows_the_switch(backend):
    """NeuralRayGenRenderer.predict_mean_for_depth_loss (renderer.py:280-316): interpolate_feature_map + dist_decoder.predict_mean as
    stand-alone autograd functions.  With the mode on their backward runs the sorted scatter and the ordered flush - recorded on the
    engine - and three runs give bitwise the same gradients; with it off they receive deterministic=False and allocate nothing."""
    from neuray_amd.network import render_ops as ro
    from neuray_amd.network.renderer import NeuralRayGenRenderer
    dev = _dev(backend)
    old = ro._TEST_LIB
    if backend == 'emu':
        ro._TEST_LIB = emu_lib()
        ro._ENGINES.clear()
    try:
        eng = ro.engine_for(dev)
        rec = _Seen(eng, ('interpolate_feats_backward', 'dist_decoder_rows_backward'))
        rng = np.random.RandomState(2)
        rfn, h, w = 3, 24, 32
        imgs = torch.from_numpy(rng.rand(rfn, 3, h, w).astype(np.float32)).to(dev)
        feats0 = torch.from_numpy(rng.randn(rfn, 32, h // 4, w // 4).astype(np.float32)).to(dev)
        for mode in (True, False):
            torch.manual_seed(1)
            r = NeuralRayGenRenderer({'use_hierarchical_sampling': True, 'use_depth_loss': True, 'depth_loss_coords_num': 700,
                                      'hip_deterministic': mode, 'init_net_type': 'none'}, init_net=torch.nn.Identity()).train().to(dev)
            assert r._deterministic_mode() is mode
            rec.seen.clear()
            before = eng.det_scratch_bytes
            runs = []
            for _ in range(3 if mode else 1):
                r.zero_grad(set_to_none=True)
                feats = feats0.clone().requires_grad_(True)
                torch.manual_seed(9)                                   # the same depth-loss pixels: 700 on 6 x 8 texels, all contended
                out = r.predict_mean_for_depth_loss({'imgs': imgs, 'ray_feats': feats})
                (out['depth_mean'].square().sum() + out['depth_mean_fine_2'].sum()).backward()
                g = {k: p_.grad.detach().clone() for k, p_ in r.named_parameters() if p_.grad is not None}
                assert any(k.startswith('dist_decoder.mean_decoder') for k in g) and any(k.startswith('fine_dist_decoder.') for k in g)
                g['ray_feats'] = feats.grad.detach().clone()
                assert float(g['ray_feats'].abs().max()) > 0
                runs.append(g)
            assert set(rec.seen) == {'interpolate_feats_backward', 'dist_decoder_rows_backward'}
            assert {m for v in rec.seen.values() for m in v} == {mode}
            assert (eng.det_scratch_bytes > before) == mode
            for other in runs[1:]:
                for k in runs[0]:
                    assert torch.equal(runs[0][k], other[k]), k
    finally:
        ro._TEST_LIB = old
        ro._ENGINES.clear()


def test_direct_rendering_backward_receives_the_mode():
    """DirectRenderFn hands PassRun.deterministic to engine.direct_render_backward, which hands it to the rows backward and the map
    scatter: False (and no scratch) by default, True with the key"""
    import test_direct_rendering_backward as drb
    z = drb._golden()
    for mode in (False, True):
        r = drb._renderer(z, 'novis', 'emu', {'hip_deterministic': True} if mode else None)
        que, ref = drb._inputs(z, 'emu')
        eng = r.engine('cpu')
        rec = _Seen(eng, ('direct_render_backward', 'dist_decoder_rows_backward', 'interpolate_feats_backward'))
        out = r.render_by_depth(torch.from_numpy(z['novis.depth']), que, ref, True, False)
        (out['pixel_colors_dr'].sum() + out['hit_prob_dr'].sum()).backward()
        assert set(rec.seen) == {'direct_render_backward', 'dist_decoder_rows_backward', 'interpolate_feats_backward'}
        assert {m for v in rec.seen.values() for m in v} == {mode}
        assert (eng.det_scratch_bytes > 0) == mode


def test_unsupported_variant_is_refused_before_a_launch():
    """the inference-only bf16 library has no backward kernels: refused by render_impl before an engine (or a library) exists"""
    que, ref = synthetic.make_scene(16, 24, 2, seed=1, que_imgs=True)
    que['coords'] = np.zeros((1, 3, 2), np.float32)
    que, ref = {k: torch.from_numpy(v) for k, v in que.items()}, {k: torch.from_numpy(v) for k, v in ref.items()}
    with pytest.raises(NotImplementedError, match='hip_deterministic'):
        NeuralRayBaseRenderer({'hip_variant': 'bf16', 'hip_deterministic': True})
    r = NeuralRayBaseRenderer({'hip_variant': 'bf16'})
    r.cfg['hip_deterministic'] = True
    with pytest.raises(NotImplementedError, match='hip_deterministic'):
        r.render_impl(que, ref, True)
    assert r.__dict__.get('_engine') is None
    assert NeuralRayBaseRenderer({'hip_variant': 'bf16x3', 'hip_deterministic': True})._deterministic_mode() is True


def test_patch_reference_carries_the_key_onto_the_reference_class():
    """integrate.patch_reference on tests/ref_stub: the reference's class, constructed by its own __init__, runs the mode from its cfg"""
    import importlib
    import sys
    from neuray_amd import integrate
    from neuray_amd.network.hip_path import HOT_PATH_METHODS
    assert '_deterministic_mode' in HOT_PATH_METHODS
    stub = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_stub')
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'network' or k.startswith('network.')}
    sys.path.insert(0, stub)
    try:
        mod = integrate.patch_reference(importlib.import_module('network.renderer'))
        try:
            cls = mod.NeuralRayBaseRenderer
            assert 'hip_deterministic' not in cls.base_cfg                  # (the stand-in's own constructor and cfg, as the reference's)
            mode, scratch = _toy_step({'hip_deterministic': True}, cls)
            assert mode is True and scratch > 0
            mode, scratch = _toy_step({}, cls)
            assert mode is False and scratch == 0
            host = cls({'hip_deterministic': True, 'hip_variant': 'bf16'})
            with pytest.raises(NotImplementedError, match='hip_deterministic'):
                host._deterministic_mode()
        finally:
            integrate.unpatch_reference(mod)
    finally:
        sys.path.remove(stub)
        for k in [k for k in sys.modules if k == 'network' or k.startswith('network.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_launcher_flag_sets_the_environment(monkeypatch, tmp_path):
    from neuray_amd import launch
    monkeypatch.setattr(launch, 'run', lambda *a, **k: None)
    monkeypatch.delenv('NEURAY_HIP_DETERMINISTIC', raising=False)
    script = tmp_path / 's.py'
    script.write_text('')
    launch.main(['--deterministic', str(script)])
    assert os.environ['NEURAY_HIP_DETERMINISTIC'] == '1'
    monkeypatch.delenv('NEURAY_HIP_DETERMINISTIC', raising=False)


@pytest.mark.parametrize('backend', BACKENDS)
def test_det_entries_check_their_arguments(backend):
    eng = _engine(backend)
    assert eng.lib.neuray_reduce_partials(None, 1, 1, None, None) != 0
    assert b'null' in eng.lib.neuray_last_error()
    assert eng.lib.neuray_deterministic_partials_floats(_lib.DET_RAYS, 512, 64) == 128 * _lib.PACKED_RAY_FLOATS
    assert eng.lib.neuray_deterministic_partials_floats(_lib.DET_POINTS, 512, 64) == 2 * 256 * eng.lib.neuray_flat_pass_floats()
    assert eng.lib.neuray_deterministic_partials_floats(99, 512, 64) == 0
    assert eng.lib.neuray_points_backward_scatter_columns(17) == 32 * 8
