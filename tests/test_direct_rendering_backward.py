"""Training through direct rendering (cfg use_dr_loss / use_dr_fine_loss, network/loss.py:70-76): the gradient of a loss on
pixel_colors_dr / hit_prob_dr through the dr backward kernels (csrc/nr_kernels_dr.h), autograd.DirectRenderFn and the dist decoder /
feature-map backward, into the pass's dist decoder and ref ray_feats.

  1. the two kernels on identical inputs against a float64 torch composition of the dr math written here (3, 8, 16 views; masked
     views and points no view sees);
  2. each pass end to end against the REFERENCE's autograd (tests/golden/case_dr_grads.npz, make_golden_dr_grads.py): every gradient
     within 5e-3 of its tensor's max (the rule of test_backward.py::test_training_gradients_match_reference_autograd), and no further
     from the float64 reference than 2x the fp32 reference is (+ a floor: the 16 x 16 SH solve is ill conditioned).  The float64
     gradients are stored as scaled fp16 differences from the fp32 ones (within 2.5e-4 x their largest: make_golden_dr_grads.py);
  3. a mixed nr + dr loss through render_impl(is_train=True) gets the sum of the two paths' gradients;
  4. use_nr_color_for_dr with a dr loss is refused; under torch.no_grad() the dr flags change nothing."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, load_weights, oracle_cfg
from emu_util import emu_lib, to_torch
from oracle import neuray_oracle as orc
from test_render_parity import BACKENDS

GROUND = -15.0


def _dev(backend):
    return 'cpu' if backend == 'emu' else 'cuda:0'


def _engine(backend):
    from neuray_amd.engine import RenderEngine
    return RenderEngine(_dev(backend), _test_lib=emu_lib() if backend == 'emu' else None)


# ---- 1. kernel level ------------------------------------------------------------------------------------------------------------
def _torch_dr(rec, near, far, rgb, dirs, que_dir, regs, use_vis):
    """float64 composition of renderer.py:85-125 + sph_solver.py + dist_decoder.py:109-144 on the record's decoder outputs.
    rec [pn,rfn,16] (fields 0 mask, 6-11 decoder outputs), near / far [pn,rfn], rgb / dirs [pn,rfn,3], que_dir [pn,3] ->
    (leaves {mu, var, aw, nu}, alpha [pn], colour [pn,3])"""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)      # noqa: E731
    m = t(rec[..., 0])
    mu = t(rec[..., 6:8]).requires_grad_(True)
    var = t(rec[..., 8:10]).requires_grad_(True)
    aw = t(rec[..., 10]).requires_grad_(True)
    nu = t(rec[..., 11]).requires_grad_(True)
    near, far = t(near)[..., None], t(far)[..., None]
    mix = torch.stack([aw, 1 - aw], -1)
    c0, c1 = 0.5 + 0.5 * torch.tanh((near - mu) * var), 0.5 + 0.5 * torch.tanh((far - mu) * var)
    if use_vis:
        c0, c1 = c0 * nu[..., None], c1 * nu[..., None]
    vis = ((1 - c0) * mix).sum(-1)
    hit = ((c1 - c0) * mix).sum(-1)
    logit = torch.log(hit / (vis - hit + 1e-5) + 1e-5)
    a_v = logit * m + (1 - m) * GROUND
    s, h = vis * m, hit * m
    alpha = (s * a_v).sum(1) / (s.sum(1) + 1e-5)
    invalid = (m.sum(1) == 0).double()
    alpha = alpha * (1 - invalid) + invalid * GROUND
    w = h / (h.sum(1, keepdim=True) + 1e-3)
    w = w + (w.sum(1, keepdim=True) < 1e-4).double() * 1e-4
    A = t(orc.sph_basis(np.asarray(dirs, np.float64)))                       # [pn,rfn,16]
    M = (A * w[..., None]).transpose(1, 2) @ A + torch.diag(t(regs))[None]
    theta = torch.linalg.solve(M, (A * w[..., None]).transpose(1, 2) @ t(rgb))
    colour = (t(orc.sph_basis(np.asarray(que_dir, np.float64)))[:, None] @ theta)[:, 0]
    return {'mu': mu, 'var': var, 'aw': aw, 'nu': nu}, alpha, colour, (h, vis * m)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('rfn,use_vis', [(3, False), (8, True), (16, False)])
def test_dr_backward_kernels_against_float64_autograd(rfn, use_vis, backend):
    from neuray_amd import _lib
    rn, dn = 10, 12
    cfg = {'dist_decoder_cfg': {'use_vis': use_vis}, 'depth_sample_num': dn, 'agg_net_cfg': {'sample_num': dn}}
    ocfg = oracle_cfg({**orc.DEFAULT_CFG, **cfg})
    weights = load_weights(use_vis)
    que, ref = orc.make_scene(32, 40, rfn, seed=20 + rfn, depth_range=(0.8, 9.0))
    ref['poses'][1] = orc.look_at_pose(orc.sphere_pos(2.5, 30.0, 25.0), target=orc.sphere_pos(8.0, 30.0, 25.0))   # samples behind it
    rng = np.random.RandomState(rfn)
    que['coords'] = (rng.rand(1, rn, 2) * np.array([39, 31])).astype(np.float32)
    depth = orc.sample_depth(que['depth_range'], rn, dn)
    _, aux = orc.render_by_depth(weights, ocfg, depth, que, ref, False, False, return_aux=True)
    prj = aux['prj']
    pt = lambda a: np.moveaxis(a[:, 0], 0, 2).reshape(rn * dn, rfn, *a.shape[4:])          # [rfn,1,rn,dn,...] -> [pn,rfn,...]  # noqa: E731
    rec = np.zeros((rn * dn, rfn, _lib.DBG_FIELDS), np.float32)
    rec[..., 0] = pt(prj['mask'])[..., 0]
    rec[..., 1:3] = pt(prj['pts'])
    rec[..., 3] = pt(prj['depth'])[..., 0]
    rec[..., 6:8], rec[..., 8:10], rec[..., 10] = pt(prj['_mean']), pt(prj['_var']), pt(prj['_aw'])[..., 0]
    rec[..., 11] = 1.0
    if use_vis:
        _, _, vis_dec, _ = orc.dist_decoder_forward(weights, 'dist_decoder.', prj['ray_feats'])
        rec[..., 11] = pt(vis_dec)[..., 0]
    rec[:dn // 2, :, 0] = 0.0                                   # ray 0's first samples: no view sees them (alpha = ground)
    assert 0 < (rec[..., 0] > 0).mean() < 1
    que_dists = orc.depth2inv_dists(depth, que['depth_range'])
    near, far = orc.get_near_far_points(prj['depth'][..., 0], que_dists[None], ref['depth_range'], True)
    regs = orc.SPH_REGS
    leaves, alpha, colour, (h, s) = _torch_dr(rec, pt(near[..., None])[..., 0], pt(far[..., None])[..., 0], pt(prj['rgb']),
                                              pt(prj['dir']), aux['que_dir'].reshape(-1, 3), regs, use_vis)
    rec[..., 4], rec[..., 5] = h.detach().numpy(), s.detach().numpy()
    alpha.retain_grad()
    colour.retain_grad()
    a = torch.sigmoid(alpha.view(rn, dn))
    T = torch.cumprod(torch.cat([torch.ones(rn, 1, dtype=torch.float64), 1 - a + 1e-10], 1), 1)[:, :-1]
    hitp = a * T
    pix = (hitp[..., None] * colour.view(rn, dn, 3)).sum(1)
    g_pix, g_hit = rng.randn(rn, 3), rng.randn(rn, dn)
    ((pix * torch.from_numpy(g_pix)).sum() + (hitp * torch.from_numpy(g_hit)).sum()).backward()

    dev = _dev(backend)
    eng = _engine(backend)
    tq, tr = to_torch(que, dev), to_torch(ref, dev)
    tq.pop('Ks_inv', None)
    views, qc = eng.prepare_views(tr), eng.prepare_query(tq)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)        # noqa: E731
    d_rec, d_depth = f(rec.reshape(rn, dn, rfn, -1)), f(depth[0])
    dr = eng.direct_render(qc, views, tq['coords'][0], d_depth, d_rec, torch.from_numpy(regs), ground=GROUND)
    assert np.abs(dr['hit_prob'].cpu().numpy() - hitp.detach().numpy()).max() <= 1e-5
    d_alpha, d_col = eng.direct_render_rays_backward(dr['alpha'], dr['colors'], f(g_pix), f(g_hit))

    def close(got, want, name, rel):
        got = got.detach().cpu().numpy().reshape(want.shape)
        scale = max(1e-6, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        print('%s [%d views, %s]: max err %.2e of %.2e' % (name, rfn, backend, err, scale))
        assert np.all(np.isfinite(got)) and err <= rel * scale, (name, err, scale)

    close(d_alpha, alpha.grad.numpy(), 'd alpha_dr', 1e-4)
    close(d_col, colour.grad.numpy(), 'd colour', 1e-5)
    # the points kernel on the float64 upstream gradients (rounded once), so its own error is what is measured
    d_dec = eng.direct_render_points_backward(qc, views, tq['coords'][0], d_depth, d_rec, torch.from_numpy(regs),
                                              f(alpha.grad.numpy()), f(colour.grad.numpy()), use_vis).cpu().numpy()
    d_dec = d_dec.reshape(rn * dn, rfn, 6)
    masked = rec[..., 0] == 0
    assert np.all(d_dec[masked] == 0.0)
    close(torch.from_numpy(d_dec[..., 0:2]), leaves['mu'].grad.numpy(), 'd mu', 5e-3)
    close(torch.from_numpy(d_dec[..., 2:4]), leaves['var'].grad.numpy(), 'd var', 5e-3)
    close(torch.from_numpy(d_dec[..., 4]), leaves['aw'].grad.numpy(), 'd aw', 5e-3)
    if use_vis:
        close(torch.from_numpy(d_dec[..., 5]), leaves['nu'].grad.numpy(), 'd vis_dec', 5e-3)
    else:
        assert np.all(d_dec[..., 5] == 0.0)


# ---- 2. end to end per pass against the reference --------------------------------------------------------------------------------
def _golden():
    return np.load(os.path.join(GOLDEN_DIR, 'case_dr_grads.npz'))


def _scene(z):
    """the golden's scene, rebuilt from its seed as tests/golden/make_golden_dr_grads.py scene() builds it (not stored: size); the
    fingerprint proves it is the same"""
    import hashlib
    rn, h, w = 24, 48, 48
    que, ref = orc.make_scene(h, w, 5, seed=6, depth_range=(0.8, 9.0))
    ref['poses'][1] = orc.look_at_pose(orc.sphere_pos(2.5, 30.0, 25.0), target=orc.sphere_pos(8.0, 30.0, 25.0))
    ref['poses'][2] = orc.look_at_pose(orc.sphere_pos(9.0, 200.0, -40.0))
    ref['depth_range'][2] = np.array([5.0, 13.0], np.float32)
    que['coords'] = (np.random.RandomState(1006).rand(1, rn, 2) * np.array([w - 1, h - 1])).astype(np.float32)
    sha = hashlib.sha256()
    for pre, d in (('que.', que), ('ref.', ref)):
        for k in sorted(d):
            a = np.ascontiguousarray(d[k])
            sha.update((pre + k + str(a.dtype) + str(a.shape)).encode())
            sha.update(a.tobytes())
    assert sha.hexdigest() == str(z['scene_sha256']), "the scene differs from the one the golden was made on"
    return que, ref


def _renderer(z, tag, backend, cfg_override=None):
    from neuray_amd.network.renderer import NeuralRayBaseRenderer
    cfg = ast.literal_eval(str(z[tag + '.cfg_json']))
    cfg.update(cfg_override or {})
    r = NeuralRayBaseRenderer(cfg)
    r.load_state_dict({k: torch.from_numpy(v) for k, v in load_weights(tag == 'vis').items()}, strict=True)
    r.train()
    if backend == 'emu':
        r._engine_test_lib = emu_lib()
    return r.to(_dev(backend))


def _inputs(z, backend):
    que, ref = _scene(z)
    que, ref = to_torch(que, _dev(backend)), to_torch(ref, _dev(backend))
    ref['ray_feats'].requires_grad_(True)
    return que, ref


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('tag', ['novis', 'vis'])
def test_dr_loss_gradients_match_reference_autograd(tag, backend):
    z = _golden()
    r = _renderer(z, tag, backend)
    que, ref = _inputs(z, backend)
    dev = _dev(backend)
    loss = 0.0
    for is_fine, key in enumerate(('depth', 'depth_fine')):
        out = r.render_by_depth(torch.from_numpy(z['%s.%s' % (tag, key)]).to(dev), que, ref, True, bool(is_fine))
        sfx = '_fine' if is_fine else ''
        for k in ('pixel_colors_dr', 'hit_prob_dr'):
            assert out[k].grad_fn is not None
            np.testing.assert_allclose(out[k].detach().cpu().numpy(), z['%s.out.%s%s' % (tag, k, sfx)], atol=2e-4)
            loss = loss + (torch.from_numpy(z['lw.' + k + sfx]).to(dev) * out[k]).sum()
    assert abs(float(loss.detach()) - float(z[tag + '.loss'])) <= 5e-3
    loss.backward()
    params = dict(r.named_parameters())
    keys = [k[len(tag) + 6:] for k in z.files if k.startswith(tag + '.grad.')]
    assert 'ref.ray_feats' in keys and any(k.startswith('fine_dist_decoder.') for k in keys)
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
    # parameters the dr path does not reach keep no gradient from it
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for k, p in params.items() if 'agg_net' in k)


# ---- 3. mixed nr + dr loss through render_impl ----------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_mixed_loss_gradients_are_the_sum_of_both_paths(backend):
    z = _golden()
    dev = _dev(backend)
    que0, _ = _inputs(z, backend)
    rn = 12
    lw = {k: torch.from_numpy(np.random.RandomState(i).randn(*shape).astype(np.float32)).to(dev) for i, (k, shape) in enumerate(
        (('pixel_colors_nr', (1, rn, 3)), ('pixel_colors_nr_fine', (1, rn, 3)), ('pixel_colors_dr', (1, rn, 3)),
         ('pixel_colors_dr_fine', (1, rn, 3)), ('hit_prob_dr', (1, rn, 16))))}

    def step(keys):
        r = _renderer(z, 'novis', backend)
        que, ref = _inputs(z, backend)
        que['coords'] = que['coords'][:, :rn]
        torch.manual_seed(77)
        out = r.render_impl(que, ref, True)
        sum((lw[k] * out[k]).sum() for k in keys).backward()
        g = {k: p.grad.detach().cpu().clone() if p.grad is not None else torch.zeros_like(p).cpu() for k, p in r.named_parameters()}
        g['ref.ray_feats'] = ref['ray_feats'].grad.detach().cpu().clone()
        return g

    nr_keys, dr_keys = ['pixel_colors_nr', 'pixel_colors_nr_fine'], ['pixel_colors_dr', 'pixel_colors_dr_fine', 'hit_prob_dr']
    both, nr, dr = step(nr_keys + dr_keys), step(nr_keys), step(dr_keys)
    assert float(dr['dist_decoder.mean_decoder.0.weight'].abs().max()) > 0 and float(dr['fine_dist_decoder.aw_decoder.4.weight'].abs().max()) > 0
    for k in both:
        want = nr[k] + dr[k]
        scale = max(1e-6, float(want.abs().max()))
        assert float((both[k] - want).abs().max()) <= 1e-5 * scale + 1e-7, k


# ---- 4. the refused combination and the unchanged inference path ------------------------------------------------------------------
def test_nr_colour_for_dr_with_a_dr_loss_is_refused():
    z = _golden()
    r = _renderer(z, 'novis', 'emu', {'use_nr_color_for_dr': True})
    que, ref = _inputs(z, 'emu')
    que['coords'] = que['coords'][:, :4]
    with pytest.raises(NotImplementedError, match='use_nr_color_for_dr'):
        r.render_impl(que, ref, True)


@pytest.mark.parametrize('backend', BACKENDS)
def test_dr_flags_leave_no_grad_outputs_bit_identical(backend):
    z = _golden()
    outs = []
    for flags in ({'use_dr_loss': False, 'use_dr_fine_loss': False}, {}):
        r = _renderer(z, 'vis', backend, flags)
        que, ref = _inputs(z, backend)
        with torch.no_grad():
            torch.manual_seed(5)
            outs.append(r.render_impl(que, ref, True))
    assert set(outs[0]) == set(outs[1])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
