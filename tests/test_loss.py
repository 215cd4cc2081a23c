"""The training losses on the HIP loss kernels (csrc/nr_kernels_loss.h, neuray_train_loss[_backward], RenderEngine.train_loss,
neuray_amd.loss) against
  * tests/golden/case_loss.npz: the reference's own network/loss.py in float64 on the seeded inputs of tests/loss_cases.py, with
    `dev32`, the largest deviation of the reference's own float32 run from it (tests/golden/make_golden_loss.py);
  * the float64 composition of tests/loss_cases.py - first held against the golden to 1e-10 relative, then the expected value at the
    shapes the golden does not have (and on the GPU box, where the reference does not exist), with dev32 from its own float32 run.
Gates, per key and per gradient tensor:  max |ours - ref64| <= 3 max(dev32, 4 * 2^-23 * max |ref64|).  The measure is the reference's
float32 error, never our output; 3 allows another summation order and log implementation on a maximum over thousands of elements,
the floor keeps a key whose reference error happens to be tiny from asking for less than four fp32 roundings.
Exact properties (determinism, independence of the other terms, masks, detached p0) are checked with ==."""
import os

import numpy as np
import pytest
import torch

import loss_cases as lc
from conftest import GOLDEN_DIR
from emu_util import emu_lib
from neuray_amd import loss as nloss

BACKENDS = ['emu', pytest.param('hip', marks=pytest.mark.gpu)]
EPS = 4 * 2.0 ** -23
FULL = {'use_dr_loss': True, 'use_dr_fine_loss': True, 'use_nr_fine_loss': True}
_ENG = {}


def engine(backend):
    from neuray_amd.engine import RenderEngine
    if backend not in _ENG:
        _ENG[backend] = RenderEngine('cpu', _test_lib=emu_lib()) if backend == 'emu' else RenderEngine('cuda:0')
    return _ENG[backend]


def golden():
    z = np.load(os.path.join(GOLDEN_DIR, 'case_loss.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def gate(what, ours, ref64, dev32):
    ours, ref64 = np.asarray(ours, np.float64), np.asarray(ref64, np.float64)
    assert ours.shape == ref64.shape, (what, ours.shape, ref64.shape)
    err = float(np.abs(ours - ref64).max())
    bound = 3 * max(float(dev32), EPS * float(np.abs(ref64).max()))
    print('%-44s err %.3e  bound %.3e  (dev32 %.3e, max |ref64| %.3e)' % (what, err, bound, float(dev32), float(np.abs(ref64).max())))
    assert err <= bound, '%s: max |ours - ref64| = %.3e > %.3e = 3 max(dev32 %.3e, 4 * 2^-23 * %.3e)' % (
        what, err, bound, float(dev32), float(np.abs(ref64).max()))


def total_and_grads(out, leaves):
    total = sum(torch.mean(v) for v in out.values())
    grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    return {k: v.detach().cpu().double().numpy() for k, v in out.items()}, \
        {k: (g.detach().cpu().double().numpy() if g is not None else None) for k, g in zip(leaves, grads)}


# ---- the three calls, ours and the composition, on one input case ------------------------------------------------------------------
def render_data(case, dtype, device):
    leaves = {k: lc.as_torch(v, dtype, device).requires_grad_(True) for k, v in case.items()
              if k.startswith('pixel_colors_') and k != 'pixel_colors_gt'}
    return {**leaves, 'pixel_colors_gt': lc.as_torch(case['pixel_colors_gt'], dtype, device), 'ray_mask': lc.as_torch(case['ray_mask'], device=device)}, leaves


def render_composition(case, use_mask, dtype, device='cpu'):
    data, leaves = render_data(case, dtype, device)
    sfx = [k[len('pixel_colors_'):] for k in leaves]
    order = ['nr'] + [s for s in ('dr', 'dr_fine', 'nr_fine') if s in sfx]
    vals = lc.render_terms([data['pixel_colors_' + s] for s in order], data['pixel_colors_gt'], data['ray_mask'] if use_mask else None)
    return total_and_grads({'loss_rgb_' + s: v for s, v in zip(order, vals)}, leaves)


def render_ours(case, use_mask, backend):
    eng = engine(backend)
    data, leaves = render_data(case, torch.float32, eng.device)
    cfg = {'use_ray_mask': use_mask, **{'use_%s_loss' % s: ('pixel_colors_' + s) in leaves for s in ('dr', 'dr_fine', 'nr_fine')}}
    return total_and_grads(nloss.RenderLoss(cfg, engine=eng)(data, {}, 0), leaves)


def consist_data(case, dtype, device):
    leaves = {k: lc.as_torch(v, dtype, device).requires_grad_(True) for k, v in case.items() if k.startswith('hit_prob_')}
    return {**leaves, 'ray_mask': lc.as_torch(case['ray_mask'], device=device)}, leaves


def consist_composition(case, dtype, device='cpu'):
    data, leaves = consist_data(case, dtype, device)
    pairs = [(data['hit_prob_nr' + s], data['hit_prob_self' + s]) for s in ('', '_fine') if 'hit_prob_nr' + s in data]
    return total_and_grads(dict(zip(['loss_prob', 'loss_prob_fine'], lc.consist_terms(pairs))), leaves)


def consist_ours(case, backend, cfg=None):
    eng = engine(backend)
    data, leaves = consist_data(case, torch.float32, eng.device)
    return total_and_grads(nloss.ConsistencyLoss(cfg or {}, engine=eng)(data, {}, 0), leaves)


def depth_composition(case, loss_type, dtype, device='cpu'):
    data_pr, data_gt, leaves = lc.depth_data(case, dtype, device)
    info = data_gt['ref_imgs_info']
    preds = [data_pr['depth_mean']] + ([data_pr['depth_mean_fine']] if 'depth_mean_fine' in data_pr else [])
    vals = lc.depth_terms(preds, info['true_depth'], info.get('depth') if case['scene_name'].startswith('gso') else None,
                          data_pr['depth_coords'], info['depth_range'], loss_type)
    return total_and_grads(dict(zip(['loss_depth', 'loss_depth_fine'], vals)), leaves)


def depth_ours(case, loss_type, backend):
    eng = engine(backend)
    data_pr, data_gt, leaves = lc.depth_data(case, torch.float32, eng.device)
    assert not data_pr['depth_mean'].is_contiguous()                  # the [..., 0] view of the decoder's read-out
    return total_and_grads(nloss.DepthLoss({'depth_loss_type': loss_type}, engine=eng)(data_pr, data_gt, 0), leaves)


def cases():
    out = []
    for name, kw in lc.RENDER_CASES.items():
        case = lc.render_inputs(**kw)
        out.append((name, case, lambda dt, c=case, m=name == 'render_mask': render_composition(c, m, dt),
                    lambda be, c=case, m=name == 'render_mask': render_ours(c, m, be)))
    for name, kw in lc.CONSIST_CASES.items():
        case = lc.consist_inputs(**kw)
        out.append((name, case, lambda dt, c=case: consist_composition(c, dt), lambda be, c=case: consist_ours(c, be)))
    for name, kw in lc.DEPTH_CASES.items():
        case = lc.depth_inputs(**kw)
        out.append((name, case, lambda dt, c=case, t=lc.DEPTH_CFG[name]: depth_composition(c, t, dt),
                    lambda be, c=case, t=lc.DEPTH_CFG[name]: depth_ours(c, t, be)))
    return out


# ---- golden -----------------------------------------------------------------------------------------------------------------------
def test_composition_matches_the_reference_in_float64():
    """inputs are the golden's (sha256), and the float64 composition equals the reference's float64 run to 1e-10 relative"""
    g = golden()
    for name, case, comp, _ in cases():
        assert lc.digest(case) == str(g['sha.' + name]), name
        vals, grads = comp(torch.float64)
        for k, v in vals.items():
            ref = g['val.%s.%s' % (name, k)]
            assert np.abs(v - ref).max() <= 1e-10 * np.abs(ref).max(), (name, k, np.abs(v - ref).max())
        for k, v in grads.items():
            if v is None:
                assert 'grad.%s.%s' % (name, k) not in g
                continue
            ref = g['grad.%s.%s' % (name, k)]
            assert np.abs(v - ref).max() <= 1e-10 * np.abs(ref).max(), (name, k, np.abs(v - ref).max())


@pytest.mark.parametrize('backend', BACKENDS)
def test_values_and_gradients_against_the_reference_golden(backend):
    g = golden()
    for name, case, _, ours in cases():
        vals, grads = ours(backend)
        want = sorted(k.split('.', 2)[2] for k in g if k.startswith('val.%s.' % name))
        assert sorted(vals) == want, name
        for k, v in vals.items():
            assert v.dtype == np.float64 and v.shape == g['val.%s.%s' % (name, k)].shape
            gate('%s %s' % (name, k), v, g['val.%s.%s' % (name, k)], g['dev32v.%s.%s' % (name, k)])
        for k, v in grads.items():
            if 'grad.%s.%s' % (name, k) not in g:
                assert v is None, (name, k)            # hit_prob_nr[_fine]: detached
                continue
            gate('%s d %s' % (name, k), v, g['grad.%s.%s' % (name, k)], g['dev32g.%s.%s' % (name, k)])


# ---- larger shapes against the composition ------------------------------------------------------------------------------------------
def against_composition(name, comp, ours, backend):
    v64, g64 = comp(torch.float64)
    v32, g32 = comp(torch.float32)
    vals, grads = ours(backend)
    assert list(vals) == list(v64)
    for k in v64:
        gate('%s %s' % (name, k), vals[k], v64[k], np.abs(v32[k] - v64[k]).max())
    for k in g64:
        if g64[k] is None:
            assert grads[k] is None
            continue
        gate('%s d %s' % (name, k), grads[k], g64[k], np.abs(g32[k] - g64[k]).max())


SHAPES = {
    # config 4 (ft: render + consist, 512 rays, 64 + 64 samples), config 5 (gen: render + depth, 8 views, 8192 coordinates, 416 x 608)
    'hip': dict(rn=512, dn=64, rfn=8, pn=8192, h=416, w=608),
    'emu': dict(rn=700, dn=20, rfn=3, pn=4500, h=70, w=52),
}


@pytest.mark.parametrize('backend', BACKENDS)
def test_render_and_consist_call_at_the_finetuning_shape(backend):
    s = SHAPES[backend]
    case = lc.render_inputs(41, 1, s['rn'], suffixes=('nr', 'nr_fine'))
    against_composition('render', lambda dt: render_composition(case, True, dt), lambda be: render_ours(case, True, be), backend)
    case = lc.consist_inputs(42, 1, s['rn'], s['dn'])
    against_composition('consist', lambda dt: consist_composition(case, dt), lambda be: consist_ours(case, be), backend)


@pytest.mark.parametrize('loss_type', ['l2', 'smooth_l1'])
@pytest.mark.parametrize('backend', BACKENDS)
def test_depth_call_at_the_generalisation_shape(backend, loss_type):
    s = SHAPES[backend]
    for gso, int_coords in ((True, True), (False, False), (False, True)):
        case = lc.depth_inputs(43 + gso, s['rfn'], s['pn'], s['h'], s['w'], gso, int_coords)
        against_composition('depth gso=%d int=%d' % (gso, int_coords), lambda dt: depth_composition(case, loss_type, dt),
                            lambda be: depth_ours(case, loss_type, be), backend)


@pytest.mark.parametrize('backend', BACKENDS)
def test_validation_call_on_a_whole_image_under_no_grad(backend):
    """RenderLoss as the trainer's validation runs it: every ray of an image, no gradient (800 x 800 on the MI355X)"""
    rn = 640000 if backend == 'hip' else 9000
    case = lc.render_inputs(45, 1, rn)
    eng = engine(backend)
    data, leaves = render_data(case, torch.float32, eng.device)
    calls = count_calls(eng)
    with torch.no_grad():
        out = nloss.RenderLoss({'use_ray_mask': True, **FULL}, engine=eng)(data, {}, 0)
    assert calls == {'fwd': 1, 'bwd': 0}
    assert all(not v.requires_grad and v.shape == (1,) and v.dtype == torch.float32 for v in out.values())
    v64, _ = render_composition(case, True, torch.float64)
    v32, _ = render_composition(case, True, torch.float32)
    for k in v64:
        gate('validation %s' % k, out[k].cpu().double().numpy(), v64[k], np.abs(v32[k] - v64[k]).max())


# ---- exact properties ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    assert list(a[0]) == list(b[0])
    for k in a[0]:
        assert a[0][k].tobytes() == b[0][k].tobytes(), k
    for k in a[1]:
        assert (a[1][k] is None and b[1][k] is None) or a[1][k].tobytes() == b[1][k].tobytes(), k


@pytest.mark.parametrize('backend', BACKENDS)
def test_two_runs_are_bitwise_equal(backend):
    for name, case, _, ours in cases()[::2]:
        same(ours(backend), ours(backend))


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_term_does_not_depend_on_the_other_terms_of_the_launch(backend):
    case = lc.render_inputs(51, 2, 2500)
    four = render_ours(case, True, backend)
    for s in ('dr', 'dr_fine', 'nr_fine'):
        sub = {k: v for k, v in case.items() if not k.startswith('pixel_colors_') or k in ('pixel_colors_gt', 'pixel_colors_nr', 'pixel_colors_' + s)}
        two = render_ours(sub, True, backend)
        for key in ('nr', s):
            assert two[0]['loss_rgb_' + key].tobytes() == four[0]['loss_rgb_' + key].tobytes(), (s, key)
            assert two[1]['pixel_colors_' + key].tobytes() == four[1]['pixel_colors_' + key].tobytes(), (s, key)
    case = lc.depth_inputs(52, 3, 2300, 40, 30, True, True)
    both = depth_ours(case, 'l2', backend)
    alone = depth_ours({**case, 'pr': {'mean': case['pr']['mean']}}, 'l2', backend)
    assert alone[0]['loss_depth'].tobytes() == both[0]['loss_depth'].tobytes()
    assert alone[1]['mean'].tobytes() == both[1]['mean'].tobytes()
    case = lc.consist_inputs(53, 2, 300, 16)
    both = consist_ours(case, backend)
    alone = consist_ours({k: v for k, v in case.items() if not k.endswith('_fine')}, backend)
    assert alone[0]['loss_prob'].tobytes() == both[0]['loss_prob'].tobytes()
    assert alone[1]['hit_prob_self'].tobytes() == both[1]['hit_prob_self'].tobytes()


@pytest.mark.parametrize('backend', BACKENDS)
def test_masks_give_exact_zeros(backend):
    case = lc.render_inputs(54, 2, 600)
    vals, grads = render_ours(case, True, backend)
    off = ~case['ray_mask']
    assert off.any()
    for k, g in grads.items():
        assert (g[off] == 0).all() and (g[~off] != 0).any(), k
    case['ray_mask'][:] = False
    vals, grads = render_ours(case, True, backend)
    assert all((v == 0).all() for v in vals.values()) and all((g == 0).all() for g in grads.values())
    # the reference multiplies by the mask: a non-finite colour under a zero mask is still NaN (row 0 only)
    case['pixel_colors_nr'][0, 5, 1] = np.inf
    vals, _ = render_ours(case, True, backend)
    assert np.isnan(vals['loss_rgb_nr'][0]) and vals['loss_rgb_nr'][1] == 0 and (vals['loss_rgb_dr'] == 0).all()


@pytest.mark.parametrize('backend', BACKENDS)
def test_consistency_loss_quirks(backend):
    """hit_prob_nr gets no gradient although it requires one; use_ray_mask changes nothing; {} without hit_prob_self"""
    case = lc.consist_inputs(55, 2, 50, 12)
    a = consist_ours(case, backend)
    assert a[1]['hit_prob_nr'] is None and a[1]['hit_prob_nr_fine'] is None and a[1]['hit_prob_self'] is not None
    same(a, consist_ours(case, backend, {'use_ray_mask': True}))
    eng = engine(backend)
    calls = count_calls(eng)
    assert nloss.ConsistencyLoss({}, engine=eng)({'hit_prob_nr': torch.zeros(1, 4, 4)}, {}, 0) == {}
    assert calls == {'fwd': 0, 'bwd': 0}


@pytest.mark.parametrize('backend', BACKENDS)
def test_depth_loss_without_true_depth_launches_nothing(backend):
    eng = engine(backend)
    calls = count_calls(eng)
    out = nloss.DepthLoss({}, engine=eng)({'pixel_colors_nr': torch.zeros(1, 4, 3, device=eng.device)}, {'ref_imgs_info': {}}, 0)
    assert calls == {'fwd': 0, 'bwd': 0}
    assert list(out) == ['loss_depth'] and out['loss_depth'].shape == (1,) and out['loss_depth'].dtype == torch.float32
    assert out['loss_depth'].device == eng.device and float(out['loss_depth']) == 0.0
    np.testing.assert_array_equal(golden()['val.depth_none.loss_depth'], out['loss_depth'].cpu().numpy())


# ---- launch budget --------------------------------------------------------------------------------------------------------------------
def count_calls(eng):
    """wrap the engine's two entry points (idempotent): -> the live counter dict"""
    if not hasattr(eng, '_loss_calls'):
        eng._loss_calls = {'fwd': 0, 'bwd': 0}
        fwd, bwd = eng.train_loss, eng.train_loss_backward

        def train_loss(*a, **k):
            eng._loss_calls['fwd'] += 1
            return fwd(*a, **k)

        def train_loss_backward(*a, **k):
            eng._loss_calls['bwd'] += 1
            return bwd(*a, **k)
        eng.train_loss, eng.train_loss_backward = train_loss, train_loss_backward
    eng._loss_calls.update(fwd=0, bwd=0)
    return eng._loss_calls


@pytest.mark.parametrize('backend', BACKENDS)
def test_one_forward_and_at_most_one_backward_call_per_loss_call(backend):
    eng = engine(backend)
    calls = count_calls(eng)
    render_ours(lc.render_inputs(56, 1, 300), True, backend)          # four terms, total.backward()
    assert calls == {'fwd': 1, 'bwd': 1}
    calls.update(fwd=0, bwd=0)
    depth_ours(lc.depth_inputs(57, 2, 300, 30, 20, True, True), 'l2', backend)
    assert calls == {'fwd': 1, 'bwd': 1}
    calls.update(fwd=0, bwd=0)
    consist_ours(lc.consist_inputs(58, 1, 64, 8), backend)
    assert calls == {'fwd': 1, 'bwd': 1}
    calls.update(fwd=0, bwd=0)
    data, _ = render_data(lc.render_inputs(59, 1, 300), torch.float32, eng.device)
    out = nloss.RenderLoss(FULL, engine=eng)({k: v.detach() for k, v in data.items()}, {}, 0)      # nothing requires grad
    assert calls == {'fwd': 1, 'bwd': 0} and not out['loss_rgb_nr'].requires_grad


def test_total_loss_is_the_trainers_sum():
    eng = engine('emu')
    data, leaves = render_data(lc.render_inputs(60, 1, 200), torch.float32, eng.device)
    cdata, cleaves = consist_data(lc.consist_inputs(61, 1, 200, 8), torch.float32, eng.device)
    losses = [nloss.name2loss[n]({**FULL}, engine=eng) for n in ('render', 'consist')]
    total, info = nloss.total_loss(losses, {**data, **cdata}, {}, 0)
    assert sorted(info) == ['loss_prob', 'loss_prob_fine', 'loss_rgb_dr', 'loss_rgb_dr_fine', 'loss_rgb_nr', 'loss_rgb_nr_fine']
    want = 0
    for k, v in info.items():
        want = want + torch.mean(v)
    assert float(total.detach()) == float(want.detach()) and total.requires_grad
    total.backward()
    assert all(v.grad is not None for v in leaves.values()) and cleaves['hit_prob_self'].grad is not None and cleaves['hit_prob_nr'].grad is None


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    eng = engine('emu')
    data, _ = render_data(lc.render_inputs(62, 1, 64), torch.float32, eng.device)
    loss = nloss.RenderLoss({}, engine=eng)
    for dtype in (torch.float64, torch.float16):
        with pytest.raises(TypeError, match='float32'):
            loss({**data, 'pixel_colors_nr': data['pixel_colors_nr'].detach().to(dtype)}, {}, 0)
        with pytest.raises(TypeError, match='float32'):
            loss({**data, 'pixel_colors_gt': data['pixel_colors_gt'].to(dtype)}, {}, 0)
    with pytest.raises(NotImplementedError, match='requires grad'):
        loss({**data, 'pixel_colors_gt': data['pixel_colors_gt'].clone().requires_grad_(True)}, {}, 0)
    data_pr, data_gt, _ = lc.depth_data(lc.depth_inputs(63, 2, 100, 20, 30, True, True))
    dl = nloss.DepthLoss({}, engine=eng)
    for key in ('true_depth', 'depth', 'depth_range'):
        info = {**data_gt['ref_imgs_info'], key: data_gt['ref_imgs_info'][key].clone().requires_grad_(True)}
        with pytest.raises(NotImplementedError, match='requires grad'):
            dl(data_pr, {**data_gt, 'ref_imgs_info': info}, 0)
    with pytest.raises(TypeError):
        dl({**data_pr, 'depth_coords': data_pr['depth_coords'].double()}, data_gt, 0)
    out = loss(data, {}, 0)
    with pytest.raises(RuntimeError):                   # once differentiable
        g, = torch.autograd.grad(out['loss_rgb_nr'].sum(), data['pixel_colors_nr'], create_graph=True)
        g.sum().backward()
    # the C ABI's own argument errors
    from neuray_amd.engine import LossTerm
    t = LossTerm(eng.device, 'depth', torch.zeros(1, 4), torch.ones(1, 1, 1, 5), coords=torch.zeros(1, 4, 2), depth_range=torch.ones(1, 2))
    with pytest.raises(RuntimeError, match='at least 2 x 2'):
        eng.train_loss([t])
    t = LossTerm(eng.device, 'render', torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    t.kind = 7
    with pytest.raises(RuntimeError, match='unknown kind'):
        eng.train_loss([t])
    t.kind, t.rows = 0, 0
    with pytest.raises(RuntimeError, match='0 rows'):
        eng.train_loss([t])
    with pytest.raises(ValueError):
        eng.train_loss([])


def test_losses_without_an_engine_need_the_gpu():
    """no host fallback: on CPU tensors the drop-in asks for the HIP engine, which refuses a CPU device"""
    data, _ = render_data(lc.render_inputs(64, 1, 16), torch.float32, 'cpu')
    with pytest.raises(RuntimeError, match='HIP device'):
        nloss.RenderLoss({})(data, {}, 0)
