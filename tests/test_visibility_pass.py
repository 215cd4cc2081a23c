"""cfg['hip_coarse_pass'] = 'visibility' (csrc/nr_kernels_vis.h): the coarse hit probabilities from the input views'
visibility alone - predict_alpha_values_dr + decode_alpha_value + alpha_values2hit_prob (network/renderer.py:85-94,121-123), the
hit_prob_dr of direct rendering - without the aggregation network and without the per-(point, view) record.

Gates.  Against the reference's own hit_prob_dr (tests/golden/case_f_dr.npz): 1e-4, the project's hit_prob tolerance.  Against the existing
route on the same device - direct_render on the point kernel's per-view record - alpha and hit_prob bit for bit: the new kernel runs the
point kernel's device functions in its operation order and dr_points_kernel's cross-view sum literally.  ray_mask is integer logic: equal
to the network pass's.  The mode end to end: the fine pass against the oracle placed on the kernel's own coarse hit_prob, at the bound of
test_render_parity.test_fine_pass_on_reference_fine_depths for the oracle on identical inputs (atol 1e-5)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import load_case, load_weights, oracle_cfg
from emu_util import emu_lib, to_torch
from oracle import neuray_oracle as orc
from test_render_parity import BACKENDS, TOL_HIT, make_renderer
from neuray_amd import _lib, synthetic
from neuray_amd.engine import RenderEngine
from neuray_amd.network.renderer import NeuralRayBaseRenderer

GROUND = -15.0
RN = 19                                       # two ray blocks of the kernel's tiling, the second one partial
RFNS, DNS = (1, 3, 8, 9, 16), (3, 16, 64)
# (decoder has a vis head, cfg use_vis); rotated over the (rfn, dn) grid so that every rfn and every dn meets every one of them
DECODERS = ((False, False), (True, True), (True, False))
GRID = [(rfn, dn) + DECODERS[(i + j) % 3] for i, rfn in enumerate(RFNS) for j, dn in enumerate(DNS)]


def engine_for(backend):
    dev = 'cpu' if backend == 'emu' else 'cuda:0'
    return RenderEngine(dev, _test_lib=emu_lib() if backend == 'emu' else None), dev


@functools.lru_cache(None)
def scene(rfn):
    """synthetic.make_scene at toy size with the wide depth range of case f_dr: samples in front of, inside and behind every view's image"""
    que, ref = synthetic.make_scene(48, 48, rfn, seed=3, depth_range=(0.8, 9.0))
    que['coords'] = (np.random.RandomState(3).rand(1, RN, 2) * 47).astype(np.float32)
    que['coords'][0, 16:] = [[0.5, 0.5], [1.0, 0.7], [0.3, 1.2]]      # the partial ray block sits in one corner: it leaves some view's image whole
    que['Ks_inv'] = torch.inverse(torch.from_numpy(que['Ks'])).numpy()        # (as the engine's host_inverse: the masks are bit-exact)
    return que, ref


@functools.lru_cache(None)
def seeded_state(vis_head):
    """seeded random weights of a coarse pass, the unfolded pack's source (with or without a vis head on the decoder)"""
    torch.manual_seed(11)
    r = NeuralRayBaseRenderer({'dist_decoder_cfg': {'use_vis': vis_head}})
    sd = {'d.' + k: v for k, v in r.dist_decoder.state_dict().items()}
    sd.update({'a.' + k: v for k, v in r.agg_net.state_dict().items()})
    assert ('d.vis_decoder.0.weight' in sd) == vis_head
    return sd


def oracle_masks(que, ref, dn):
    """[rfn, rn, dn] validity of every (view, sample point), on the CPU"""
    depth = orc.sample_depth(que['depth_range'], RN, dn)
    pts, _ = orc.depth2points(que['coords'], que['poses'], que['Ks_inv'], depth)
    h, w = ref['imgs'].shape[-2:]
    valid = orc.project_points_ref_views(ref['poses'], ref['Ks'], h, w, pts.reshape(-1, 3))[3]
    return valid.reshape(-1, RN, dn), depth


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_visibility_pass_matches_the_reference_hit_prob_dr(backend):
    cfg, que, ref, out, mid, extra = load_case('f_dr')
    r, dev = make_renderer({k: v for k, v in cfg.items() if k != 'use_dr_prediction'}, load_weights(False), backend)
    eng = r.engine(dev)
    tq, tr = to_torch(que, dev), to_torch(ref, dev)
    depth = eng.sample_coarse_depth(tq['depth_range'], que['coords'].shape[1], cfg['depth_sample_num'])
    got = eng.visibility_pass(eng.prepare_query(tq), eng.prepare_views(tr), tq['coords'][0], depth, r._packed_pass(eng, False),
                              use_vis=cfg['dist_decoder_cfg']['use_vis'], ground=GROUND)
    err = np.abs(got['hit_prob'].cpu().numpy() - out['hit_prob_dr'][0]).max()
    print('hit_prob against the reference hit_prob_dr [%s]: %.2e' % (backend, err))
    assert err <= TOL_HIT
    assert np.array_equal(got['ray_mask'].cpu().numpy(), out['ray_mask'][0])


# ---- 2. against the existing route, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('rfn,dn,vis_head,use_vis', GRID)
def test_visibility_pass_equals_direct_render_on_the_per_view_record(rfn, dn, vis_head, use_vis, backend):
    que, ref = scene(rfn)
    # the inputs exercise what the test is about: the ground-state branch, partial visibility, a skipped (tile, view) slot
    valid, _ = oracle_masks(que, ref, dn)
    seen = valid.sum(0)
    assert (seen == 0).any()
    assert rfn == 1 or ((seen > 0) & (seen < rfn)).any()
    blocks = [valid[:, b:b + 16] for b in range(0, RN, 16)]                  # the kernel's tiles: one sample of 16 neighbouring rays
    assert any((~blk.any(1)).any() for blk in blocks)

    eng, dev = engine_for(backend)
    tq, tr = to_torch(que, dev), to_torch(ref, dev)
    qc, views = eng.prepare_query(tq), eng.prepare_views(tr)
    depth = eng.sample_coarse_depth(tq['depth_range'], RN, dn)
    packed = eng.pack_pass(seeded_state(vis_head), 'd.', 'a.', fold=False)
    assert packed.has_vis_head == vis_head
    net = eng.render_pass(qc, views, tq['coords'][0], depth, packed, use_vis=use_vis, want_dbg=True)
    want = eng.direct_render(qc, views, tq['coords'][0], depth, net['dbg'], torch.from_numpy(orc.SPH_REGS), ground=GROUND)
    got = eng.visibility_pass(qc, views, tq['coords'][0], depth, packed, use_vis=use_vis, ground=GROUND)
    for k in ('alpha', 'hit_prob'):
        a, b = got[k].cpu().numpy(), want[k].cpu().numpy()
        assert np.all(np.isfinite(a))
        assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))
    assert np.array_equal(got['ray_mask'].cpu().numpy(), net['ray_mask'].cpu().numpy())
    assert np.array_equal(got['nvalid'].cpu().numpy(), seen.astype(np.int32))
    assert np.array_equal(got['alpha'].cpu().numpy()[seen == 0], np.full(int((seen == 0).sum()), GROUND, np.float32))


# ---- 3. the mode end to end -------------------------------------------------------------------------------------------------------
def visibility_case(backend, **override):
    cfg, que, ref, out, mid, extra = load_case('f_dr')
    cfg = {**{k: v for k, v in cfg.items() if k != 'use_dr_prediction'}, 'hip_coarse_pass': 'visibility', **override}
    weights = load_weights(False)
    r, dev = make_renderer(cfg, weights, backend)
    return cfg, que, ref, out, weights, r, dev


@pytest.mark.parametrize('backend', BACKENDS)
def test_visibility_mode_renders_the_fine_pass_on_its_own_coarse_hit_prob(backend):
    cfg, que, ref, out, weights, r, dev = visibility_case(backend)
    tq, tr = to_torch(que, dev), to_torch(ref, dev)
    with torch.no_grad():
        got = {k: v.cpu().numpy() for k, v in r.render_impl(tq, tr, False).items()}
    assert set(got) == {'hit_prob_dr', 'ray_mask', 'pixel_colors_nr_fine', 'hit_prob_nr_fine', 'ray_mask_fine'}
    assert 'pixel_colors_nr' not in got
    assert np.abs(got['hit_prob_dr'] - out['hit_prob_dr']).max() <= TOL_HIT
    # the oracle places its fine samples from the kernel's coarse hit_prob (its test hook): only the fine pass is compared
    ocfg = oracle_cfg({**orc.DEFAULT_CFG, **{k: v for k, v in cfg.items() if not k.startswith('hip_')}})
    want = orc.render_impl(weights, ocfg, que, ref, coarse_hit_prob=got['hit_prob_dr'])
    err = np.abs(got['pixel_colors_nr_fine'] - want['pixel_colors_nr_fine']).max()
    print('fine pass on the visibility hit_prob [%s]: pixel err %.2e' % (backend, err))
    np.testing.assert_allclose(got['pixel_colors_nr_fine'], want['pixel_colors_nr_fine'], atol=1e-5)
    np.testing.assert_allclose(got['hit_prob_nr_fine'], want['hit_prob_nr_fine'], atol=TOL_HIT)
    assert np.array_equal(got['ray_mask_fine'], want['ray_mask_fine'])
    # a query with images adds the ground-truth colours, as in the network mode; render() drops every hit_prob* at inference
    tq2 = {k: v for k, v in tq.items() if not k.startswith('_')}
    tq2['imgs'] = tr['imgs'][:1]
    with torch.no_grad():
        got2 = r.render_impl(tq2, tr, False)
        assert set(got2) == set(got) | {'pixel_colors_gt', 'pixel_colors_gt_fine'}
        assert set(r.render(tq2, tr, False)) == {'ray_mask', 'pixel_colors_nr_fine', 'ray_mask_fine', 'pixel_colors_gt', 'pixel_colors_gt_fine'}


@pytest.mark.parametrize('backend', BACKENDS)
def test_visibility_mode_is_independent_of_batching(backend):
    cfg, que, ref, out, weights, r, dev = visibility_case(backend)
    tq, tr = to_torch(que, dev), to_torch(ref, dev)
    with torch.no_grad():
        full = r.render_impl(tq, tr, False)
        parts = []
        for sl in (slice(0, 21), slice(21, None)):                          # neither part a multiple of the 16-ray tile
            sub = {k: v for k, v in tq.items() if not k.startswith('_')}
            sub['coords'] = tq['coords'][:, sl]
            parts.append(r.render_impl(sub, tr, False))
    for k, v in full.items():
        assert torch.equal(v, torch.cat([p[k] for p in parts], 1)), k
    # sharded rendering (parallel.py): every rank's contiguous ray range through render(), the tiles put back together
    from neuray_amd import parallel
    with torch.no_grad():
        whole = r.render({k: v for k, v in tq.items() if not k.startswith('_')}, tr, False)
        shards = [parallel.render_ray_shard(r, {k: v for k, v in tq.items() if not k.startswith('_')}, tr, rank, 3)[0] for rank in range(3)]
    assert set(whole) == {'ray_mask', 'pixel_colors_nr_fine', 'ray_mask_fine'}
    for k, v in whole.items():
        assert torch.equal(v, torch.cat([sh[k] for sh in shards], 1)) and torch.equal(v, full[k]), k


@pytest.mark.parametrize('backend', BACKENDS)
def test_visibility_mode_keeps_multi_view_queries_and_training_style_uniforms(backend):
    cfg, que, ref, out, weights, r, dev = visibility_case(backend)
    tq, tr = to_torch(que, dev), to_torch(ref, dev)
    with torch.no_grad():
        one = r.render_impl(tq, tr, False)
        tq2 = {k: torch.cat([v, v], 0) for k, v in tq.items() if not k.startswith('_')}
        two = r.render_impl(tq2, tr, False)                                   # qn = 2: the per-view loop
        for k, v in one.items():
            assert torch.equal(two[k][0:1], v) and torch.equal(two[k][1:2], v), k
        torch.manual_seed(5)
        tr_like = r.render_impl({k: v for k, v in tq.items() if not k.startswith('_')}, tr, True)       # is_train under no_grad
    assert set(tr_like) == set(one)
    assert torch.equal(tr_like['hit_prob_dr'], one['hit_prob_dr']) and not torch.equal(tr_like['hit_prob_nr_fine'], one['hit_prob_nr_fine'])


# ---- 4. switches and refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_network_is_the_default_and_the_environment_wins(backend, monkeypatch):
    monkeypatch.delenv('NEURAY_HIP_COARSE', raising=False)
    cfg, que, ref, out, mid, extra = load_case('a_small')
    weights = load_weights(False)

    def render(c):
        r, dev = make_renderer(c, weights, backend)
        with torch.no_grad():
            return {k: v.cpu().numpy() for k, v in r.render_impl(to_torch(que, dev), to_torch(ref, dev), False).items()}
    assert 'hip_coarse_pass' not in cfg
    plain = render(cfg)
    named = render({**cfg, 'hip_coarse_pass': 'network'})
    assert set(plain) == set(named) and 'pixel_colors_nr' in plain
    for k in plain:
        assert np.array_equal(plain[k], named[k]), k
    monkeypatch.setenv('NEURAY_HIP_COARSE', 'visibility')
    vis = render({**cfg, 'hip_coarse_pass': 'network'})                        # the environment wins over the cfg ...
    assert 'pixel_colors_nr' not in vis and 'hit_prob_dr' in vis
    monkeypatch.setenv('NEURAY_HIP_COARSE', 'network')
    net = render({**cfg, 'hip_coarse_pass': 'visibility'})                     # ... in both directions
    for k in plain:
        assert np.array_equal(plain[k], net[k]), k
    monkeypatch.setenv('NEURAY_HIP_COARSE', 'coarse')
    with pytest.raises(ValueError):
        render(cfg)


def test_visibility_mode_refuses_what_it_cannot_serve(monkeypatch):
    monkeypatch.delenv('NEURAY_HIP_COARSE', raising=False)
    cfg, que, ref, out, mid, extra = load_case('f_dr')
    base = {**{k: v for k, v in cfg.items() if k != 'use_dr_prediction'}, 'hip_coarse_pass': 'visibility'}
    weights = load_weights(False)
    tq, tr = to_torch(que, 'cpu'), to_torch(ref, 'cpu')

    def run(c, grad=False, w=weights):
        r = NeuralRayBaseRenderer(c)
        r.load_state_dict({k: torch.from_numpy(v) for k, v in w.items() if k in r.state_dict()}, strict=True)
        r._engine_test_lib = emu_lib()
        with torch.enable_grad() if grad else torch.no_grad():
            return r.render_impl({k: v for k, v in tq.items()}, {k: v for k, v in tr.items()}, False)
    with pytest.raises(ValueError, match='use_hierarchical_sampling'):        # no pass left that renders colours
        run({**base, 'use_hierarchical_sampling': False})
    with pytest.raises(NotImplementedError, match='use_dr_prediction'):
        run({**base, 'use_dr_prediction': True})
    with pytest.raises(NotImplementedError, match='inference only'):          # a grad-enabled pass that needs gradients
        run(base, grad=True)
    with pytest.raises(NotImplementedError, match='hip_variant'):
        run({**base, 'hip_variant': 'bf16'})
    with pytest.raises(ValueError, match='hip_coarse_pass'):
        run({**base, 'hip_coarse_pass': 'visible'})
    assert set(run(base)) == {'hit_prob_dr', 'ray_mask', 'pixel_colors_nr_fine', 'hit_prob_nr_fine', 'ray_mask_fine'}


def test_patch_reference_carries_the_mode_onto_a_grafted_class():
    """integrate.patch_renderer_class (what patch_reference applies to the reference's class) grafts HOT_PATH_METHODS: a class that has none of the HIP path's methods renders in the mode"""
    from neuray_amd import integrate
    from neuray_amd.network.hip_path import HOT_PATH_METHODS
    assert {'_coarse_pass_mode', '_visibility_coarse', 'render_impl'} <= set(HOT_PATH_METHODS)
    cfg, que, ref, out, weights, r, dev = visibility_case('emu')

    class Host(torch.nn.Module):                      # what the reference's constructor leaves: cfg + the four modules
        def __init__(self, src):
            super().__init__()
            self.cfg = dict(src.cfg)
            self.dist_decoder, self.agg_net = src.dist_decoder, src.agg_net
            self.fine_dist_decoder, self.fine_agg_net = src.fine_dist_decoder, src.fine_agg_net
    integrate.patch_renderer_class(Host)
    try:
        host = Host(r).eval()
        host._engine_test_lib = emu_lib()
        with torch.no_grad():
            got = host.render_impl(to_torch(que, 'cpu'), to_torch(ref, 'cpu'), False)
            want = r.render_impl(to_torch(que, 'cpu'), to_torch(ref, 'cpu'), False)
    finally:
        integrate.unpatch_renderer_class(Host)
    assert set(got) == set(want) and 'pixel_colors_nr' not in got
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---- 5. C-level argument checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_visibility_entries_check_their_arguments(backend):
    eng, dev = engine_for(backend)
    que, ref = scene(3)
    tq, tr = to_torch(que, dev), to_torch(ref, dev)
    qc, views = eng.prepare_query(tq), eng.prepare_views(tr)
    dn = 16
    depth = eng.sample_coarse_depth(tq['depth_range'], RN, dn)
    packed = eng.pack_pass(seeded_state(False), 'd.', 'a.', fold=False)
    alpha = torch.full((RN, dn), 7.0, device=dev)
    nvalid = torch.full((RN, dn), -1, dtype=torch.int32, device=dev)
    coords = tq['coords'][0].contiguous()

    def args(**kw):
        v = dict(query_const_dev=qc.data_ptr(), view_const_dev=views.view_const.data_ptr(), coords_dev=coords.data_ptr(),
                 depth_dev=depth.data_ptr(), ray_feats_nhwc_dev=views.ray_feats.data_ptr(), packed_weights_dev=packed.dev.data_ptr(),
                 rfn=views.rfn, rn=RN, dn=dn, h=views.h, w=views.w, fh=views.fh, fw=views.fw, has_vis_head=0, use_vis=0, var_bias=0.05,
                 ground=GROUND, alpha_dev=alpha.data_ptr(), nvalid_dev=nvalid.data_ptr())
        v.update(kw)
        return _lib.NeurayVisibilityArgs(**v)

    def refused(rc, word):
        msg = eng.lib.neuray_last_error().decode()
        assert rc != 0 and msg.startswith('neuray_visibility_') and word in msg, (rc, msg)
    s = eng._stream()
    refused(eng.lib.neuray_visibility_points(C.byref(args(rfn=0)), s), 'rfn=0')
    refused(eng.lib.neuray_visibility_points(C.byref(args(rfn=17)), s), 'rfn=17')
    refused(eng.lib.neuray_visibility_points(C.byref(args(dn=2)), s), 'dn=2')
    refused(eng.lib.neuray_visibility_points(C.byref(args(alpha_dev=None)), s), 'alpha_dev')
    refused(eng.lib.neuray_visibility_points(C.byref(args(nvalid_dev=None)), s), 'nvalid_dev')
    refused(eng.lib.neuray_visibility_points(C.byref(args(use_vis=1)), s), 'vis head')
    refused(eng.lib.neuray_visibility_points(None, s), 'null args')
    hit = torch.full((RN, dn), 7.0, device=dev)
    refused(eng.lib.neuray_visibility_rays(alpha.data_ptr(), nvalid.data_ptr(), RN, dn, 2, 8, None, None, s), 'hit_prob')
    refused(eng.lib.neuray_visibility_rays(None, nvalid.data_ptr(), RN, dn, 2, 8, hit.data_ptr(), None, s), 'alpha')
    refused(eng.lib.neuray_visibility_rays(alpha.data_ptr(), nvalid.data_ptr(), 0, dn, 2, 8, hit.data_ptr(), None, s), 'rn=0')
    if dev != 'cpu':
        torch.cuda.synchronize()
    # nothing was launched: the outputs still hold their fill values
    assert bool((alpha == 7.0).all()) and bool((nvalid == -1).all()) and bool((hit == 7.0).all())
    # ... and the same arguments without a fault are accepted
    assert eng.lib.neuray_visibility_points(C.byref(args()), s) == 0
    assert eng.lib.neuray_visibility_rays(alpha.data_ptr(), nvalid.data_ptr(), RN, dn, 2, 8, hit.data_ptr(), None, s) == 0
    assert bool((nvalid >= 0).all()) and bool((hit <= 1.0).all())
