"""Geometry export (neuray_amd/geometry.py, csrc/nr_kernels_fuse.h): the depth consistency kernel against the float64
reference, the fusion stage against its integer logic, properties of the fused cloud on procedural scenes (distance to the true surface,
normals, de-duplication, determinism, outlier rejection, an empty view) and the public surface (PLY, filter_depth, render_depth_maps, the
command line, argument errors).

Cases: 5 views of 40 x 56 (partial tiles both ways) of three procedural scenes, depth and colour from render_numpy(float64), with S = 4 (all
other views) and with two sources per view in a table padded with -1 and one self entry.

Near-threshold (pixel, slot) pairs are left out of the discrete comparisons: u + 0.5 or v + 0.5 within 2e-4 of an integer, |z| < 1e-4,
|e_px - tau_px| < 1e-3, |e_d - tau_d| < 1e-5, |(z - d_j) / d_j - tau_d| < 1e-5; at most 0.5 % of a case's valid pairs (measured: 0.13 ..
0.19 %).

Tolerances.  They come from the reference alone: the float32 evaluation against the float64 evaluation of the same formulas on the six cases
(test_reference_float32_agrees_with_float64 measures and asserts them on the CPU; the discrete outputs differed in 0 places).  Worst values
measured: fused_depth 1.95e-7 relative; with the same bits and texels, xyz 6.40e-7, colour 9.54e-8, normal 1.26e-5 absolute (normals
where the reference's cross product exceeds 1e-3 x the product of the two difference lengths).  The gates are 4 x these."""
import functools
import os

import numpy as np
import pytest
import torch

from emu_util import emu_lib
from test_procedural import hand_prims
from neuray_amd import geometry as geo, procedural as proc, synthetic
from neuray_amd.engine import RenderEngine

BACKENDS = ['emu', pytest.param('hip', marks=pytest.mark.gpu)]
H, W, N = 40, 56, 5
ANGLES = ((20.0, 25.0), (60.0, 35.0), (100.0, 20.0), (140.0, 40.0), (340.0, 30.0))
TAU_PX, TAU_D, MIN_VIEWS, TAU_N = 1.0, 0.01, 2, 0.05
MAX_LEFT_OUT = 0.005
REF_FD_ERR, REF_XYZ_ERR, REF_COLOUR_ERR, REF_NORMAL_ERR = 1.95e-7, 6.40e-7, 9.54e-8, 1.26e-5   # float32 reference against float64 reference
TOL_FD, TOL_XYZ, TOL_COLOUR, TOL_NORMAL = 4 * REF_FD_ERR, 4 * REF_XYZ_ERR, 4 * REF_COLOUR_ERR, 4 * REF_NORMAL_ERR
NORMAL_CROSS_REL = 1e-3
SCENES = ('generated7', 'generated3', 'hand')
TABLES = ('all', 'padded')
CASES = [(s, t) for s in SCENES for t in TABLES]
ALL_OUT = ('count', 'fused_depth', 'consistent_bits', 'occluded_bits', 'src_texel')


def engine_for(backend):
    dev = 'cpu' if backend == 'emu' else 'cuda:0'
    return RenderEngine(dev, _test_lib=emu_lib() if backend == 'emu' else None)


@functools.lru_cache(None)
def cameras():
    poses = np.stack([synthetic.look_at_pose(synthetic.sphere_pos(proc.CAMERA_RADIUS, a, e)) for a, e in ANGLES]).astype(np.float32)
    Ks = np.repeat(proc.intrinsics(H, W)[None], N, 0)
    for a in (poses, Ks):
        a.setflags(write=False)
    return poses, Ks


@functools.lru_cache(None)
def scene(name):
    if name == 'generated7':
        return proc.make_scene(7, 'black')
    if name == 'generated3':
        return proc.make_scene(3, 'white')
    if name == 'hand':                                     # mutual occluders (tests/test_procedural.py)
        return proc.pack_scene(hand_prims(), light=(0.3, -0.2, 1.0), ambient=0.35, background='white')
    raise KeyError(name)


@functools.lru_cache(None)
def table(name):
    if name == 'all':                                      # S = 4: every other view
        t = np.array([[j for j in range(N) if j != i] for i in range(N)], np.int32)
    else:                                                  # two sources, an empty slot and the view itself
        t = np.array([[(i + 1) % N, -1, i, (i + 3) % N] for i in range(N)], np.int32)
    t.setflags(write=False)
    return t


@functools.lru_cache(None)
def views(name):
    """depth [n,h,w] and colour [n,3,h,w] of the scene, float32 of render_numpy(float64); computed once, read-only"""
    poses, Ks = cameras()
    out = proc.render_numpy(scene(name), poses, Ks, H, W, 1)
    depth, rgb = out['depth'].astype(np.float32), out['rgb'].astype(np.float32)
    depth.setflags(write=False)
    rgb.setflags(write=False)
    return depth, rgb


@functools.lru_cache(None)
def reference(name, tab, dtype='float64'):
    poses, Ks = cameras()
    out = geo.consistency_numpy(views(name)[0], poses, Ks, table(tab), TAU_PX, TAU_D, dtype=np.dtype(dtype), details=dtype == 'float64')
    for v in out.values():
        v.setflags(write=False)
    return out


def near_threshold(ref):
    """[n,S,h,w] bool: the pairs the discrete comparisons leave out, and the share of the valid pairs they are"""
    with np.errstate(invalid='ignore'):
        def near_int(a):
            return np.abs(a + 0.5 - np.round(a + 0.5)) < 2e-4
        near = near_int(ref['u']) | near_int(ref['v']) | (np.abs(ref['z']) < 1e-4) | (np.abs(ref['e_px'] - TAU_PX) < 1e-3)
        near |= (np.abs(ref['e_d'] - np.float32(TAU_D)) < 1e-5) | (np.abs(ref['occ'] - np.float32(TAU_D)) < 1e-5)
    near &= ref['valid']
    return near, near.sum() / max(ref['valid'].sum(), 1)


def compare_consistency(got, ref, what):
    """the gates of test 1 on one case -> worst relative fused_depth error; got: dict of numpy arrays"""
    near, left_out = near_threshold(ref)
    assert left_out <= MAX_LEFT_OUT, (what, left_out)
    keep = ~near
    S = near.shape[1]
    assert np.array_equal(got['src_texel'][keep], ref['src_texel'][keep]), what
    for k in ('consistent_bits', 'occluded_bits'):
        for s in range(S):
            assert np.array_equal(((got[k] >> s) & 1)[keep[:, s]], ((ref[k] >> s) & 1)[keep[:, s]]), (what, k, s)
        assert np.all((got[k] >> S) == 0), (what, k)
    clean = ~near.any(1)
    assert np.array_equal(got['count'][clean], ref['count'][clean]), what
    assert np.all(np.isfinite(got['fused_depth'])), what
    has = ref['fused_depth'] > 0
    assert np.all(got['fused_depth'][~has] == 0), what
    sel = clean & has
    err = float(np.max(np.abs(got['fused_depth'][sel] - ref['fused_depth'][sel]) / ref['fused_depth'][sel]))
    print('%s: left out %.3f %% of %d pairs, fused_depth %.2e relative' % (what, 100 * left_out, ref['valid'].sum(), err))
    return err


@functools.lru_cache(None)
def kernel_consistency(backend, name, tab):
    """the kernel's result on one case, computed once per backend and shared (numpy arrays, read-only)"""
    poses, Ks = cameras()
    out = engine_for(backend).depth_consistency(views(name)[0], poses, Ks, table(tab), TAU_PX, TAU_D, outputs=ALL_OUT)
    assert out['count'].dtype == torch.uint8 and out['fused_depth'].dtype == torch.float32 and out['src_texel'].shape == (N, 4, H, W)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def kernel_fuse(backend, name, tab, cons=None, dedup=True, depth=None, snapshots=None):
    """-> dict of numpy arrays [n, ...] (emit, xyz, colour, normal) + the final taken masks"""
    poses, Ks = cameras()
    eng = engine_for(backend)
    d, rgb = views(name)
    d = d if depth is None else depth
    cons = kernel_consistency(backend, name, tab) if cons is None else cons
    dev_cons = {k: torch.from_numpy(np.ascontiguousarray(cons[k])).to(eng.device) for k in ('count', 'fused_depth', 'consistent_bits')}
    taken = torch.zeros(N, H, W, dtype=torch.uint8, device=eng.device) if dedup else None
    per_view = []
    for i in range(N):
        if snapshots is not None:
            snapshots.append(taken[i].cpu().numpy().copy())
        per_view.append(eng.fuse_view(i, d, rgb, poses, Ks, table(tab), dev_cons, taken, MIN_VIEWS, TAU_N))
    out = {k: np.stack([v[k].cpu().numpy() for v in per_view]) for k in ('emit', 'xyz', 'colour', 'normal')}
    out['taken'] = taken.cpu().numpy() if dedup else None
    return out


# ---- the reference against itself: where the tolerances come from -----------------------------------------------------------------
def test_reference_float32_agrees_with_float64():
    poses, Ks = cameras()
    worst = {'fd': 0.0, 'xyz': 0.0, 'colour': 0.0, 'normal': 0.0}
    for name, tab in CASES:
        ref, f32 = reference(name, tab), reference(name, tab, 'float32')
        worst['fd'] = max(worst['fd'], compare_consistency(f32, ref, 'float32 reference %s %s' % (name, tab)))
        assert 0.3 < (views(name)[0] > 0).mean() < 0.9 and (ref['count'] >= MIN_VIEWS).mean() > 0.05
        if tab == 'all':                                   # occlusion happens: some pairs see a nearer surface in the source
            assert (ref['occluded_bits'] != 0).mean() > 0.01
        depth, rgb = views(name)
        a = geo.fuse_numpy(depth, rgb, poses, Ks, table(tab), ref['consistent_bits'], ref['src_texel'], MIN_VIEWS, TAU_N)
        b = geo.fuse_numpy(depth, rgb, poses, Ks, table(tab), ref['consistent_bits'], ref['src_texel'], MIN_VIEWS, TAU_N, dtype=np.float32)
        assert np.array_equal(a['emit'], b['emit']) and np.array_equal(a['taken'], b['taken'])
        assert np.max(np.abs(a['fused_depth'] - ref['fused_depth'])) == 0          # recomputed from bits and texels: the same numbers
        e = a['emit'] > 0
        for k in ('xyz', 'colour', 'normal'):
            sel = e & (a['cross_rel'] > NORMAL_CROSS_REL) if k == 'normal' else e
            worst[k] = max(worst[k], float(np.abs(a[k] - b[k])[sel].max()))
    print('worst: fused_depth %.3e relative, xyz %.3e, colour %.3e, normal %.3e' % (worst['fd'], worst['xyz'], worst['colour'], worst['normal']))
    # the gates are 4 x what was measured when they were written down; the measurement still holds
    assert worst['fd'] <= REF_FD_ERR * 1.0001 and worst['xyz'] <= REF_XYZ_ERR * 1.0001
    assert worst['colour'] <= REF_COLOUR_ERR * 1.0001 and worst['normal'] <= REF_NORMAL_ERR * 1.0001


# ---- 1. the consistency kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name,tab', CASES)
def test_consistency_kernel_matches_the_float64_reference(name, tab, backend):
    got = kernel_consistency(backend, name, tab)
    err = compare_consistency(got, reference(name, tab), 'kernel [%s] %s %s' % (backend, name, tab))
    assert err <= TOL_FD
    if tab == 'padded':                                    # the empty slot and the self entry see nothing
        assert np.all(got['src_texel'][:, 1:3] == -1) and np.all((got['consistent_bits'] & 0b0110) == 0) and np.all((got['occluded_bits'] & 0b0110) == 0)


@pytest.mark.parametrize('backend', BACKENDS)
def test_optional_consistency_outputs_are_skipped(backend):
    poses, Ks = cameras()
    full = kernel_consistency(backend, 'hand', 'all')
    some = engine_for(backend).depth_consistency(views('hand')[0], poses, Ks, table('all'), TAU_PX, TAU_D, outputs=('count', 'occluded_bits'))
    assert set(some) == {'count', 'occluded_bits'}
    assert np.array_equal(some['count'].cpu().numpy(), full['count']) and np.array_equal(some['occluded_bits'].cpu().numpy(), full['occluded_bits'])


# ---- 2. the fuse stage, exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name,tab', CASES)
def test_fuse_stage_equals_the_integer_logic(name, tab, backend):
    """fuse_numpy is handed the kernel's own consistent_bits and src_texel: emit and taken are then integer logic and must be equal"""
    poses, Ks = cameras()
    cons = kernel_consistency(backend, name, tab)
    got = kernel_fuse(backend, name, tab)
    depth, rgb = views(name)
    want = geo.fuse_numpy(depth, rgb, poses, Ks, table(tab), cons['consistent_bits'], cons['src_texel'], MIN_VIEWS, TAU_N)
    assert np.array_equal(got['emit'], want['emit'])
    assert np.array_equal(got['taken'], want['taken'])
    e = want['emit'] > 0
    assert e.sum() > 300
    errs = {}
    for k in ('xyz', 'colour', 'normal'):
        assert np.all(np.isfinite(got[k])) and np.all(got[k][~e] == 0), k
        sel = e & (want['cross_rel'] > NORMAL_CROSS_REL) if k == 'normal' else e
        errs[k] = float(np.abs(got[k] - want[k])[sel].max())
    print('fuse [%s] %s %s: %d points, xyz %.2e, colour %.2e, normal %.2e' % (backend, name, tab, e.sum(), errs['xyz'], errs['colour'], errs['normal']))
    assert (e & (want['cross_rel'] > NORMAL_CROSS_REL)).sum() > 0.5 * e.sum()
    assert errs['xyz'] <= TOL_XYZ and errs['colour'] <= TOL_COLOUR and errs['normal'] <= TOL_NORMAL


# ---- 3. properties -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', SCENES)
def test_fused_points_lie_on_the_surface_and_normals_face_the_camera(name, backend):
    poses, Ks = cameras()
    got = kernel_fuse(backend, name, 'all')
    depth = views(name)[0]
    Ki = np.linalg.inv(Ks.astype(np.float64))
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    pix = np.stack([xs, ys, np.ones_like(xs)], -1).astype(np.float64)
    with_normal = 0
    for i in range(N):
        e = got['emit'][i] > 0
        # (a) every averaged depth lies within tau_d d of an exact on-surface depth along its ray
        ray_len = np.linalg.norm(pix @ Ki[i].T, axis=-1)
        dist = geo.surface_distance(scene(name), got['xyz'][i][e])
        assert np.all(dist <= (TAU_D * depth[i] * ray_len)[e] + 1e-4), (i, float(dist.max()))
        # (b) unit or zero, facing the camera
        nrm = got['normal'][i][e].astype(np.float64)
        length = np.linalg.norm(nrm, axis=-1)
        assert np.all((length == 0) | (np.abs(length - 1) < 1e-5))
        centre = -poses[i, :, :3].astype(np.float64).T @ poses[i, :, 3].astype(np.float64)
        assert np.all(np.sum(nrm * (got['xyz'][i][e] - centre), -1)[length > 0] < 0)
        with_normal += int((length > 0).sum())
    assert with_normal > 0.5 * (got['emit'] > 0).sum()


@pytest.mark.parametrize('backend', BACKENDS)
def test_deduplication_and_determinism(backend):
    snaps = []
    on = kernel_fuse(backend, 'generated7', 'all', snapshots=snaps)
    off = kernel_fuse(backend, 'generated7', 'all', dedup=False)
    # (c) fewer points, a subset of the kept pixels, and nobody is emitted whose byte was set when its view ran
    assert 0 < on['emit'].sum() < off['emit'].sum()
    assert np.all(off['emit'][on['emit'] > 0] == 1)
    assert np.array_equal(off['emit'] > 0, kernel_consistency(backend, 'generated7', 'all')['count'] >= MIN_VIEWS)
    for i in range(N):
        assert not np.any((on['emit'][i] > 0) & (snaps[i] > 0))
        assert np.array_equal(on['emit'][i] > 0, (off['emit'][i] > 0) & (snaps[i] == 0))
    # (d) two runs: the same bytes
    again = kernel_fuse(backend, 'generated7', 'all')
    for k in ('emit', 'xyz', 'colour', 'normal', 'taken'):
        assert on[k].tobytes() == again[k].tobytes(), k
    poses, Ks = cameras()
    second = engine_for(backend).depth_consistency(views('generated7')[0], poses, Ks, table('all'), TAU_PX, TAU_D, outputs=ALL_OUT)
    for k, v in kernel_consistency(backend, 'generated7', 'all').items():
        assert second[k].cpu().numpy().tobytes() == v.tobytes(), k


BLOCK_VIEW, BLOCK_Y, BLOCK_X = 1, 20, 24          # a 6 x 6 block of view 1 of the hand-made scene, on the sphere in its middle


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_corrupted_block_is_rejected_and_nothing_else_changes(backend):
    poses, Ks = cameras()
    clean_depth = views('hand')[0]
    block = np.zeros((H, W), bool)
    block[BLOCK_Y:BLOCK_Y + 6, BLOCK_X:BLOCK_X + 6] = True
    assert np.all(clean_depth[BLOCK_VIEW][block] > 0)
    depth = clean_depth.copy()
    depth[BLOCK_VIEW][block] *= 1.2
    ref_clean = reference('hand', 'all')
    ref = geo.consistency_numpy(depth, poses, Ks, table('all'), TAU_PX, TAU_D)
    assert np.all(ref_clean['count'][BLOCK_VIEW][block] >= MIN_VIEWS)               # the block was kept before ...
    assert np.all(ref['count'][BLOCK_VIEW][block] < MIN_VIEWS)                      # ... and the float64 reference rejects all of it
    eng = engine_for(backend)
    got = {k: v.cpu().numpy() for k, v in eng.depth_consistency(depth, poses, Ks, table('all'), TAU_PX, TAU_D, outputs=ALL_OUT).items()}
    base = kernel_consistency(backend, 'hand', 'all')
    fused = kernel_fuse(backend, 'hand', 'all', cons=got, dedup=False, depth=depth)
    fused_base = kernel_fuse(backend, 'hand', 'all', dedup=False)
    assert not np.any(fused['emit'][BLOCK_VIEW][block])
    # a pair (view i, slot s) samples the block when its source is the corrupted view and its texel lies inside (the texel depends on the
    # pixel's own depth alone: the same in both runs); the corrupted view's own block pixels are the other pairs that may change
    block_texels = np.flatnonzero(block.reshape(-1))
    touched = np.zeros((N, 4, H, W), bool)
    for i in range(N):
        for s in range(4):
            if table('all')[i, s] == BLOCK_VIEW:
                touched[i, s] = np.isin(base['src_texel'][i, s], block_texels)
    touched[BLOCK_VIEW] |= block
    assert touched[[i for i in range(N) if i != BLOCK_VIEW]].any()
    assert np.array_equal(got['src_texel'][~touched], base['src_texel'][~touched])
    for k in ('consistent_bits', 'occluded_bits'):
        for s in range(4):
            assert np.array_equal(((got[k] >> s) & 1)[~touched[:, s]], ((base[k] >> s) & 1)[~touched[:, s]]), (k, s)
    same = ~touched.any(1)
    assert same[BLOCK_VIEW].sum() == H * W - 36
    for k in ('count', 'fused_depth'):
        assert np.array_equal(got[k][same], base[k][same]), k
    for k in ('emit', 'xyz', 'colour'):
        assert np.array_equal(fused[k][same], fused_base[k][same]), k


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_view_without_depth_contributes_nothing_and_breaks_nothing(backend):
    poses, Ks = cameras()
    depth = views('generated3')[0].copy()
    depth[2] = 0
    eng = engine_for(backend)
    got = {k: v.cpu().numpy() for k, v in eng.depth_consistency(depth, poses, Ks, table('all'), TAU_PX, TAU_D, outputs=ALL_OUT).items()}
    ref = geo.consistency_numpy(depth, poses, Ks, table('all'), TAU_PX, TAU_D, details=True)
    compare_consistency(got, ref, 'empty view [%s]' % backend)
    assert np.all(got['count'][2] == 0) and np.all(got['fused_depth'][2] == 0) and np.all(got['src_texel'][2] == -1)
    for i in range(N):
        for s in range(4):
            if table('all')[i, s] == 2:                    # nobody sees anything in the empty view
                assert np.all(got['src_texel'][i, s] == -1) and not np.any((got['consistent_bits'][i] >> s) & 1)
    fused = kernel_fuse(backend, 'generated3', 'all', cons=got, depth=depth)
    assert fused['emit'][2].sum() == 0 and fused['taken'][2].sum() == 0 and fused['emit'].sum() > 300
    for k in ('xyz', 'colour', 'normal'):
        assert np.all(np.isfinite(fused[k])), k


# ---- 4. the public surface -----------------------------------------------------------------------------------------------------------------
def test_ply_round_trip(tmp_path):
    rng = np.random.RandomState(0)
    pts, nrm, col = rng.randn(37, 3).astype(np.float32), rng.randn(37, 3).astype(np.float32), rng.rand(37, 3).astype(np.float32)
    path = str(tmp_path / 'cloud.ply')
    geo.write_ply(path, torch.from_numpy(pts), col, nrm)
    head = open(path, 'rb').read(400).decode('ascii', 'replace')
    assert head.startswith('ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\n') and 'property uchar blue\nend_header\n' in head
    assert os.path.getsize(path) == head.index('end_header\n') + len('end_header\n') + 37 * 27
    back = geo.read_ply(path)
    assert back['points'].tobytes() == pts.tobytes() and back['normals'].tobytes() == nrm.tobytes()
    assert np.array_equal(back['colors'], np.clip(col * 255, 0, 255).astype(np.uint8))
    geo.write_ply(path, pts[:0])
    assert geo.read_ply(path)['points'].shape == (0, 3)
    with open(path, 'wb') as f:
        f.write(b'ply\nformat ascii 1.0\nend_header\n')
    with pytest.raises(ValueError):
        geo.read_ply(path)


@pytest.mark.parametrize('backend', BACKENDS)
def test_filter_depth_and_fuse_points_choose_the_nearest_cameras(backend):
    poses, Ks = cameras()
    depth, rgb = views('hand')
    eng = engine_for(backend)
    nn = geo.nearest_sources(poses, 3)
    assert nn.shape == (N, 3) and all(i not in nn[i] and len(set(nn[i])) == 3 for i in range(N))
    assert geo.nearest_sources(poses, 8).shape == (N, 8) and np.all(geo.nearest_sources(poses, 8)[:, 4:] == -1)
    got = geo.filter_depth(depth, poses, Ks, src=3, engine=eng)
    want = eng.depth_consistency(depth, poses, Ks, nn)
    kept = want['count'] >= MIN_VIEWS
    assert torch.equal(got['depth'], torch.where(kept, want['fused_depth'], torch.zeros_like(want['fused_depth'])))
    assert torch.equal(got['count'], want['count']) and torch.equal(got['consistent_bits'], want['consistent_bits'])
    assert torch.equal(got['occluded_bits'], want['occluded_bits']) and 0 < int(kept.sum()) < int((torch.from_numpy(depth) > 0).sum())
    cloud = geo.fuse_points(depth, rgb, poses, Ks, src=3, engine=eng)
    m = cloud['points'].shape[0]
    assert m > 300 and all(cloud[k].shape == (m, 3) for k in ('points', 'colors', 'normals')) and cloud['view'].shape == (m,)
    order = (cloud['view'] * (H * W) + cloud['pixel']).cpu().numpy()
    assert np.all(np.diff(order) > 0)                      # (view, row, column)
    view, pixel = cloud['view'].cpu().numpy(), cloud['pixel'].cpu().numpy()
    assert np.all(got['depth'].cpu().numpy()[view, pixel // W, pixel % W] > 0)      # every point comes from a kept pixel
    # the path without a device: the float32 reference, the same cloud up to the reference's own error
    host = geo.fuse_points(depth, rgb, poses, Ks, nn_ids=nn, engine=None) if not torch.cuda.is_available() else None
    if host is not None:
        assert torch.equal(host['view'], cloud['view'].cpu()) and torch.equal(host['pixel'], cloud['pixel'].cpu())
        assert float((host['points'] - cloud['points'].cpu()).abs().max()) <= TOL_XYZ


def test_render_depth_maps_on_the_emulator():
    from neuray_amd.network import render_ops as ro
    from neuray_amd.network import encoders, renderer as R
    ro._ENGINES.clear()
    ro._TEST_LIB = emu_lib()
    encoders.set_x3_conv(False)                            # (PyTorch's CPU convolutions in the encoders, as tests/test_scene_renderers.py)
    try:
        torch.manual_seed(0)
        gen = R.NeuralRayGenRenderer({'use_hierarchical_sampling': True, 'depth_sample_num': 8, 'fine_depth_sample_num': 8,
                                      'agg_net_cfg': {'sample_num': 8}, 'fine_agg_net_cfg': {'sample_num': 8}, 'ray_batch_num': 512,
                                      'init_net_type': 'depth', 'depth_loss_coords_num': 8}).eval()
        gen._engine_test_lib = emu_lib()
        db = proc.ProceduralDatabase('procedural/3/white_16', n_views=5, h=12, w=16, ss=1)
        ids = db.get_img_ids()
        maps = geo.render_depth_maps(gen, db, ids[1:2], work_num=2, pad_interval=32)      # (the init net's ResNet needs 32 pixels)
        assert gen.cfg['render_depth'] is False            # (put back)
        assert maps['depth'].shape == (1, 12, 16) and maps['depth'].dtype == np.float32 and np.all(np.isfinite(maps['depth']))
        assert maps['imgs'].shape == (1, 3, 12, 16) and maps['poses'].shape == (1, 3, 4) and maps['Ks'].shape == (1, 3, 3)
        near, far = db.get_depth_range(ids[0])
        assert np.all(maps['depth'] >= 0) and np.all(maps['depth'] <= far * 1.01) and maps['depth'].std() > 0      # (sum of hit_prob x depth, hit_prob sums to <= 1)
        assert len(maps['working_ids']) == 1 and len(maps['working_ids'][0]) == 2 and ids[1] not in maps['working_ids'][0]
        own = geo.database_depth_maps(db, ids[1:2])
        assert np.array_equal(own['depth'], np.stack([db.get_depth(i) for i in ids[1:2]])) and np.array_equal(own['imgs'], maps['imgs'])
    finally:
        encoders.set_x3_conv(True)
        ro._TEST_LIB = None
        ro._ENGINES.clear()


def test_command_line_exports_a_procedural_database(tmp_path, capsys):
    import json
    from neuray_amd import export_points
    out, js = str(tmp_path / 'cloud.ply'), str(tmp_path / 'cloud.json')
    res = export_points.main(['--database', 'procedural/5/white_64', '--depth', 'database', '--out', out, '--src', '6', '--json', js])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.load(open(js)) and line['points'] == res['points'] and line['views'] == 48 and (line['h'], line['w']) == (64, 64)
    cloud = geo.read_ply(out)
    assert cloud['points'].shape == (res['points'], 3) and 5000 < res['points'] < res['pixels_with_depth']
    # exact depth maps: the cloud lies on the surface (bound (a) of the property test at the far end of the depth range)
    assert res['surface_distance']['max'] <= 0.01 * 6.0 * 1.2 + 1e-4 and res['surface_distance']['median'] < 0.01
    dist = geo.surface_distance(proc.make_scene(5, 'white'), cloud['points'])
    assert abs(float(dist.max()) - res['surface_distance']['max']) < 1e-6
    length = np.linalg.norm(cloud['normals'], axis=1)
    assert np.all((length == 0) | (np.abs(length - 1) < 1e-5))
    with pytest.raises(SystemExit):
        export_points.main(['--depth', 'database', '--out', out])
    with pytest.raises(SystemExit):
        export_points.main(['--database', 'procedural/5/white_64', '--src', '17', '--out', out])


def test_surface_distance_is_the_closed_form():
    sc = proc.pack_scene([{'kind': 'sphere', 'p': (0.5, 0.0, 0.0), 'e': 0.25, 'b': (0.5, 0.5, 0.5)},
                          {'kind': 'box', 'p': (-1.0, 0.0, 0.0), 'e': (0.5, 0.25, 0.125), 'b': (0.5, 0.5, 0.5)}])
    pts = np.array([[0.5, 0.0, 1.0], [0.5, 0.0, 0.0], [-1.0, 0.0, 0.625], [-1.0, 0.0, 0.0], [-2.0, 1.0, 0.0], [0.75, 0.0, 0.0]])
    want = np.array([0.75, 0.25, 0.5, 0.125, np.hypot(0.5, 0.75), 0.0])
    assert np.allclose(geo.surface_distance(sc, pts), want, atol=1e-7)


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_the_entry_points_check_their_arguments(backend):
    import ctypes as C
    from neuray_amd import _lib
    eng = engine_for(backend)
    poses, Ks = cameras()
    depth, rgb = views('hand')
    nn = table('all')
    with pytest.raises(RuntimeError, match='n_src=17'):
        eng.depth_consistency(depth, poses, Ks, np.full((N, 17), -1, np.int32))
    with pytest.raises(RuntimeError, match='n_src=0'):
        eng.depth_consistency(depth, poses, Ks, np.zeros((N, 0), np.int32))
    with pytest.raises(RuntimeError, match='bad size'):
        eng.depth_consistency(depth[:, :0], poses, Ks, nn)
    for kw in ({'tau_px': 0.0}, {'tau_d': -1.0}, {'tau_px': float('nan')}):
        with pytest.raises(RuntimeError, match='thresholds'):
            eng.depth_consistency(depth, poses, Ks, nn, **kw)
    for name in ('neuray_depth_consistency', 'neuray_fuse_view'):
        with pytest.raises(RuntimeError, match='null args'):
            eng._check(getattr(eng.lib, name)(None, eng._stream()))
    with pytest.raises(RuntimeError, match='missing'):
        eng._check(eng.lib.neuray_depth_consistency(C.byref(_lib.NeurayDepthConsistencyArgs(n=N, h=H, w=W, n_src=4, tau_px=1.0, tau_d=0.01)), eng._stream()))
    cons = {k: torch.from_numpy(np.ascontiguousarray(v)).to(eng.device) for k, v in kernel_consistency(backend, 'hand', 'all').items()}
    taken = torch.zeros(N, H, W, dtype=torch.uint8, device=eng.device)
    for view in (-1, N):
        with pytest.raises(RuntimeError, match='view='):
            eng.fuse_view(view, depth, rgb, poses, Ks, nn, cons, taken)
    with pytest.raises(RuntimeError, match='min_views=0'):
        eng.fuse_view(0, depth, rgb, poses, Ks, nn, cons, taken, min_views=0)
    with pytest.raises(RuntimeError, match='thresholds'):
        eng.fuse_view(0, depth, rgb, poses, Ks, nn, cons, taken, tau_n=0.0)
    with pytest.raises(RuntimeError, match='n_src=17'):
        eng.fuse_view(0, depth, rgb, poses, Ks, np.full((N, 17), -1, np.int32), cons, taken)
    with pytest.raises(RuntimeError, match='missing'):
        eng._check(eng.lib.neuray_fuse_view(C.byref(_lib.NeurayFuseViewArgs(n=N, h=H, w=W, n_src=4, view=0, min_views=2, tau_n=0.05)), eng._stream()))
    assert int(taken.sum()) == 0                           # nothing ran
    with pytest.raises(ValueError):
        geo.consistency_numpy(depth, poses, Ks, np.full((N, 17), -1, np.int32))
    with pytest.raises(ValueError):
        geo.filter_depth(depth, poses, Ks, min_views=0, engine=eng)
    # ... and 16 slots are accepted
    wide = np.full((N, 16), -1, np.int32)
    wide[:, 15] = nn[:, 0]
    out = eng.depth_consistency(depth, poses, Ks, wide)
    assert np.array_equal(out['consistent_bits'].cpu().numpy() >> 15, kernel_consistency(backend, 'hand', 'all')['consistent_bits'] & 1)
