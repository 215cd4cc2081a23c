"""Procedural 3-D scenes (neuray_amd/procedural.py, csrc/nr_kernels_proc.h): the ray-cast kernel against the float64
reference renderer, the zero-component branch of the slab method, multi-view consistency of pose / K / z-depth, the database and the
training stream built on it, and the first test in which there is something to learn.

Tolerances.  They come from the reference alone: render_numpy(float32) against render_numpy(float64) on the four scenes and two sub-sampling
factors below (3 views of 40 x 56), near-degenerate pixels left out (test_reference_float32_agrees_with_float64 measures and asserts it on the
CPU).  Worst values measured: depth 2.04e-5 relative (the 32-primitive scene; 1.6e-5 .. 1.9e-5 on the others: the cancellation in a sphere's
discriminant B^2 - A C near its silhouette), rgb 2.60e-4 absolute (the 32-primitive scene, ss 1; 3e-5 .. 1.5e-4 on the others).  The gates are
4 x these - the device library's division, sinf and powf may round differently from numpy's: TOL_DEPTH = 8.16e-5 relative, TOL_RGB = 1.04e-3
absolute.  At most 0.5 % of a case's pixels may be near-degenerate (measured: 0 .. 0.34 %; see full_prims for what decides it)."""
import functools

import numpy as np
import pytest
import torch

from emu_util import emu_lib
from oracle import neuray_oracle as orc
from neuray_amd import database, pipeline, procedural as proc, synthetic
from neuray_amd.engine import RenderEngine, host_inverse

BACKENDS = ['emu', pytest.param('hip', marks=pytest.mark.gpu)]
H, W = 40, 56                                   # neither a multiple of the 64 x 4 tile: partial tiles in both directions, two tile rows ... ten
REL = 1e-5                                      # the near-degenerate gates
MAX_LEFT_OUT = 0.005
REF_DEPTH_ERR, REF_RGB_ERR = 2.04e-5, 2.60e-4   # float32 reference against float64 reference, worst over the cases (see the docstring)
TOL_DEPTH, TOL_RGB = 4 * REF_DEPTH_ERR, 4 * REF_RGB_ERR


def engine_for(backend):
    dev = 'cpu' if backend == 'emu' else 'cuda:0'
    return RenderEngine(dev, _test_lib=emu_lib() if backend == 'emu' else None), dev


def cameras():
    poses = np.stack([synthetic.look_at_pose(synthetic.sphere_pos(proc.CAMERA_RADIUS, a, e)) for a, e in ((20.0, 25.0), (140.0, 40.0), (260.0, 15.0))])
    return poses.astype(np.float32), np.repeat(proc.intrinsics(H, W)[None], 3, 0)


def wave(k, phi, a):
    return (np.asarray(k, np.float64), phi, np.asarray(a, np.float64))


def hand_prims():
    """five primitives of both kinds that hide parts of one another from every camera of cameras()"""
    tex = [wave((1.1, -0.7, 0.4), 0.3, (0.12, -0.08, 0.05)), wave((-0.5, 1.3, 0.9), 1.7, (-0.06, 0.1, 0.09)),
           wave((0.8, 0.6, -1.4), 2.9, (0.07, 0.07, -0.11)), wave((-1.5, -0.2, 0.3), 4.1, (0.04, -0.12, 0.06))]
    return [
        {'kind': 'box', 'p': (0.0, 0.0, -0.9), 'e': (1.1, 1.1, 0.04), 'b': (0.55, 0.5, 0.45), 's': 0.1, 'm': 12.0, 'waves': tex},
        {'kind': 'sphere', 'p': (0.1, -0.1, -0.2), 'e': 0.55, 'b': (0.8, 0.3, 0.3), 's': 0.35, 'm': 30.0, 'waves': tex[::-1]},
        {'kind': 'box', 'p': (-0.55, 0.5, -0.35), 'e': (0.3, 0.25, 0.5), 'b': (0.3, 0.7, 0.4), 's': 0.2, 'm': 18.0, 'waves': tex[1:] + tex[:1]},
        {'kind': 'sphere', 'p': (0.7, 0.55, -0.5), 'e': 0.33, 'b': (0.35, 0.4, 0.85), 's': 0.3, 'm': 9.0, 'waves': tex[2:] + tex[:2]},
        {'kind': 'box', 'p': (0.45, -0.75, 0.1), 'e': (0.2, 0.35, 0.17), 'b': (0.75, 0.7, 0.3), 's': 0.15, 'm': 25.0, 'waves': tex},
    ]


def full_prims():
    """32 primitives: the plate, 3 spheres and 28 small boxes scattered above it.  Few spheres on purpose: the gate |discriminant| < 1e-5 B^2
    takes a band around every sphere's silhouette whose AREA does not depend on the sphere's size - 1e-5 . 2 pi f^2 pixels per ray, 1.7e-4 of
    this image - so that with 5 rays per pixel (ss 2) four spheres in view already use up the 0.5 % that may be left out."""
    rng = np.random.RandomState(0)
    prims = [hand_prims()[0]]
    for i in range(31):
        kind = 'sphere' if i < 3 else 'box'
        p = rng.uniform(-0.9, 0.9, size=3) * np.array([1, 1, 0.5]) + np.array([0, 0, -0.2])
        e = rng.uniform(0.15, 0.3) if kind == 'sphere' else rng.uniform(0.06, 0.22, size=3)
        prims.append(proc.random_prim(rng, kind, p=p, e=e))
    return prims


@functools.lru_cache(None)
def scene(name):
    if name == 'hand':
        return proc.pack_scene(hand_prims(), light=(0.3, -0.2, 1.0), ambient=0.35, background='white')
    if name == 'generated':
        return proc.make_scene(7, 'black')
    if name == 'single':
        return proc.pack_scene(hand_prims()[1:2], light=(0.3, -0.2, 1.0), ambient=0.3, background='black')
    if name == 'full':
        return proc.pack_scene(full_prims(), light=(0.2, 0.3, 1.0), ambient=0.3, background='white')
    if name == 'albedo':                                   # s = 0, ambient 1: the colour is the object-space albedo, the same from every view
        return proc.pack_scene([{**p, 's': 0.0} for p in hand_prims()], light=(0.3, -0.2, 1.0), ambient=1.0, background='black')
    raise KeyError(name)


CASES = [(s, ss) for s in ('hand', 'generated', 'single', 'full') for ss in (1, 2)]


@functools.lru_cache(None)
def reference(name, ss, dtype='float64'):
    """computed once, shared, never modified (the arrays are read-only)"""
    poses, Ks = cameras()
    out = proc.render_numpy(scene(name), poses, Ks, H, W, ss, dtype=np.dtype(dtype), degenerate_rel=REL if dtype == 'float64' else None)
    for v in out.values():
        v.setflags(write=False)
    return out


def compare(got, want, what):
    """the gates of test 1 on one case -> (worst relative depth error, worst rgb error); got: dict of numpy arrays"""
    keep = ~want['degenerate']
    left_out = 1.0 - keep.mean()
    assert left_out <= MAX_LEFT_OUT, (what, left_out)
    for k in ('rgb', 'depth'):
        assert np.all(np.isfinite(got[k])), (what, k)
    assert np.array_equal(got['mask'][keep], want['mask'][keep]), what
    assert np.array_equal(got['prim'][keep], want['prim'][keep]), what
    hit = keep & (want['mask'] > 0)
    assert np.all(got['depth'][keep & (want['mask'] == 0)] == 0)
    d_err = float(np.max(np.abs(got['depth'][hit] - want['depth'][hit]) / want['depth'][hit])) if hit.any() else 0.0
    c_err = float(np.max(np.abs(got['rgb'].astype(np.float64) - want['rgb'])[np.broadcast_to(keep[:, None], got['rgb'].shape)]))
    print('%s: left out %.3f %%, depth %.2e relative, rgb %.2e' % (what, 100 * left_out, d_err, c_err))
    return d_err, c_err


def kernel_render(backend, sc, poses, Ks, h, w, ss):
    eng, dev = engine_for(backend)
    out = eng.procedural_render(sc, poses, Ks, h, w, ss)
    assert out['rgb'].dtype == torch.float32 and out['depth'].dtype == torch.float32 and out['mask'].dtype == torch.uint8 and out['prim'].dtype == torch.int8
    assert out['rgb'].shape == (len(poses), 3, h, w) and all(out[k].shape == (len(poses), h, w) for k in ('depth', 'mask', 'prim'))
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- the reference against itself: where the tolerances come from -----------------------------------------------------------------
def test_reference_float32_agrees_with_float64():
    worst_d = worst_c = 0.0
    for name, ss in CASES:
        d, c = compare(reference(name, ss, 'float32'), reference(name, ss), 'float32 reference %s ss %d' % (name, ss))
        worst_d, worst_c = max(worst_d, d), max(worst_c, c)
        want = reference(name, ss)
        assert 0.05 < want['mask'].mean() < 0.95                      # the cameras see the scene and its silhouette
    print('worst: depth %.3e relative, rgb %.3e' % (worst_d, worst_c))
    # the gates are 4 x what was measured when they were written down; the measurement still holds
    assert worst_d <= REF_DEPTH_ERR * 1.0001 and worst_c <= REF_RGB_ERR * 1.0001
    # mutual occlusion in the hand-made scene: every primitive is seen, and none of the four upper ones is seen whole from every camera
    prim = reference('hand', 1)['prim']
    assert set(np.unique(prim)) == {-1, 0, 1, 2, 3, 4}
    poses, Ks = cameras()
    for i in range(1, 5):
        alone = proc.render_numpy(proc.pack_scene(hand_prims()[i:i + 1]), poses, Ks, H, W)['mask']
        assert ((alone > 0) & (prim != i)).any(), i


def test_default_generator_keeps_its_promises():
    for seed in range(12):
        sc = proc.make_scene(seed)
        assert sc.dtype == np.float32 and sc.tobytes() == proc.make_scene(seed).tobytes()
        n = proc.scene_prims(sc)
        assert 6 <= n <= 12 and sc[0] == n and sc.size == proc.HEADER + n * proc.PRIM
        P = sc[proc.HEADER:].reshape(n, proc.PRIM)
        assert {0.0, 1.0} == set(P[:, 0])
        # the farthest point of a sphere: |p| + r; of a box: its farthest corner
        far = np.where(P[:, 0] == 0, np.linalg.norm(P[:, 1:4], axis=1) + P[:, 4], np.linalg.norm(np.abs(P[:, 1:4]) + P[:, 4:7], axis=1))
        assert np.all(far <= proc.SCENE_RADIUS)
        assert abs(np.linalg.norm(sc[1:4]) - 1) < 1e-6
    assert proc.make_scene(1).tobytes() != proc.make_scene(2).tobytes()
    with pytest.raises(NotImplementedError):
        proc.make_scene(0, 'green')


# ---- 1. parity with the float64 reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name,ss', CASES)
def test_kernel_matches_the_float64_reference(name, ss, backend):
    poses, Ks = cameras()
    got = kernel_render(backend, scene(name), poses, Ks, H, W, ss)
    d_err, c_err = compare(got, reference(name, ss), 'kernel [%s] %s ss %d' % (backend, name, ss))
    assert d_err <= TOL_DEPTH
    assert c_err <= TOL_RGB


@pytest.mark.parametrize('backend', BACKENDS)
def test_optional_outputs_are_skipped(backend):
    poses, Ks = cameras()
    eng, dev = engine_for(backend)
    full = eng.procedural_render(scene('hand'), poses, Ks, H, W, 2)
    only = eng.procedural_render(scene('hand'), poses, Ks, H, W, 2, outputs=())
    some = eng.procedural_render(scene('hand'), poses, Ks, H, W, 2, outputs=('depth',))
    assert set(only) == {'rgb'} and set(some) == {'rgb', 'depth'}
    assert torch.equal(only['rgb'], full['rgb']) and torch.equal(some['rgb'], full['rgb']) and torch.equal(some['depth'], full['depth'])


# ---- 2. the zero-component branch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('ss', [1, 2])
def test_rays_with_a_zero_component_take_the_explicit_branch(ss, backend):
    """a camera on the -y axis looks along +y at a box; f = 64 and cx = 28, cy = 20 are exact in fp32 and so is K^-1: the rays of column 28
    have d_x == 0, those of row 20 d_z == 0, exactly.  The box is off centre: column 28 is inside its x slab, row 20 outside its z slab
    beside it, and the plate below is crossed by rays with d_x == 0 as well."""
    pose = synthetic.look_at_pose((0.0, -proc.CAMERA_RADIUS, 0.0))[None].astype(np.float32)
    K = np.array([[[64.0, 0, 28.0], [0, 64.0, 20.0], [0, 0, 1]]], np.float32)
    Ki = host_inverse(torch.from_numpy(K)).numpy()
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    _, d = orc.coords2rays(np.stack([xs, ys], -1).reshape(1, -1, 2).astype(np.float32), pose, Ki)
    d = d.reshape(H, W, 3)
    assert np.all(d[:, 28, 0] == 0) and np.all(d[20, :, 2] == 0) and np.all(d[:, 27, 0] != 0)
    prims = [{**hand_prims()[2], 'p': (0.1, 0.0, 0.45), 'e': (0.5, 0.4, 0.3)}, {**hand_prims()[0], 'p': (0.0, 0.0, -0.5)}]
    sc = proc.pack_scene(prims, light=(0.2, -0.6, 1.0), ambient=0.4, background='white')
    want = proc.render_numpy(sc, pose, K, H, W, ss, degenerate_rel=REL)
    assert want['prim'][0, 10, 28] == 0 and want['prim'][0, 20, 28] == -1 and want['prim'][0, 30, 28] >= 0      # d_x == 0: hit, miss, hit
    assert not want['degenerate'][0, :, 28].any() or ss == 2
    got = kernel_render(backend, sc, pose, K, H, W, ss)
    for k in ('rgb', 'depth'):
        assert np.all(np.isfinite(got[k])), k                       # nothing is excluded by NaN: there is none
    d_err, c_err = compare(got, want, 'zero component [%s] ss %d' % (backend, ss))
    assert d_err <= TOL_DEPTH and c_err <= TOL_RGB


# ---- 3. multi-view consistency -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_views_agree_on_the_surface_they_share(backend):
    """pose, K and z-depth mean what the render path means by them: X = c_A + d_A depth_A (oracle.coords2rays) lies on the surface, so the
    ray from view B's centre through X hits nothing behind X, and where it hits at X it finds the colour view A shows (albedo only: s = 0,
    ambient 1).  Colour bound: TOL_RGB plus the albedo's Lipschitz constant (2 pi sum_w |k_w| max|a_w|, the largest over the primitives)
    times the distance between X and B's hit point - the two are different points of the surface by what the fp32 depth is off."""
    sc = scene('albedo')
    poses, Ks = cameras()
    got = kernel_render(backend, sc, poses, Ks, H, W, 1)
    want = proc.render_numpy(sc, poses, Ks, H, W, 1, degenerate_rel=REL)
    P = sc[proc.HEADER:].reshape(-1, proc.PRIM)[:, 12:40].reshape(-1, 4, 7).astype(np.float64)
    lipschitz = float(np.max(2 * np.pi * np.sum(np.linalg.norm(P[:, :, :3], axis=2) * np.abs(P[:, :, 4:]).max(2), axis=1)))
    Ki = np.concatenate([host_inverse(torch.from_numpy(Ks[i:i + 1])).numpy() for i in range(3)])
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    coords = np.stack([xs, ys], -1).reshape(1, -1, 2).astype(np.float32)
    shared = 0
    for a, b in ((0, 1), (1, 2), (2, 0)):
        c_a, d_a = orc.coords2rays(coords, poses[a:a + 1], Ki[a:a + 1])
        c_b, _ = orc.coords2rays(coords[:, :1], poses[b:b + 1], Ki[b:b + 1])
        sel = ((got['mask'][a] > 0) & ~want['degenerate'][a]).reshape(-1)
        depth = got['depth'][a].reshape(-1)[sel].astype(np.float64)
        X = c_a[0, sel].astype(np.float64) + d_a[0, sel].astype(np.float64) * depth[:, None]
        o = np.broadcast_to(c_b[0, 0].astype(np.float64), X.shape)
        t, prim = proc.cast_numpy(sc, o, X - o)
        assert np.all(t <= 1 + TOL_DEPTH), float(t.max())          # never behind X (t = 1) by more than the depth tolerance
        same = np.abs(t - 1) <= TOL_DEPTH
        assert np.array_equal(prim[same], got['prim'][a].reshape(-1)[sel][same])
        hit = o[same] + t[same, None] * (X - o)[same]
        colour_b = proc.albedo_numpy(sc, hit, prim[same])
        colour_a = got['rgb'][a].reshape(3, -1).T[sel][same].astype(np.float64)
        bound = TOL_RGB + lipschitz * np.linalg.norm(hit - X[same], axis=1)
        assert np.all(np.abs(colour_a - colour_b).max(1) <= bound), float((np.abs(colour_a - colour_b).max(1) - bound).max())
        shared += int(same.sum())
        assert (~same).any()                                        # ... and some of A's surface is hidden from B: occlusion
    assert shared > 500


# ---- 4. database --------------------------------------------------------------------------------------------------------------------
def test_database_surface():
    db = database.parse_database_name('procedural/3/white_32')
    assert isinstance(db, proc.ProceduralDatabase) and database.name2database['procedural'] is proc.ProceduralDatabase
    assert (db.seed, db.background, db.h, db.w) == (3, 'white', 32, 32) and len(db.get_img_ids()) == 48
    train, val = database.get_database_split(db, 'val_all')
    assert val == db.get_img_ids()[::8] and len(val) == 6 and len(train) == 42 and not set(train) & set(val)
    assert database.get_database_split(db, 'test')[1] == val
    with pytest.raises(NotImplementedError):
        proc.ProceduralDatabase('procedural/3/green_32')
    small = proc.ProceduralDatabase('procedural/3/white_32', n_views=5, h=24, w=40)
    ids = small.get_img_ids()
    img, mask, depth = small.get_image(ids[1]), small.get_mask(ids[1]), small.get_depth(ids[1])
    assert img.dtype == np.uint8 and img.shape == (24, 40, 3) and mask.dtype == np.bool_ and mask.shape == (24, 40)
    assert depth.dtype == np.float32 and depth.shape == (24, 40)
    assert small.get_K(ids[0]).shape == (3, 3) and small.get_pose(ids[0]).shape == (3, 4) and small.get_pose(ids[0]).dtype == np.float32
    x0, y0, bw, bh = small.get_bbox(ids[1])
    assert mask[y0:y0 + bh, x0:x0 + bw].sum() == mask.sum() and mask[y0].any() and mask[:, x0].any()
    # (ss 2: a pixel whose centre ray misses may still carry colour from a sub-ray that hits; away from the silhouettes it is background)
    assert np.mean(np.all(img[~mask] == 255, -1)) > 0.8 and 0.1 < mask.mean() < 0.95
    # the same seed twice: the same bytes
    again = proc.ProceduralDatabase('procedural/3/white_32', n_views=5, h=24, w=40)
    assert again.scene.tobytes() == small.scene.tobytes()
    for i in ids:
        assert again.get_image(i).tobytes() == small.get_image(i).tobytes() and again.get_depth(i).tobytes() == small.get_depth(i).tobytes()
        near, far = small.get_depth_range(i)
        d = small.get_depth(i)[small.get_mask(i)]
        assert (near, far) == (2.0, 6.0) and d.size and near < d.min() and d.max() < far
        assert np.all(small.get_depth(i)[~small.get_mask(i)] == 0)
    assert proc.ProceduralDatabase('procedural/4/white_32', n_views=5, h=24, w=40).get_image(ids[1]).tobytes() != img.tobytes()
    # the host pipeline on it, unchanged
    info = pipeline.build_imgs_info(small, ids[:3])
    assert info['imgs'].shape == (3, 3, 24, 40) and info['imgs'].dtype == np.float32 and info['masks'].shape == (3, 1, 24, 40)
    assert info['depth'].shape == (3, 1, 24, 40) and info['poses'].shape == (3, 3, 4) and info['Ks'].shape == (3, 3, 3)
    assert np.array_equal(info['depth_range'], np.repeat([[2.0, 6.0]], 3, 0).astype(np.float32))
    dev = pipeline.DeviceViewCache(small, 'cpu').imgs_info(ids[:3])
    for k, shape, dt in (('imgs', (3, 3, 24, 40), torch.float32), ('masks', (3, 1, 24, 40), torch.float32), ('depth', (3, 1, 24, 40), torch.float32),
                         ('poses', (3, 3, 4), torch.float32), ('Ks', (3, 3, 3), torch.float32), ('depth_range', (3, 2), torch.float32)):
        assert tuple(dev[k].shape) == shape and dev[k].dtype == dt, k
        assert np.allclose(dev[k].numpy(), info[k]), k
    poses, Ks, shapes, ranges, ref_ids, render_ids = database.prepare_eval_render(small)
    assert render_ids == ids[::8] and poses.shape == (1, 3, 4) and tuple(shapes[0]) == (24, 40)


def test_every_view_of_the_default_database_stays_inside_the_depth_range():
    """the assertion behind depth_range = (2, 6): 48 cameras at radius 4.03, everything inside the ball of radius 1.9"""
    db = proc.ProceduralDatabase('procedural/0/white_16', ss=1)
    seen = set()
    for i in db.get_img_ids():
        d, m = db.get_depth(i), db.get_mask(i)
        assert m.any() and 2.0 < d[m].min() and d[m].max() < 6.0
        seen.add(db.get_pose(i).tobytes())
    assert len(seen) == 48


# ---- 5. the stream -------------------------------------------------------------------------------------------------------------------
GEN_CFG = {'init_net_type': 'cost_volume', 'use_hierarchical_sampling': True, 'use_depth_loss': True, 'dist_decoder_cfg': {'use_vis': False},
           'fine_dist_decoder_cfg': {'use_vis': False}, 'ray_batch_num': 2048, 'depth_loss_coords_num': 256}


@pytest.mark.gpu
def test_stream_batches_train_a_generalisation_step():
    from neuray_amd.loss import name2loss, total_loss
    from neuray_amd.network.renderer import NeuralRayGenRenderer
    dev = torch.device('cuda:0')
    h, w, rfn, extra, rays = 64, 96, 2, 2, 64
    stream = proc.ProceduralStream(dev, seed=5, h=h, w=w, rfn=rfn, extra_src=extra, rays=rays)
    first, batch = next(stream), next(stream)
    assert first['scene_name'] != batch['scene_name'] and not torch.equal(first['ref_imgs_info']['poses'], batch['ref_imgs_info']['poses'])
    assert not torch.equal(first['que_imgs_info']['imgs'], batch['que_imgs_info']['imgs'])          # a new scene and new cameras every batch
    # the dictionary of bench.gen_train_case: keys, shapes, dtypes, device
    f32, n_src = torch.float32, rfn + extra
    want = {'que_imgs_info': {'imgs': ((1, 3, h, w), f32), 'poses': ((1, 3, 4), f32), 'Ks': ((1, 3, 3), f32), 'Ks_inv': ((1, 3, 3), f32),
                              'depth_range': ((1, 2), f32), 'coords': ((1, rays, 2), f32)},
            'ref_imgs_info': {'imgs': ((rfn, 3, h, w), f32), 'masks': ((rfn, 1, h, w), f32), 'depth': ((rfn, 1, h, w), f32),
                              'true_depth': ((rfn, 1, h, w), f32), 'poses': ((rfn, 3, 4), f32), 'Ks': ((rfn, 3, 3), f32), 'depth_range': ((rfn, 2), f32),
                              'nn_ids': ((rfn, 3), torch.int64)},
            'src_imgs_info': {'imgs': ((n_src, 3, h, w), f32), 'poses': ((n_src, 3, 4), f32), 'Ks': ((n_src, 3, 3), f32), 'depth_range': ((n_src, 2), f32)}}
    for part, spec in want.items():
        for k, (shape, dt) in spec.items():
            t = batch[part][k]
            assert tuple(t.shape) == shape and t.dtype == dt and t.device == dev, (part, k)
    assert isinstance(batch['scene_name'], str)
    nn = batch['ref_imgs_info']['nn_ids'].cpu().numpy()
    assert all(v not in nn[v] and len(set(nn[v])) == 3 and nn[v].max() < n_src for v in range(rfn))
    # true_depth is the reference renderer's depth of the same scene and cameras
    sc, poses, _, _ = stream.host_batch(1)
    ref = proc.render_numpy(sc, poses[1:1 + rfn], np.repeat(stream.K[None], rfn, 0), h, w, 1, degenerate_rel=REL)
    got = batch['ref_imgs_info']['true_depth'][:, 0].cpu().numpy()
    keep = ~ref['degenerate'] & (ref['mask'] > 0)
    assert keep.mean() > 0.2 and np.array_equal(batch['ref_imgs_info']['masks'][:, 0].cpu().numpy()[~ref['degenerate']] > 0, ref['mask'][~ref['degenerate']] > 0)
    assert np.max(np.abs(got[keep] - ref['depth'][keep]) / ref['depth'][keep]) <= TOL_DEPTH
    # one training step with the render and the depth loss
    torch.manual_seed(0)
    np.random.seed(0)
    model = NeuralRayGenRenderer(GEN_CFG).train().to(dev)
    losses = [name2loss['render']({'use_nr_fine_loss': True}), name2loss['depth']({})]
    out = model({k: dict(v) if isinstance(v, dict) else v for k, v in batch.items()})
    total, log = total_loss(losses, out, batch, 0)
    assert {'loss_rgb_nr', 'loss_rgb_nr_fine', 'loss_depth', 'loss_depth_fine'} <= set(log) and bool(torch.isfinite(total))
    total.backward()
    grads = [p.grad for p in model.parameters() if p.requires_grad and p.grad is not None]
    assert len(grads) > 20 and all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)


# ---- 6. learning on ground truth ----------------------------------------------------------------------------------------------------
SMALL = {'use_hierarchical_sampling': True, 'depth_sample_num': 8, 'fine_depth_sample_num': 8,
         'agg_net_cfg': {'sample_num': 8}, 'fine_agg_net_cfg': {'sample_num': 8}, 'ray_batch_num': 16}      # tests/test_scene_renderers.py


@pytest.mark.gpu
def test_the_render_loss_goes_down_on_ground_truth():
    """On the random-image MemoryDatabase there is nothing to learn; here the views show one surface.  60 Adam steps of NeuralRayFtRenderer,
    fixed seeds: the mean render loss of steps 41-60 is below that of steps 1-20."""
    from neuray_amd.network.renderer import NeuralRayFtRenderer
    dev = 'cuda:0'
    db = proc.ProceduralDatabase('procedural/0/white_64', n_views=12, h=64, w=80)
    ids = db.get_img_ids()
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = {**SMALL, 'use_self_hit_prob': True, 'neighbor_view_num': 3, 'neighbor_pool_ratio': 1, 'train_ray_num': 64, 'foreground_ratio': 0.5,
           'ray_feats_res': [16, 20], 'use_validation': False}
    ft = NeuralRayFtRenderer(cfg, scene={'ref_imgs_info': pipeline.build_imgs_info(db, ids), 'database': db}).train().to(dev)
    opt = torch.optim.Adam(ft.parameters(), lr=2e-3)
    losses = []
    for _ in range(60):
        opt.zero_grad(set_to_none=True)
        out = ft({})
        gt = out['pixel_colors_gt']
        loss = ((out['pixel_colors_nr'] - gt) ** 2).mean() + ((out['pixel_colors_nr_fine'] - gt) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().numpy()
    assert np.all(np.isfinite(losses))
    head, tail = float(losses[:20].mean()), float(losses[40:].mean())
    print('render loss: steps 1-20 %.4f, steps 41-60 %.4f' % (head, tail))
    assert tail < head


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_the_entry_point_checks_its_arguments(backend):
    eng, dev = engine_for(backend)
    poses, Ks = cameras()
    sc = scene('hand')
    for ss in (0, 5, -1):
        with pytest.raises(RuntimeError, match='ss='):
            eng.procedural_render(sc, poses, Ks, H, W, ss)
    with pytest.raises(RuntimeError, match='n_prims=33'):
        eng.procedural_render(np.zeros(proc.HEADER + 33 * proc.PRIM, np.float32), poses, Ks, H, W)
    with pytest.raises(RuntimeError, match='bad size'):
        eng.procedural_render(sc, poses, Ks, 0, W)
    with pytest.raises(RuntimeError, match='bad size'):
        eng.procedural_render(sc, poses, Ks, H, 0)
    with pytest.raises(RuntimeError, match='null args'):
        eng._check(eng.lib.neuray_procedural_render(None, eng._stream()))
    with pytest.raises(ValueError):
        proc.pack_scene(hand_prims() * 7)
    # ... and 32 primitives, ss 4 are accepted
    out = eng.procedural_render(scene('full'), poses[:1], Ks[:1], 8, 70, 4)
    assert bool(torch.isfinite(out['rgb']).all())
