"""Plane-sweep stereo (neuray_amd/stereo.py, csrc/nr_kernels_stereo.h): the float32 reference against the float64 reference,
the kernel against the float64 reference, an analytic plane, accuracy against the true depth of a procedural scene, properties (determinism,
empty source tables, a constant image, tile skipping, splitting the views) and the public surface (estimate_depth, WithStereoDepth, the
command line, fuse_mesh on stereo depth, argument errors).

Cases: 5 cameras within 25 degrees of each other, 40 x 56 pixels (partial 16 x 16 tiles both ways), three procedural scenes, images from
render_numpy(float64); D = 24 planes, r = 2; source tables "all others" (S = 4) and a table padded with a -1 and a self entry; on scene 7 also
r = 1, r = 3, D = 3 and a different depth range for every view.

Left out of the comparison of WHERE there is an estimate (test 2 d): pixels where, on some plane, a source's window variance (or the
reference window's) lies within VAR_BAND of var_min, or a warp of the window lies within stereo.EDGE_BAND = 2e-4 of an image edge (1e-4 of
z = 0).  At most 0.5 % of a case's pixels with an estimate (measured: REF_LEFT_OUT below is the worst case).

Tolerances.  They come from the reference alone: plane_sweep_numpy in float32 against float64 on the ten cases
(test_reference_float32_agrees_with_float64 measures and asserts them on the CPU).  Worst values measured:
  aggregated cost over the volume, where both are valid and the same sources count   6.9e-4 .. 1.8e-3 (2.7e-4 at D = 3), REF_ERR per case
  refined depth, same plane, second difference above its floor, exceptions aside     5.7e-5 .. 4.4e-4 relative (1.1e-3 at r = 1), REF_ERR
  per-(pixel, plane, source) validity flags that differ                              at most 2.8e-6 of all flags (REF_FLAG_SHARE)
  pixels left out of (d)                                                             at most 0.35 % (REF_LEFT_OUT)
The gates of a case are 4 x its own two values; (a) and (b) hold on every pixel where both have an estimate.  (c) holds where the winner is the
reference's and the reference's second difference exceeds CURV_MIN, except - decided from the float64 reference alone - where a validity
flag of the winning plane or of one of its two neighbours lies in those bands (a flag that flips moves that plane's mean by a discrete step)
or the second difference lies within 4 x REF_COST_ERR of CURV_MIN (it is a sum of four costs and may fall on either side).  Those exceptions
are 0.7 .. 1.9 % of the candidates (4.4 % at r = 1; REF_ERR's third value, measured in test 1); the kernel test allows that share + 0.5 %.
The analytic case (sources shifted by 20 and 16 whole pixels on the face's plane; the second difference is 0.024 .. 0.34 inside the face, so
the parabola applies everywhere): the float64 reference's largest |offset| is REF_ANALYTIC_OFF, float32 differs from it per pixel by at most
REF_ANALYTIC_OFF_ERR.
Accuracy (test 4; 80 x 112, D = 64, r = 2, S = 4, scene 7; float64 reference, measured on the CPU): after max_cost = 0.5 coverage 93.05 % of the
foreground, median relative error 1.768 %; after the geometric filter as well (tau_d = 1 %, two agreeing sources) 41.10 % and 0.814 %.
fuse_mesh on stereo depth (recorded, not gated): see test_fuse_mesh_on_stereo_depth."""
import functools
import json

import numpy as np
import pytest
import torch

from emu_util import emu_lib
from test_procedural import hand_prims
from neuray_amd import database as ndb, geometry as geo, procedural as proc, stereo, synthetic
from neuray_amd.engine import RenderEngine

BACKENDS = ['emu', pytest.param('hip', marks=pytest.mark.gpu)]
H, W, N = 40, 56, 5
ANGLES = ((20.0, 30.0), (32.0, 36.0), (8.0, 24.0), (26.0, 18.0), (14.0, 40.0))       # (azimuth, elevation): within 25 degrees of each other
D, R = 24, 2
VAR_BAND = 4e-7            # 4 x the float32 reference's worst error of a variance below 1e-4 (8.2e-8), rounded up
MAX_LEFT_OUT = 0.005
# float32 reference against float64 reference, the worst of the ten cases (measured by test_reference_float32_agrees_with_float64)
REF_FLAG_SHARE, REF_LEFT_OUT = 2.8e-6, 0.0035
REF_ERR = {             # case -> (REF_COST_ERR, REF_DEPTH_ERR, the share of the refinement candidates that are exceptions), each rounded up
    ('generated7', 'all', 24, 2, 'same'): (0.00109, 0.000123, 0.00974),
    ('generated7', 'padded', 24, 2, 'same'): (0.00109, 0.000272, 0.0115),
    ('generated3', 'all', 24, 2, 'same'): (0.00138, 8.24e-05, 0.00973),
    ('generated3', 'padded', 24, 2, 'same'): (0.00123, 5.74e-05, 0.00962),
    ('hand', 'all', 24, 2, 'same'): (0.000689, 0.000439, 0.00802),
    ('hand', 'padded', 24, 2, 'same'): (0.000694, 6.35e-05, 0.00818),
    ('generated7', 'all', 24, 1, 'same'): (0.00152, 0.00114, 0.0436),
    ('generated7', 'all', 24, 3, 'same'): (0.000926, 0.000329, 0.00658),
    ('generated7', 'all', 3, 2, 'same'): (0.000267, 0.000185, 0.0191),
    ('generated7', 'all', 24, 2, 'per_view'): (0.00178, 0.000192, 0.0119),
}
MAX_EXC_EXTRA = 0.005      # the exceptions are a property of the reference; only the candidates vary, by the few pixels whose winners differ
REF_ANALYTIC_OFF, REF_ANALYTIC_OFF_ERR = 0.237, 7.0e-6
# (coverage of the foreground, median relative depth error) of the float64 reference: after max_cost, after the geometric filter as well
REF_ACCURACY = {'photometric': (0.9305, 0.01768), 'geometric': (0.4110, 0.00814)}
SCENES = ('generated7', 'generated3', 'hand')
CASES = [(s, t, D, R, 'same') for s in SCENES for t in ('all', 'padded')] + \
    [('generated7', 'all', D, 1, 'same'), ('generated7', 'all', D, 3, 'same'), ('generated7', 'all', 3, R, 'same'), ('generated7', 'all', D, R, 'per_view')]


TOL_ANALYTIC_COST = 4 * REF_ERR[CASES[0]][0]           # the analytic case has the first case's sizes


def engine_for(backend):
    dev = 'cpu' if backend == 'emu' else 'cuda:0'
    return RenderEngine(dev, _test_lib=emu_lib() if backend == 'emu' else None)


def ring(angles, h, w):
    poses = np.stack([synthetic.look_at_pose(synthetic.sphere_pos(proc.CAMERA_RADIUS, a, e)) for a, e in angles]).astype(np.float32)
    return poses, np.repeat(proc.intrinsics(h, w)[None], len(angles), 0)


@functools.lru_cache(None)
def cameras():
    poses, Ks = ring(ANGLES, H, W)
    for a in (poses, Ks):
        a.setflags(write=False)
    return poses, Ks


@functools.lru_cache(None)
def scene(name):
    if name == 'generated7':
        return proc.make_scene(7, 'black')
    if name == 'generated3':
        return proc.make_scene(3, 'white')
    if name == 'hand':
        return proc.pack_scene(hand_prims(), light=(0.3, -0.2, 1.0), ambient=0.35, background='white')
    raise KeyError(name)


@functools.lru_cache(None)
def table(name):
    if name == 'all':
        t = np.array([[j for j in range(N) if j != i] for i in range(N)], np.int32)
    else:
        t = np.array([[(i + 1) % N, -1, i, (i + 3) % N] for i in range(N)], np.int32)
    t.setflags(write=False)
    return t


@functools.lru_cache(None)
def ranges(name):
    rng = np.repeat(np.array([proc.DEPTH_RANGE], np.float32), N, 0)
    if name == 'per_view':
        rng = rng * np.array([[1.0, 1.0], [0.95, 1.1], [1.05, 0.98], [0.9, 1.2], [1.02, 1.05]], np.float32)
    rng.setflags(write=False)
    return rng


@functools.lru_cache(None)
def views(name):
    """colour [n,3,h,w] and true depth [n,h,w] of the scene, float32 of render_numpy(float64); computed once, read-only"""
    poses, Ks = cameras()
    out = proc.render_numpy(scene(name), poses, Ks, H, W, 1)
    rgb, depth = out['rgb'].astype(np.float32), out['depth'].astype(np.float32)
    rgb.setflags(write=False)
    depth.setflags(write=False)
    return rgb, depth


@functools.lru_cache(None)
def reference(case, dtype='float64'):
    name, tab, planes, radius, rng = case
    poses, Ks = cameras()
    out = stereo.plane_sweep_numpy(views(name)[0], poses, Ks, ranges(rng), table(tab), planes, radius, dtype=np.dtype(dtype), details=True)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(None)
def kernel(backend, case):
    name, tab, planes, radius, rng = case
    poses, Ks = cameras()
    out = engine_for(backend).plane_sweep(views(name)[0], poses, Ks, ranges(rng), table(tab), planes, radius)
    assert out['depth'].dtype == torch.float32 and out['cost'].dtype == torch.float32 and out['plane'].dtype == torch.int32
    assert all(v.shape == (N, H, W) for v in out.values())
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def near_band(ref):
    """[n,D,h,w] bool: on this plane some source's validity flag of this pixel may be decided by rounding"""
    var_min = stereo.VAR_MIN
    with np.errstate(invalid='ignore'):
        near = (np.abs(ref['src_var'] - var_min) < VAR_BAND) | ref['near_edge']          # [n,D,S,h,w]; NaN (no window) compares false
        return near.any(2) | (np.abs(ref['ref_var'] - var_min) < VAR_BAND)[:, None]


def left_out(ref):
    """[n,h,w] bool: the pixels test 2 (d) leaves out - some flag is near its band and no plane has a valid cost clear of every band (such
    a plane settles that there is an estimate) - and their share of the pixels with an estimate"""
    near = near_band(ref)
    settled = (np.isfinite(ref['volume']) & ~near).any(1)
    pix = near.any(1) & ~settled & (ref['ref_var'] >= stereo.VAR_MIN - VAR_BAND)      # (a flat reference window never has an estimate)
    return pix, pix.sum() / max((ref['plane'] >= 0).sum(), 1)


def at_plane(vol, plane):
    return np.take_along_axis(vol, np.maximum(plane, 0)[:, None].astype(np.int64), 1)[:, 0]


def refine_exceptions(ref, case):
    """[n,h,w] bool, decided from the float64 reference alone: the pixels whose refinement may legitimately differ - a validity flag of the
    winning plane or of one of its two neighbours lies in a band (a flag that flips moves that plane's mean by a discrete step), or the
    second difference lies within CURV_BAND = 4 x REF_COST_ERR of its floor (it is the sum of four costs) and may fall on either side"""
    near = near_band(ref)
    k = ref['plane']
    planes = near.shape[1]
    hit = at_plane(near, k) | at_plane(near, np.maximum(k - 1, 0)) | at_plane(near, np.minimum(k + 1, planes - 1))
    with np.errstate(invalid='ignore'):
        return hit | (np.abs(ref['curv'] - stereo.CURV_MIN) < 4 * REF_ERR[case][0])


def refine_candidates(ref, other_plane):
    with np.errstate(invalid='ignore'):
        return (ref['plane'] >= 0) & (other_plane == ref['plane']) & (ref['curv'] > stereo.CURV_MIN)


def offsets(depth, plane, rng, planes):
    """the refined offset in planes that a depth map implies"""
    inv_near, inv_far = 1.0 / rng[:, 0].astype(np.float64), 1.0 / rng[:, 1].astype(np.float64)
    with np.errstate(divide='ignore'):
        t = (1.0 / depth.astype(np.float64) - inv_near[:, None, None]) / (inv_far - inv_near)[:, None, None]
    return t * (planes - 1) - plane


# ---- 1. the reference against itself ---------------------------------------------------------------------------------------------------
def compare_references(case):
    r64, r32 = reference(case), reference(case, 'float32')
    same_flags = (np.isfinite(r64['src_cost']) == np.isfinite(r32['src_cost'])).all(2)      # (a flag that differs changes the mean discretely)
    both = np.isfinite(r64['volume']) & np.isfinite(r32['volume']) & same_flags
    cost_err = float(np.abs(r64['volume'] - r32['volume'])[both].max())
    cand = refine_candidates(r64, r32['plane'])
    exc = cand & refine_exceptions(r64, case)
    sel = cand & ~exc
    depth_err = float((np.abs(r64['depth'] - r32['depth'])[sel] / r64['depth'][sel]).max())
    flags = float((np.isfinite(r64['src_cost']) != np.isfinite(r32['src_cost'])).mean())
    return cost_err, depth_err, flags, left_out(r64)[1], int((r64['plane'] != r32['plane']).sum()), exc.sum() / max(cand.sum(), 1)


def test_reference_float32_agrees_with_float64():
    worst = np.zeros(2)
    for case in CASES:
        cost_err, depth_err, flags, out, planes_differ, exc = compare_references(case)
        print('%r: (%.3g, %.3g, %.3g),   # flags differ %.2e, left out %.4f, winner differs in %d pixels' % (case, cost_err, depth_err, exc, flags, out, planes_differ))
        worst = np.maximum(worst, (flags, out))
        ref_cost, ref_depth, ref_exc = REF_ERR[case]
        assert cost_err <= ref_cost and depth_err <= ref_depth and exc <= ref_exc, case
        assert cost_err >= ref_cost / 2 and depth_err >= ref_depth / 2, case           # the constants are what is measured, not a loose cover
    print('worst: REF_FLAG_SHARE %.3g, REF_LEFT_OUT %.3g' % tuple(worst))
    assert worst[0] <= REF_FLAG_SHARE and worst[1] <= REF_LEFT_OUT <= MAX_LEFT_OUT


def test_reference_recovers_the_scene():
    """the float64 reference itself is stereo: most of the foreground gets a depth near the true one (one plane step is 8 % at D = 24)"""
    ref = reference(CASES[0])
    true = views('generated7')[1]
    ok = (ref['plane'] >= 0) & (ref['cost'] <= 0.5) & (true > 0)
    err = np.abs(ref['depth'] - true)[ok] / true[ok]
    print('coverage %.3f, median relative error %.4f' % (ok.sum() / (true > 0).sum(), np.median(err)))
    assert ok.sum() / (true > 0).sum() > 0.8 and np.median(err) < 0.04


# ---- 2. the kernel against the float64 reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_kernel_against_float64_reference(backend, case):
    ref, got = reference(case), kernel(backend, case)
    planes = case[2]
    TOL_COST, TOL_DEPTH = 4 * REF_ERR[case][0], 4 * REF_ERR[case][1]
    vol = np.where(np.isfinite(ref['volume']), ref['volume'], 1e30)
    drop, share = left_out(ref)
    assert share <= MAX_LEFT_OUT, share
    # (d) an estimate at exactly the reference's pixels
    has_got, has_ref = got['plane'] >= 0, ref['plane'] >= 0
    assert np.array_equal(has_got[~drop], has_ref[~drop])
    assert np.all(got['depth'][~has_got] == 0) and np.all(got['cost'][~has_got] == np.float32(stereo.COST_NONE)) and np.all(got['plane'] < planes)
    assert np.all(np.isfinite(got['depth'])) and np.all(np.isfinite(got['cost']))
    sel = has_got & has_ref
    at = at_plane(vol, got['plane'])
    # (a) the kernel's winner is near-optimal under the reference's volume; (b) its cost is the reference's cost of that plane
    slack = float((at - vol.min(1))[sel].max())
    cost_err = float(np.abs(got['cost'] - at)[sel].max())
    # (c) the refined depth where the winner is the reference's and the reference's parabola applies; the exceptions come from the
    # reference alone, so their share is the one test 1 measured, up to the few pixels whose winners differ
    cand = refine_candidates(ref, got['plane']) & has_got
    exc = cand & refine_exceptions(ref, case)
    fit = cand & ~exc
    assert exc.sum() <= (REF_ERR[case][2] + MAX_EXC_EXTRA) * cand.sum(), exc.sum() / cand.sum()
    depth_err = float((np.abs(got['depth'] - ref['depth'])[fit] / ref['depth'][fit]).max()) if fit.any() else 0.0
    off_got = offsets(got['depth'], got['plane'], ranges(case[4]), planes)
    print('%s %s: left out %.4f, slack %.2e, cost %.2e, refined depth %.2e relative (%d pixels, %d exceptions), winner differs in %d'
          % (backend, case, share, slack, cost_err, depth_err, fit.sum(), exc.sum(), (got['plane'] != ref['plane'])[sel].sum()))
    assert slack <= TOL_COST and cost_err <= TOL_COST and depth_err <= TOL_DEPTH
    assert np.all(np.abs(off_got[sel]) <= 0.5 + 1e-4)


# ---- 3. an analytic case -----------------------------------------------------------------------------------------------------------------
ANALYTIC_K, ANALYTIC_SHIFT = 9, ((20, 0), (0, -16))          # the plane of the face; the sources' shifts on it in whole pixels (x, y)


@functools.lru_cache(None)
def analytic():
    """A box face fronto-parallel to camera 0 (identity pose) at the z-depth d_k of the plane table, seen by two sources that are pure
    translations by a whole number of pixels on that plane: the warp lands on pixel centres and the face is diffuse, so the cost is
    rounding.  -> imgs, poses, Ks, range, table, the pixels well inside the face"""
    rng = np.repeat(np.array([proc.DEPTH_RANGE], np.float32), 3, 0)
    d_k = float(stereo.plane_depths(rng, D)[0, ANALYTIC_K])
    K = proc.intrinsics(H, W)
    poses = np.zeros((3, 3, 4), np.float32)
    poses[:, :, :3] = np.eye(3)
    for s, (mx, my) in enumerate(ANALYTIC_SHIFT):
        poses[s + 1, :, 3] = (mx * d_k / K[0, 0], my * d_k / K[1, 1], 0.0)       # t = -c: the camera moves against the image shift
    rs = np.random.RandomState(5)
    waves = [(rs.uniform(-5.0, 5.0, size=3), rs.uniform(0.0, 6.28), rs.uniform(-0.16, 0.16, size=3)) for _ in range(4)]
    box = {'kind': 'box', 'p': (0.0, 0.0, d_k + 0.25), 'e': (3.0, 2.5, 0.25), 'b': (0.5, 0.5, 0.5), 's': 0.0, 'm': 1.0, 'waves': waves}
    sc = proc.pack_scene([box], light=(0.2, 0.1, -1.0), ambient=0.4, background='black')
    Ks = np.repeat(K[None], 3, 0)
    out = proc.render_numpy(sc, poses, Ks, H, W, 1)
    assert np.all(out['mask'] > 0) and np.allclose(out['depth'], d_k, rtol=1e-6)
    tab = np.array([[1, 2], [-1, -1], [-1, -1]], np.int32)
    inner = np.zeros((H, W), bool)
    inner[R + 4 + 16:H - R - 4, R + 4:W - R - 4 - 20] = True       # (the shifted windows stay inside the sources, also on the planes next to k)
    return out['rgb'].astype(np.float32), poses, Ks, rng, tab, inner


def analytic_offsets(res, rng):
    return offsets(res['depth'][:1], res['plane'][:1], rng[:1], D)[0]


def test_analytic_plane_reference():
    imgs, poses, Ks, rng, tab, inner = analytic()
    r64 = stereo.plane_sweep_numpy(imgs, poses, Ks, rng, tab, D, R, dtype=np.float64, views=(0, 1))
    r32 = stereo.plane_sweep_numpy(imgs, poses, Ks, rng, tab, D, R, dtype=np.float32, views=(0, 1))
    o64, o32 = analytic_offsets(r64, rng)[inner], analytic_offsets(r32, rng)[inner]
    r64d = stereo.plane_sweep_numpy(imgs, poses, Ks, rng, tab, D, R, dtype=np.float64, views=(0, 1), details=True)
    print('analytic: float64 cost max %.2e, |offset| max %.3e, float32 offset differs by %.3e, second difference %.3g .. %.3g' %
          (r64['cost'][0][inner].max(), np.abs(o64).max(), np.abs(o64 - o32).max(), r64d['curv'][0][inner].min(), r64d['curv'][0][inner].max()))
    assert r64d['curv'][0][inner].min() > 2 * stereo.CURV_MIN           # (the parabola applies everywhere inside the face)
    assert np.all(r64['plane'][0][inner] == ANALYTIC_K) and np.all(r32['plane'][0][inner] == ANALYTIC_K)
    assert r64['cost'][0][inner].max() <= TOL_ANALYTIC_COST
    assert np.abs(o64).max() <= REF_ANALYTIC_OFF and np.abs(o64 - o32).max() <= REF_ANALYTIC_OFF_ERR
    assert np.abs(o64).max() >= REF_ANALYTIC_OFF / 2


@pytest.mark.parametrize('backend', BACKENDS)
def test_analytic_plane(backend):
    imgs, poses, Ks, rng, tab, inner = analytic()
    got = {k: v.cpu().numpy() for k, v in engine_for(backend).plane_sweep(imgs, poses, Ks, rng, tab, D, R, views=(0, 1)).items()}
    off = analytic_offsets(got, rng)[inner]
    o64 = analytic_offsets(stereo.plane_sweep_numpy(imgs, poses, Ks, rng, tab, D, R, dtype=np.float64, views=(0, 1)), rng)[inner]
    print('%s analytic: cost max %.2e, |offset| max %.3e, differs from float64 by %.3e' %
          (backend, got['cost'][0][inner].max(), np.abs(off).max(), np.abs(off - o64).max()))
    assert np.all(got['plane'][0][inner] == ANALYTIC_K)
    assert got['cost'][0][inner].max() <= TOL_ANALYTIC_COST
    assert np.abs(off).max() <= REF_ANALYTIC_OFF + 4 * REF_ANALYTIC_OFF_ERR and np.abs(off - o64).max() <= 4 * REF_ANALYTIC_OFF_ERR


# ---- 4. accuracy against the truth ---------------------------------------------------------------------------------------------------------
ACC_H, ACC_W, ACC_D = 80, 112, 64


@functools.lru_cache(None)
def accuracy_views():
    poses, Ks = ring(ANGLES, ACC_H, ACC_W)
    out = proc.render_numpy(scene('generated7'), poses, Ks, ACC_H, ACC_W, 1)
    return out['rgb'].astype(np.float32), out['depth'].astype(np.float32), poses, Ks, np.repeat(np.array([proc.DEPTH_RANGE], np.float32), N, 0)


def accuracy(depth, true):
    ok = (depth > 0) & (true > 0)
    return float(ok.sum() / (true > 0).sum()), float(np.median(np.abs(depth - true)[ok] / true[ok]))


def test_accuracy_of_the_float64_reference():
    imgs, true, poses, Ks, rng = accuracy_views()
    ref = stereo.plane_sweep_numpy(imgs, poses, Ks, rng, table('all'), ACC_D, R, dtype=np.float64)
    photo = np.where(ref['cost'] > 0.5, 0, ref['depth']).astype(np.float32)
    flt = geo.consistency_numpy(photo, poses, Ks, table('all'), dtype=np.float64)
    geom = np.where(flt['count'] >= 2, flt['fused_depth'], 0).astype(np.float32)
    for name, depth in (('photometric', photo), ('geometric', geom)):
        cov, err = accuracy(depth, true)
        print('float64 reference, %s: coverage %.4f, median relative error %.5f' % (name, cov, err))
        assert abs(cov - REF_ACCURACY[name][0]) < 5e-4 and abs(err - REF_ACCURACY[name][1]) < 5e-5


@pytest.mark.parametrize('backend', ['numpy', pytest.param('hip', marks=pytest.mark.gpu)])
def test_accuracy_against_true_depth(backend, monkeypatch):
    imgs, true, poses, Ks, rng = accuracy_views()
    if backend == 'numpy':
        monkeypatch.setattr(proc, '_device_engine', lambda device=None: None)
    for geometric in (False, True):
        est = stereo.estimate_depth(imgs, poses, Ks, rng, table('all'), planes=ACC_D, radius=R, max_cost=0.5, geometric=geometric)
        assert est['depth'].device.type == ('cuda' if backend == 'hip' else 'cpu')
        assert set(est) == {'depth', 'photometric_depth', 'cost', 'plane'} | ({'count'} if geometric else set())
        cov, err = accuracy(est['depth'].cpu().numpy(), true)
        ref_cov, ref_err = REF_ACCURACY['geometric' if geometric else 'photometric']
        print('%s, geometric=%s: coverage %.4f (reference %.4f), median relative error %.5f (reference %.5f)' % (backend, geometric, cov, ref_cov, err, ref_err))
        assert cov >= ref_cov - 0.02 and err <= 1.25 * ref_err


# ---- 5. properties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_two_runs_skipping_and_splitting_give_the_same_bytes(backend):
    case = CASES[1]                                       # (the padded table)
    first = kernel(backend, case)
    poses, Ks = cameras()
    eng = engine_for(backend)
    args = (views(case[0])[0], poses, Ks, ranges(case[4]), table(case[1]), D, R)
    second = {k: v.cpu().numpy() for k, v in eng.plane_sweep(*args).items()}
    noskip = {k: v.cpu().numpy() for k, v in eng.plane_sweep(*args, skip=False).items()}
    halves = [eng.plane_sweep(*args, views=v) for v in ((0, 2), (2, N))]
    for k in first:
        assert np.array_equal(first[k].view(np.int32), second[k].view(np.int32)), k
        assert np.array_equal(first[k].view(np.int32), noskip[k].view(np.int32)), k
        split = torch.cat([h[k] for h in halves]).cpu().numpy()
        assert np.array_equal(first[k].view(np.int32), split.view(np.int32)), k


@pytest.mark.parametrize('backend', BACKENDS)
def test_skipping_far_sources_changes_nothing(backend):
    """a depth range far in front of the scene: most (tile, plane, source) triples project outside the source and are skipped"""
    poses, Ks = cameras()
    rng = np.repeat(np.array([[0.05, 6.0]], np.float32), N, 0)
    eng = engine_for(backend)
    args = (views('generated7')[0], poses, Ks, rng, table('all'), D, R)
    a, b = eng.plane_sweep(*args), eng.plane_sweep(*args, skip=False)
    ref = stereo.plane_sweep_numpy(*args, dtype=np.float32, details=True)
    assert np.isnan(ref['src_cost'][:, :4]).all() and np.isfinite(ref['src_cost']).any()       # (the near planes see nothing at all)
    for k in a:
        assert np.array_equal(a[k].cpu().numpy().view(np.int32), b[k].cpu().numpy().view(np.int32)), k


@pytest.mark.parametrize('backend', BACKENDS)
def test_no_sources_and_constant_images_give_no_estimate(backend):
    poses, Ks = cameras()
    eng = engine_for(backend)
    tab = table('all').copy()
    tab[2] = -1
    out = eng.plane_sweep(views('hand')[0], poses, Ks, ranges('same'), tab, D, R)
    assert torch.all(out['depth'][2] == 0) and torch.all(out['plane'][2] == -1) and torch.all(out['cost'][2] == stereo.COST_NONE)
    assert torch.any(out['plane'][1] >= 0)
    flat = eng.plane_sweep(np.full((N, 3, H, W), 0.4, np.float32), poses, Ks, ranges('same'), table('all'), D, R)
    assert torch.all(flat['depth'] == 0) and torch.all(flat['plane'] == -1)
    ref = stereo.plane_sweep_numpy(np.full((N, 3, H, W), 0.4, np.float32), poses, Ks, ranges('same'), table('all'), D, R, dtype=np.float32)
    assert np.all(ref['plane'] == -1) and np.all(ref['depth'] == 0)


def test_one_source_needs_one_valid_cost():
    poses, Ks = cameras()
    tab = np.full((N, 2), -1, np.int32)
    tab[:, 1] = [(i + 1) % N for i in range(N)]
    ref = stereo.plane_sweep_numpy(views('generated7')[0], poses, Ks, ranges('same'), tab, D, R, dtype=np.float32)
    got = engine_for('emu').plane_sweep(views('generated7')[0], poses, Ks, ranges('same'), tab, D, R)
    assert (ref['plane'] >= 0).mean() > 0.3
    for k in ref:
        assert np.array_equal(got[k].numpy().view(np.int32), ref[k].view(np.int32)), k       # (the emulator follows the float32 reference's order)
    two = stereo.plane_sweep_numpy(views('generated7')[0], poses, Ks, ranges('same'), tab, D, R, dtype=np.float32, min_src=2)
    assert np.all(two['plane'] == -1)


# ---- 6. the surface ----------------------------------------------------------------------------------------------------------------------------
def test_command_line_writes_depth_files(tmp_path, capsys):
    from neuray_amd import estimate_depth
    root = str(tmp_path / 'scene')
    argv = ['--database', 'procedural/7/black_24', '--planes', '8', '--src', '2', '--write', '--root', root]
    res = estimate_depth.main(argv)
    text = capsys.readouterr().out.strip().splitlines()
    line = json.loads(text[-1])
    assert line['views'] == 48 and len(line['written']) == 48 and line['median_rel_error'] is not None and 0 < line['coverage'] <= 1
    assert sum(t.startswith('view ') and 'coverage' in t for t in text) == 48
    db = proc.ProceduralDatabase('procedural/7/black_24')
    maps = stereo.stereo_depth_maps(db, db.get_img_ids(), src=2, planes=8)
    assert maps['depth'].shape == (48, 24, 24) and set(maps) == {'depth', 'imgs', 'poses', 'Ks'}
    first = stereo.depth_path(db, '0', root)
    assert first == res['written'][0] and first.endswith('colmap_depth/0.jpg.geometric.bin')
    for k, p in enumerate(res['written']):
        assert np.array_equal(ndb.read_colmap_array(p).view(np.int32), maps['depth'][k].view(np.int32))
    before = open(first, 'rb').read()
    with pytest.raises(SystemExit):
        estimate_depth.main(argv)
    assert open(first, 'rb').read() == before
    estimate_depth.main(argv + ['--overwrite', '--no-geometric'])
    assert open(first, 'rb').read() != before
    with pytest.raises(SystemExit):
        estimate_depth.main(['--database', 'procedural/7/black_24', '--write'])          # (a database without files needs --root)
    with pytest.raises(SystemExit):
        estimate_depth.main(['--planes', '8'])


@functools.lru_cache(None)
def small_database():
    db = proc.ProceduralDatabase('procedural/7/black_56', n_views=N, h=H, w=W, ss=1)
    db.poses = cameras()[0].copy()
    return db


def test_with_stereo_depth_feeds_build_imgs_info():
    from neuray_amd.pipeline import build_imgs_info
    db = small_database()
    ids = db.get_img_ids()
    maps = stereo.stereo_depth_maps(db, ids, planes=D, geometric=False)
    wrapped = stereo.WithStereoDepth(db, maps, ids)
    info = build_imgs_info(wrapped, ids, has_depth=True)
    assert info['depth'].shape == (N, 1, H, W) and np.array_equal(info['depth'][:, 0], maps['depth']) and (maps['depth'] > 0).mean() > 0.2
    assert np.array_equal(info['imgs'], build_imgs_info(db, ids)['imgs']) and wrapped.get_depth_range(ids[0]).shape == (2,)
    assert not np.array_equal(info['depth'], build_imgs_info(db, ids)['depth'])
    by_id = stereo.WithStereoDepth(db, {ids[1]: maps['depth'][1]})
    assert by_id.get_img_ids(check_depth_exist=True) == [ids[1]] and np.array_equal(by_id.get_depth(ids[1]), maps['depth'][1])
    with pytest.raises(KeyError):
        by_id.get_depth(ids[0])


def test_fuse_mesh_on_stereo_depth():
    """Recorded, not gated: 5 views of 40 x 56, D = 24 (a plane step is 8 % of the depth), voxel 0.04: 1 172 vertices, 1 046 faces, the
    surface_distance of the vertices has median 0.0200 and 95th percentile 0.0772."""
    from neuray_amd import mesh
    db = small_database()
    ids = db.get_img_ids()
    maps = stereo.stereo_depth_maps(db, ids, planes=D)
    out = mesh.fuse_mesh(maps['depth'], maps['imgs'], maps['poses'], maps['Ks'], voxel_size=0.04, filter=False)
    assert out['vertices'].shape[0] > 100 and out['faces'].shape[0] > 100
    dist = geo.surface_distance(db.scene, out['vertices'])
    print('fuse_mesh on stereo depth: %d vertices, %d faces, surface distance median %.4f, 95th percentile %.4f'
          % (out['vertices'].shape[0], out['faces'].shape[0], np.median(dist), np.percentile(dist, 95)))


def test_exporters_take_stereo_depth(tmp_path, capsys):
    from neuray_amd import export_points
    res = export_points.main(['--database', 'procedural/7/black_24', '--depth', 'stereo', '--out', str(tmp_path / 'cloud.ply')])
    assert res['depth'] == 'stereo' and res['views'] == 48
    from neuray_amd import export_mesh, mesh
    out = str(tmp_path / 'mesh.ply')
    res = export_mesh.main(['--database', 'procedural/7/black_24', '--depth', 'stereo', '--voxel', '0.08', '--out', out])
    assert res['depth'] == 'stereo' and res['views'] == 48 and res['vertices'] > 0 and res['faces'] > 0
    assert mesh.read_mesh_ply(out)['vertices'].shape == (res['vertices'], 3)


def test_argument_errors():
    poses, Ks = cameras()
    imgs, rng, tab = views('hand')[0], ranges('same'), table('all')
    eng = engine_for('emu')
    for sweep in (lambda *a, **k: stereo.plane_sweep_numpy(*a, dtype=np.float32, **k), eng.plane_sweep):
        for planes, radius in ((2, 2), (257, 2), (24, 0), (24, 4)):
            with pytest.raises(ValueError):
                sweep(imgs, poses, Ks, rng, tab, planes, radius)
        with pytest.raises(ValueError):
            sweep(imgs, poses, Ks, rng, np.full((N, 17), -1, np.int32), D, R)
        with pytest.raises(ValueError):
            sweep(imgs, poses, Ks, rng, np.zeros((N, 0), np.int32), D, R)
        with pytest.raises(ValueError):
            sweep(imgs, poses[:4], Ks, rng, tab, D, R)
        with pytest.raises(ValueError):
            sweep(imgs, poses, Ks, rng[:, :1], tab, D, R)
        with pytest.raises(ValueError):
            sweep(imgs[:, :2], poses, Ks, rng, tab, D, R)
        with pytest.raises(ValueError):
            sweep(imgs[:, :, :4], poses, Ks, rng, tab, D, R)          # (no room for a window)
        with pytest.raises(ValueError):
            sweep(imgs, poses, Ks, rng[:, ::-1], tab, D, R)           # (near >= far)
        with pytest.raises(ValueError):
            sweep(imgs, poses, Ks, rng, tab, D, R, views=(3, 3))
    with pytest.raises(ValueError):
        stereo.estimate_depth(imgs, poses, Ks, rng, tab, planes=2)
    # the C entry checks the same, and a missing buffer
    import ctypes as C
    from neuray_amd import _lib
    for bad in (dict(planes=2), dict(planes=257), dict(radius=4), dict(n_src=17), dict(v1=9)):
        a = dict(n=N, h=H, w=W, n_src=4, planes=D, radius=R, v0=0, v1=N, var_min=1e-5)
        a.update(bad)
        with pytest.raises(RuntimeError):
            eng._check(eng.lib.neuray_plane_sweep(C.byref(_lib.NeurayPlaneSweepArgs(**a)), eng._stream()))
    with pytest.raises(RuntimeError, match='missing'):
        eng._check(eng.lib.neuray_plane_sweep(C.byref(_lib.NeurayPlaneSweepArgs(n=N, h=H, w=W, n_src=4, planes=D, radius=R, v0=0, v1=N, var_min=1e-5)), eng._stream()))


def test_other_variants_raise_not_implemented():
    poses, Ks = cameras()
    eng = engine_for('emu')
    eng.variant = 'bf16'
    with pytest.raises(NotImplementedError):
        eng.plane_sweep(views('hand')[0], poses, Ks, ranges('same'), table('all'), D, R)
