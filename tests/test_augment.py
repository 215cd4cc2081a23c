"""Depth-noise and ray-sampling augmentation of the procedural stream (neuray_amd/procedural.py, csrc/nr_kernels_aug.h):
the Philox function against Random123's known answers, the three kernels against procedural.augment_numpy / stats_numpy and against the
definition of the ray selection (np.lexsort on the composites), the stream with and without augmentation, one training step.

Engine-level cases: 5 views of 40 x 56 (neither a multiple of a wave nor of the 1024-pixel chunk of the selection: three workgroups, the last
one partial), views 1 .. 3 the working views.  View 0: a blob; 1: a mask touching all four borders; 2: one pixel; 3: empty; 4: a blob with
depth values outside (1e-3, 1e4) inside it.

Tolerance of the depth ranges.  It comes from the reference alone: augment_numpy(float32) against augment_numpy(float64) over RANGE_CASES
and SHRINK_CASES (test_reference_float32_agrees_with_float64 measures and asserts it on the CPU).  Worst value measured: 5.84e-7 absolute (on
ranges of 1 .. 10).  The gate is 4 x that - the device's division may round differently from numpy's: TOL_RANGE = 2.34e-6.  Everything
behind the ranges (plan, noisy depth, coordinates) is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

from emu_util import emu_lib
from neuray_amd import procedural as proc
from neuray_amd.engine import RenderEngine

BACKENDS = ['emu', pytest.param('hip', marks=pytest.mark.gpu)]
H, W, N, RFN, VIEW0 = 40, 56, 5, 3, 1
KEY = (12345, 7)
REF_RANGE_ERR = 5.85e-7                          # float32 reference against float64 reference, worst over the cases (see the docstring)
TOL_RANGE = 4 * REF_RANGE_ERR


@functools.lru_cache(None)
def engine_for(backend):
    dev = 'cpu' if backend == 'emu' else 'cuda:0'
    return RenderEngine(dev, _test_lib=emu_lib() if backend == 'emu' else None), dev


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(None)
def maps():
    """(mask [N,H,W] uint8, depth [N,H,W] float32), read-only"""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    mask = np.zeros((N, H, W), np.uint8)
    mask[0] = ((xs - 30) ** 2 + 2 * (ys - 17) ** 2 < 150) | ((abs(xs - 12) < 4) & (abs(ys - 30) < 5))
    mask[1] = (abs(xs - ys) < 9) | (abs(xs + ys - 70) < 4) | ((ys == H - 1) & (xs < 3)) | ((ys < 2) & (xs == W - 1))
    mask[2, 23, 41] = 1
    mask[4] = ((xs - 20) ** 2 + (ys - 20) ** 2 < 120)
    assert mask[1][0].any() and mask[1][-1].any() and mask[1][:, 0].any() and mask[1][:, -1].any() and not mask[3].any()
    depth = ((3.0 + 0.013 * xs + 0.021 * ys)[None] + 0.1 * np.arange(N)[:, None, None]).astype(np.float32) * (mask > 0)
    for (y, x), d in zip(((20, 20), (21, 20), (22, 21), (14, 18), (25, 25)), (0.0, 1e-4, 2e4, 1e4, 1e-3)):
        assert mask[4, y, x]
        depth[4, y, x] = d                       # (1e4 and 1e-3 themselves are outside the open interval)
    return frozen(mask, depth)


def host_numbers(head, views, large=(0.05, 0.1, 0.5, 1.0, 0.1)):
    """head: (shrink, u_far, u_near, widen, u0, u1, consistent); views: per working view ((on, u_c, u_lx, u_ly, u_off, neg) x 2, global)"""
    out = np.zeros((1 + len(views), proc.AUG_HOST), np.float32)
    out[0, :7], out[0, 8:13] = head, large
    for r, (big, small, glob) in enumerate(views):
        out[1 + r, :6], out[1 + r, 6:12], out[1 + r, 12] = big, small, glob
    return out.reshape(-1)


def u24(x):
    return round(x * 2 ** 24) / 2.0 ** 24        # a uniform as the host draws it: a multiple of 2^-24


OFF = (0, 0, 0, 0, 0, 0)
ALL_OFF = [(OFF, OFF, 0)] * RFN
# non-equal input ranges: view 1 is the longest after the augmentation, view 0 takes the near * 0.5 clamp (its margin exceeds half its near),
# the others the margin branch
RANGES_A = np.array([[2.6, 6.0], [1.5, 8.0], [2.0, 7.5], [1.8, 7.0], [2.4, 7.4]], np.float32)
RANGE_CASES = [
    ('shrink+widen+consistent', (1, u24(0.3), u24(0.6), 1, u24(0.2), u24(0.9), 1)),
    ('widen+consistent', (0, 0, 0, 1, u24(0.7), u24(0.1), 1)),
    ('consistent', (0, 0, 0, 0, 0, 0, 1)),
    ('shrink', (1, u24(0.5), u24(0.5), 0, 0, 0, 0)),
]
# the shrink branches, plain numbers: every valid masked depth lies in [3, 4] (shrink_maps), all views share one range
SHRINK_CASES = [('far only', (3.0, 8.0)), ('near only', (2.0, 4.0)), ('neither', (3.0, 4.0)), ('both', (2.0, 8.0))]
U_FAR, U_NEAR = 0.25, 0.75


@functools.lru_cache(None)
def shrink_maps():
    mask, _ = maps()
    depth = np.where(mask > 0, np.float32(3.5), np.float32(0))
    for v in (0, 1, 4):
        ys, xs = np.nonzero(mask[v])
        depth[v, ys[0], xs[0]], depth[v, ys[-1], xs[-1]] = 3.0 + 0.25 * (v == 1), 4.0 - 0.25 * (v == 4)
    return frozen(mask, depth.astype(np.float32))


def kernel_depth(backend, mask, depth, ranges, host, key=KEY):
    eng, dev = engine_for(backend)
    t_depth = torch.tensor(depth).to(dev)
    before = t_depth.clone()
    stats = eng.augment_stats(torch.tensor(mask).to(dev), t_depth)
    out = eng.augment_depth(t_depth, torch.tensor(mask).to(dev), ranges, stats, host, key, VIEW0, RFN)
    assert torch.equal(t_depth, before)                                   # the exact maps (true_depth) are inputs only
    assert out['depth_range_aug'].shape == (N, 2) and out['depth_range'].shape == (N, 2) and out['plan'].shape == (RFN, 2, 8)
    assert out['depth_aug'].shape == (RFN, H, W) and all(v.dtype == torch.float32 for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. Philox ------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """the three vectors of Random123's kat_vectors for philox4x32-10"""
    f = 0xffffffff
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((f, f, f, f), (f, f), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = proc.philox4x32(np.array(ctr, np.uint32), key)
        assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want
    # vectorised: a batch of counters gives the rows of the single calls
    ctrs = np.array([[0, 0, 0, 0], [f, f, f, f], [5, 1, 3, 0]], np.uint32)
    batch = proc.philox4x32(ctrs, (f, f))
    assert batch.shape == (3, 4) and tuple(int(x) for x in batch[1]) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert np.array_equal(batch[2], proc.philox4x32(ctrs[2], (f, f)))


def test_defaults_are_the_reference_s():
    want = {'aug_gso_shrink_range_prob': 0.5, 'aug_use_depth_offset': True, 'aug_depth_offset_prob': 0.25, 'aug_depth_offset_region_min': 0.05,
            'aug_depth_offset_region_max': 0.1, 'aug_depth_offset_min': 0.5, 'aug_depth_offset_max': 1.0, 'aug_depth_offset_local': 0.1,
            'aug_use_depth_small_offset': True, 'aug_depth_small_offset_prob': 0.5, 'aug_use_global_noise': True, 'aug_global_noise_prob': 0.5,
            'foreground_ratio': 0.5, 'use_consistent_depth_range': True}
    assert proc.AUGMENT_DEFAULTS == want
    assert proc.augment_config(None) is None and proc.augment_config(False) is None and proc.augment_config(True) == want
    assert proc.augment_config({'foreground_ratio': 0.25})['foreground_ratio'] == 0.25
    with pytest.raises(KeyError):
        proc.augment_config({'no_such_key': 1})
    host = proc.augment_host_numbers(np.random.RandomState(3), RFN, want).reshape(1 + RFN, proc.AUG_HOST)
    assert host.dtype == np.float32
    draws = np.concatenate([host[0, [1, 2, 4, 5]], host[1:, 1:5].ravel(), host[1:, 7:11].ravel()])
    assert np.all((draws >= 0) & (draws < 1)) and np.all(draws * 2 ** 24 == np.round(draws * 2 ** 24))
    assert set(np.unique(host[0, [0, 3, 6]])) | set(np.unique(host[1:, [0, 5, 6, 11, 12]])) <= {0.0, 1.0} and host[0, 6] == 1


# ---- 2. statistics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_stats_equal_numpy(backend):
    mask, depth = maps()
    eng, dev = engine_for(backend)
    got = eng.augment_stats(torch.tensor(mask).to(dev), torch.tensor(depth).to(dev))
    want = proc.stats_numpy(mask, depth)
    for k in ('count', 'bbox', 'row_counts'):
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), want[k]), k
    for k in ('depth_min', 'depth_max'):
        assert same_bits(got[k].cpu().numpy(), want[k]), k
    # ... and numpy against the cases by hand: all four borders, one pixel, empty (the sentinels), invalid depth left out
    assert tuple(want['bbox'][1]) == (0, W - 1, 0, H - 1)
    assert want['count'][2] == 1 and tuple(want['bbox'][2]) == (41, 41, 23, 23) and want['depth_min'][2] == want['depth_max'][2] == depth[2, 23, 41]
    assert want['count'][3] == 0 and tuple(want['bbox'][3]) == (W, -1, H, -1) and want['depth_min'][3] == np.inf and want['depth_max'][3] == -np.inf
    inside = depth[4][mask[4] > 0]
    assert inside.min() == 0 and inside.max() == 2e4 and 3 < want['depth_min'][4] < want['depth_max'][4] < 5
    assert want['count'][4] == int(mask[4].sum()) and want['row_counts'].sum() == int(mask.sum())
    # a float mask (the stream's `masks`) is compared with 0 the same way
    again = eng.augment_stats(torch.tensor(mask.astype(np.float32)).to(dev)[:, None], torch.tensor(depth).to(dev)[:, None])
    assert torch.equal(again['stats'], got['stats']) and torch.equal(again['row_counts'], got['row_counts'])


# ---- 3. depth: where the tolerance comes from ---------------------------------------------------------------------------------------------
def shrink_expectation(near, far):
    """the range augmentation of SHRINK_CASES by hand, in float64: depth extrema 3 and 4 exactly"""
    far_ratio, near_ratio = 1.1 * 4.0 / far, near / (0.9 * 3.0)
    if far_ratio < 1:
        far = far * (far_ratio + (1 - far_ratio) * U_FAR)
    if near_ratio < 1:
        near = near / (near_ratio + (1 - near_ratio) * U_NEAR)
    return near, far


def test_reference_float32_agrees_with_float64():
    worst = 0.0
    mask, depth = maps()
    for name, head in RANGE_CASES:
        host = host_numbers(head, ALL_OFF)
        a, b = (proc.augment_numpy(depth, mask, RANGES_A, host, KEY, VIEW0, RFN, dtype=T) for T in (np.float32, np.float64))
        assert a['depth_range'].dtype == np.float32 and b['depth_range'].dtype == np.float64
        for k in ('depth_range_aug', 'depth_range'):
            worst = max(worst, float(np.max(np.abs(a[k].astype(np.float64) - b[k]))))
        if head[6]:                              # both branches of consistent_depth_range are taken, by the views the comment names
            near, far = b['depth_range_aug'][:, 0], b['depth_range_aug'][:, 1]
            margin = ((far - near).max() - (far - near)) / 2
            assert margin[0] > 0.5 * near[0] and np.all(margin[1:] < 0.5 * near[1:]) and (margin[2:] > 0).all()
            assert np.allclose(b['depth_range'][0, 0], 0.5 * near[0]) and np.allclose(b['depth_range'][2:, 0], (near - margin)[2:])
            assert np.allclose(b['depth_range'][:, 1] - b['depth_range'][:, 0], (far - near).max())
    smask, sdepth = shrink_maps()
    for name, (near, far) in SHRINK_CASES:
        host = host_numbers((1, U_FAR, U_NEAR, 0, 0, 0, 0), ALL_OFF)
        rng = np.repeat(np.array([[near, far]], np.float32), N, 0)
        a, b = (proc.augment_numpy(sdepth, smask, rng, host, KEY, VIEW0, RFN, dtype=T) for T in (np.float32, np.float64))
        worst = max(worst, float(np.max(np.abs(a['depth_range'].astype(np.float64) - b['depth_range']))))
        assert np.allclose(b['depth_range'], np.repeat([shrink_expectation(near, far)], N, 0), rtol=1e-7, atol=0), name
    print('worst |float32 - float64| of the ranges: %.3e' % worst)
    # the gate is 4 x what was measured when it was written down; the measurement still holds
    assert worst <= REF_RANGE_ERR * 1.0001


# ---- 3A. ranges against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name,head', RANGE_CASES)
def test_ranges_match_the_float64_reference(name, head, backend):
    mask, depth = maps()
    host = host_numbers(head, ALL_OFF)
    got = kernel_depth(backend, mask, depth, RANGES_A, host)
    want = proc.augment_numpy(depth, mask, RANGES_A, host, KEY, VIEW0, RFN, dtype=np.float64)
    for k in ('depth_range_aug', 'depth_range'):
        err = float(np.max(np.abs(got[k].astype(np.float64) - want[k])))
        print('%s [%s] %s: %.3e' % (name, backend, k, err))
        assert err <= TOL_RANGE, k
    if not head[0] and not head[3]:
        assert same_bits(got['depth_range_aug'], RANGES_A)
    if not head[6]:
        assert same_bits(got['depth_range'], got['depth_range_aug'])


# ---- 3D. the shrink branches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name,rng', SHRINK_CASES)
def test_shrink_branches(name, rng, backend):
    """far_ratio = 4.4 / far, near_ratio = near / 2.7 over the views with a valid depth (the empty view 3 takes no part, view 2's single pixel
    3.5 does): far only (0.55 < 1 <= 1.11), near only (0.74 < 1 <= 1.1), neither, both"""
    smask, sdepth = shrink_maps()
    host = host_numbers((1, U_FAR, U_NEAR, 0, 0, 0, 0), ALL_OFF)
    ranges = np.repeat(np.array([rng], np.float32), N, 0)
    got = kernel_depth(backend, smask, sdepth, ranges, host)
    near, far = shrink_expectation(*rng)
    assert (near == rng[0]) == (name in ('far only', 'neither')) and (far == rng[1]) == (name in ('near only', 'neither'))
    assert np.max(np.abs(got['depth_range_aug'].astype(np.float64) - np.array([near, far]))) <= TOL_RANGE
    if near == rng[0]:
        assert np.all(got['depth_range_aug'][:, 0] == np.float32(rng[0]))       # an untouched side is untouched: the same bits
    if far == rng[1]:
        assert np.all(got['depth_range_aug'][:, 1] == np.float32(rng[1]))
    assert same_bits(got['depth_range'], got['depth_range_aug'])
    # with the shrink decision off nothing moves
    off = kernel_depth(backend, smask, sdepth, ranges, host_numbers((0, U_FAR, U_NEAR, 0, 0, 0, 0), ALL_OFF))
    assert same_bits(off['depth_range_aug'], ranges)


# ---- 3B / 3C. plan and noisy depth, bit for bit ----------------------------------------------------------------------------------------------
HEAD_B = (1, u24(0.3), u24(0.6), 1, u24(0.2), u24(0.9), 1)
NOISE_CASES = {
    # view 1 (all four borders): centre rank 0 = its top-left pixel, the region crosses the image border; a negative large offset
    'both on, global on': [((1, 0.0, u24(0.9), u24(0.8), u24(0.4), 1), (1, u24(0.55), u24(0.3), u24(0.7), u24(0.5), 0), 1),
                           ((1, u24(0.5), u24(0.5), u24(0.5), u24(0.5), 0), (1, u24(0.99), u24(0.1), u24(0.2), u24(0.3), 1), 1),     # one pixel: empty regions
                           ((1, u24(0.5), u24(0.5), u24(0.5), u24(0.5), 0), (1, u24(0.2), u24(0.1), u24(0.2), u24(0.3), 1), 1)],     # empty mask: no region
    'both on, global off': [((1, u24(0.999999), u24(0.9), u24(0.8), u24(0.4), 0), (1, u24(0.41), u24(0.99), u24(0.99), u24(0.0), 1), 0),
                            ((1, 0.0, u24(0.5), u24(0.5), u24(0.5), 1), (1, 0.0, u24(0.1), u24(0.2), u24(0.3), 0), 0),
                            ((1, 0.0, 0.0, 0.0, 0.0, 0), (1, 0.0, 0.0, 0.0, 0.0, 0), 0)],
    'both off, global off': ALL_OFF,
    'one each': [((1, u24(0.37), u24(0.2), u24(0.6), u24(0.1), 1), OFF, 0), (OFF, (1, u24(0.5), u24(0.5), u24(0.5), u24(0.5), 0), 1), (OFF, OFF, 1)],
}


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', sorted(NOISE_CASES))
def test_plan_and_noisy_depth_equal_the_float32_reference_bit_for_bit(name, backend):
    mask, depth = maps()
    views = NOISE_CASES[name]
    host = host_numbers(HEAD_B, views)
    got = kernel_depth(backend, mask, depth, RANGES_A, host)
    want = proc.augment_numpy(depth, mask, RANGES_A, host, KEY, VIEW0, RFN, dtype=np.float32, depth_range_aug=got['depth_range_aug'])
    assert same_bits(got['plan'], want['plan'])
    assert same_bits(got['depth_aug'], want['depth_aug'])
    assert same_bits(got['depth_range'], want['depth_range'])       # (the same operations on the same float32 inputs)
    plan, exact = got['plan'], depth[VIEW0:VIEW0 + RFN]
    L = got['depth_range_aug'][VIEW0:VIEW0 + RFN, 1] - got['depth_range_aug'][VIEW0:VIEW0 + RFN, 0]
    assert same_bits(plan[:, :, 7], np.repeat(L[:, None], 2, 1))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    for r, (big, small, glob) in enumerate(views):
        count = int((mask[VIEW0 + r] > 0).sum())
        inside = np.zeros((H, W), bool)
        for k, reg in enumerate((big, small)):
            on = bool(reg[0]) and count > 0
            assert plan[r, k, 0] == (1.0 if on else 0.0)
            if not on:
                assert not plan[r, k, :7].any()
                continue
            cx, cy = int(plan[r, k, 1]), int(plan[r, k, 2])
            assert mask[VIEW0 + r, cy, cx] and (plan[r, k, 5] < 0) == bool(reg[5]) and plan[r, k, 5] != 0
            region = (mask[VIEW0 + r] > 0) & (abs(xs - cx) < plan[r, k, 3]) & (abs(ys - cy) < plan[r, k, 4])
            assert region.any() == (count > 1)                        # a one-pixel mask: lx = ly = 0, an empty region
            inside |= region
        if not glob:                                                  # C: outside every region the exact map, bit for bit
            assert same_bits(got['depth_aug'][r][~inside], exact[r][~inside])
            assert np.all(got['depth_aug'][r][inside] != exact[r][inside])
        else:                                                         # the global noise reaches every pixel, the background included
            bound = np.float32(0.005) * L[r] + 1e-6                   # (+ the rounding of the sum)
            diff = got['depth_aug'][r][~inside] - exact[r][~inside]
            assert np.all(np.abs(diff) <= bound) and np.mean(diff != 0) > 0.99 and np.abs(diff[mask[VIEW0 + r][~inside] == 0]).max() > 0.5 * bound
    if name == 'both on, global on':
        assert (plan[0, 0, 1], plan[0, 0, 2]) == (0.0, 0.0) and plan[0, 0, 3] > 1 and plan[0, 0, 5] < 0        # the corner region, negative
    if name == 'both on, global off':                                 # rank int(u count) = count - 1: the last foreground pixel
        ys1, xs1 = np.nonzero(mask[VIEW0])
        assert (plan[0, 0, 1], plan[0, 0, 2]) == (xs1[-1], ys1[-1])
    if name == 'both off, global off':
        assert same_bits(got['depth_aug'], exact)


# ---- 4. ray coordinates ---------------------------------------------------------------------------------------------------------------------
def coords_by_lexsort(mask, ray_num, ratio, key, view):
    """the definition: the k smallest composites (word, pixel), stage by stage"""
    h, w = mask.shape
    ctr = np.zeros((h * w, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = np.arange(h * w), view, 3
    words = proc.philox4x32(ctr, key)
    p = np.arange(h * w)
    fg = mask.reshape(-1) > 0
    k1 = min(int(ray_num * ratio), int(fg.sum()))
    order1 = np.lexsort((p, words[:, 0]))
    pick1 = np.sort(order1[fg[order1]][:k1])
    left = np.ones(h * w, bool)
    left[pick1] = False
    order2 = np.lexsort((p, words[:, 1]))
    pick2 = np.sort(order2[left[order2]][:ray_num - k1])
    pix = np.concatenate([pick1, pick2])
    return np.stack([pix % w, pix // w], -1)[None].astype(np.float32), k1


def coord_masks():
    mask, _ = maps()
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    small = np.zeros((H, W), np.uint8)
    small[5, 3:9] = small[31, 50:54] = 1
    return {'half': (xs < W // 2).astype(np.uint8), 'small': small, 'all': np.ones((H, W), np.uint8), 'empty': mask[3], 'blob': mask[0]}


COORD_CASES = [('half', 64, 0.5), ('small', 64, 0.5), ('all', 64, 0.5), ('empty', 64, 0.5), ('blob', 64, 0.0), ('blob', 64, 1.0),
               ('small', 64, 1.0), ('half', H * W, 0.5), ('blob', 1, 0.5), ('blob', 301, 0.3)]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name,ray_num,ratio', COORD_CASES)
def test_coords_equal_the_k_smallest_composites(name, ray_num, ratio, backend):
    eng, dev = engine_for(backend)
    mask = coord_masks()[name]
    view = 2
    got = eng.sample_coords(torch.tensor(mask).to(dev), ray_num, ratio, KEY, view=view)
    assert got.shape == (1, ray_num, 2) and got.dtype == torch.float32
    got = got.cpu().numpy()
    want, k1 = coords_by_lexsort(mask, ray_num, ratio, KEY, view)
    assert np.array_equal(got, want)
    assert np.array_equal(proc.sample_coords_numpy(mask, ray_num, ratio, KEY, view), want)
    x, y = got[0, :, 0].astype(int), got[0, :, 1].astype(int)
    assert np.all((x >= 0) & (x < W) & (y >= 0) & (y < H)) and np.all(got == np.floor(got))
    assert len(set(zip(x.tolist(), y.tolist()))) == ray_num                     # distinct pixels
    assert k1 == min(int(ray_num * ratio), int(mask.sum())) and np.all(mask[y[:k1], x[:k1]] > 0)
    pix = y * W + x
    assert np.all(np.diff(pix[:k1]) > 0) and np.all(np.diff(pix[k1:]) > 0)      # each stage in row-major order
    if name == 'all':
        assert k1 == 32
    if name == 'small':                                                         # all of the foreground, topped up from the pool
        assert k1 == 10 and set(pix[:k1]) == set(np.flatnonzero(mask.reshape(-1)))
    # another key or view: another draw
    if ray_num < H * W:
        assert not np.array_equal(eng.sample_coords(torch.tensor(mask).to(dev), ray_num, ratio, (KEY[0], KEY[1] + 1), view=view).cpu().numpy(), got)
        assert not np.array_equal(eng.sample_coords(torch.tensor(mask).to(dev), ray_num, ratio, KEY, view=view + 1).cpu().numpy(), got)


@pytest.mark.parametrize('backend', BACKENDS)
def test_the_entry_points_check_their_arguments(backend):
    eng, dev = engine_for(backend)
    mask, depth = maps()
    t_mask = torch.tensor(mask).to(dev)
    with pytest.raises(RuntimeError, match='ray_num='):
        eng.sample_coords(t_mask[0], H * W + 1, 0.5, KEY)
    with pytest.raises(RuntimeError, match='ray_num='):
        eng.sample_coords(t_mask[0], 0, 0.5, KEY)
    with pytest.raises(RuntimeError, match='want_fg='):
        eng.sample_coords(t_mask[0], 8, 1.5, KEY)
    with pytest.raises(ValueError):
        proc.sample_coords_numpy(mask[0], H * W + 1, 0.5, KEY)
    stats = eng.augment_stats(t_mask, torch.tensor(depth).to(dev))
    with pytest.raises(RuntimeError, match='working views'):
        eng.augment_depth(torch.tensor(depth), t_mask, RANGES_A, stats, host_numbers(HEAD_B, ALL_OFF + ALL_OFF), KEY, 3, RFN)
    for entry in ('neuray_augment_stats', 'neuray_augment_depth', 'neuray_sample_coords'):
        with pytest.raises(RuntimeError, match='null args'):
            eng._check(getattr(eng.lib, entry)(None, eng._stream()))


def test_the_bf16_variants_refuse():
    from emu_util import emu_lib_bf16
    eng = RenderEngine('cpu', _test_lib=emu_lib_bf16(), variant='bf16')
    mask, depth = maps()
    with pytest.raises(NotImplementedError):
        eng.augment_stats(mask, depth)
    with pytest.raises(NotImplementedError):
        eng.sample_coords(mask[0], 8, 0.5, KEY)
    for entry in ('neuray_augment_stats', 'neuray_augment_depth', 'neuray_sample_coords'):
        with pytest.raises(RuntimeError, match='fp32 library'):
            eng._check(getattr(eng.lib, entry)(None, eng._stream()))


# ---- 5. the stream -----------------------------------------------------------------------------------------------------------------------
SH, SW, SRFN, SEXTRA, SRAYS, SSEED = 48, 64, 3, 1, 64, 0


def make_stream(backend, **kw):
    eng, dev = engine_for(backend)
    return proc.ProceduralStream(dev, seed=SSEED, h=SH, w=SW, rfn=SRFN, extra_src=SEXTRA, rays=SRAYS, engine=eng, **kw)


def flat(batch):
    return {(part, k): v for part in ('que_imgs_info', 'ref_imgs_info', 'src_imgs_info') for k, v in batch[part].items()}


def batches_equal(a, b):
    fa, fb = flat(a), flat(b)
    return a['scene_name'] == b['scene_name'] and set(fa) == set(fb) and all(torch.equal(fa[k], fb[k]) for k in fa)


@pytest.mark.parametrize('backend', BACKENDS)
def test_stream_with_augmentation(backend):
    plain, aug = make_stream(backend), make_stream(backend, augment=True)
    n = 1 + SRFN + SEXTRA
    for index in range(4):
        p, a = next(plain), next(aug)
        pq, pr, ps, aq, ar, as_ = (b[k] for b in (p, a) for k in ('que_imgs_info', 'ref_imgs_info', 'src_imgs_info'))
        # scene, cameras and neighbours of the batch are the plain stream's, bit for bit
        assert a['scene_name'] == p['scene_name']
        for x, y in ((pq, aq), (pr, ar), (ps, as_)):
            assert set(x) == set(y)
            for k in ('imgs', 'masks', 'poses', 'Ks', 'Ks_inv', 'nn_ids', 'true_depth'):
                if k in x:
                    assert torch.equal(x[k], y[k]), k
        assert pr['depth'].data_ptr() == pr['true_depth'].data_ptr() and ar['depth'].data_ptr() != ar['true_depth'].data_ptr()
        assert torch.equal(aq['depth'], pq['depth'])
        masks = torch.cat([aq['masks'], ar['masks']])[:, 0].cpu().numpy()
        exact = torch.cat([aq['depth'], ar['true_depth']])[:, 0].cpu().numpy()
        fg = masks.reshape(1 + SRFN, -1).sum(1)
        assert np.all((fg > 1100) & (fg < 1900))                                  # want_fg = 32 foreground pixels are always there
        # the exact maps of all views: the extra source view's come from the plain batch's stats
        last = aug.last_augment
        stats = {k: last['stats'][k].cpu().numpy() for k in ('count', 'bbox', 'depth_min', 'depth_max', 'row_counts')}
        want_stats = proc.stats_numpy(masks, exact)
        for k in stats:
            assert np.array_equal(stats[k][:1 + SRFN], want_stats[k]), k
        assert 2.7 < stats['depth_min'].min() and stats['depth_max'].max() < 5.7
        near_ratio, far_ratio = (2.0 / (0.9 * stats['depth_min'])).max(), (1.1 * stats['depth_max'] / 6.0).max()
        assert near_ratio < 1 and (far_ratio < 1 if index == 1 else True) and (far_ratio >= 1 if index == 3 else True)
        # the ranges: finite, ordered, consistent, the slices of one array; against float64 on the working set of views
        host, key = last['host'], last['key']
        assert key == (SSEED, index)
        rng_all = torch.cat([aq['depth_range'], as_['depth_range']]).cpu().numpy()
        assert rng_all.shape == (n, 2) and np.all(np.isfinite(rng_all)) and np.all((0 < rng_all[:, 0]) & (rng_all[:, 0] < rng_all[:, 1]))
        assert torch.equal(ar['depth_range'], as_['depth_range'][:SRFN])
        assert np.ptp(rng_all[:, 1] - rng_all[:, 0]) <= 4 * TOL_RANGE
        # augment_numpy on the batch's exact maps (the extra view's map: rendered again, plainly)
        eng, dev = engine_for(backend)
        sc, poses, _, _ = aug.host_batch(index)
        full = eng.procedural_render(sc, poses, np.repeat(aug.K[None], n, 0), SH, SW, 1, outputs=('depth', 'mask'))
        f_depth, f_mask = full['depth'].cpu().numpy(), full['mask'].cpu().numpy()
        assert np.array_equal(f_depth[:1 + SRFN], exact) and np.array_equal(f_mask[:1 + SRFN] > 0, masks > 0)
        rng_in = np.repeat(np.asarray(proc.DEPTH_RANGE, np.float32)[None], n, 0)
        range_aug = last['depth_range_aug'].cpu().numpy()
        w64 = proc.augment_numpy(f_depth, f_mask, rng_in, host, key, 1, SRFN, dtype=np.float64)
        assert np.max(np.abs(range_aug - w64['depth_range_aug'])) <= TOL_RANGE and np.max(np.abs(rng_all - w64['depth_range'])) <= TOL_RANGE
        w32 = proc.augment_numpy(f_depth, f_mask, rng_in, host, key, 1, SRFN, dtype=np.float32, depth_range_aug=range_aug)
        plan = last['plan'].cpu().numpy()
        assert same_bits(plan, w32['plan']) and same_bits(ar['depth'][:, 0].cpu().numpy(), w32['depth_aug']) and same_bits(rng_all, w32['depth_range'])
        # depth differs from true_depth where the plan says
        H_ = host.reshape(1 + SRFN, proc.AUG_HOST)
        for r in range(SRFN):
            changed = (ar['depth'][r, 0] != ar['true_depth'][r, 0]).cpu().numpy()
            if H_[1 + r, 12]:
                assert changed.mean() > 0.99
            elif not plan[r, :, 0].any():
                assert not changed.any()
            else:
                assert changed.any() and not changed[masks[1 + r] == 0].any()
        # the rays: the kernel's, half of them on the query view's foreground
        coords = aq['coords'].cpu().numpy()
        assert coords.shape == (1, SRAYS, 2) and np.array_equal(coords, proc.sample_coords_numpy(masks[0], SRAYS, 0.5, key, 0))
        assert np.all(masks[0][coords[0, :SRAYS // 2, 1].astype(int), coords[0, :SRAYS // 2, 0].astype(int)] > 0)
        assert not np.array_equal(coords, pq['coords'].cpu().numpy())


@pytest.mark.parametrize('backend', BACKENDS)
def test_stream_without_augmentation_is_unchanged_and_seeds_repeat(backend):
    ref = next(make_stream(backend))
    for kw in ({'augment': None}, {'augment': False}):
        assert batches_equal(next(make_stream(backend, **kw)), ref)
    a, b = make_stream(backend, augment=True), make_stream(backend, augment={'aug_global_noise_prob': 0.5})
    first = next(a)
    assert batches_equal(first, next(b)) and not batches_equal(first, ref)
    assert not batches_equal(next(a), first)
    # a dict overrides the defaults: no noise at all, every ray from the foreground
    quiet = next(make_stream(backend, augment={'aug_use_depth_offset': False, 'aug_use_depth_small_offset': False, 'aug_use_global_noise': False,
                                                'foreground_ratio': 1.0, 'use_consistent_depth_range': False}))
    qr, qq = quiet['ref_imgs_info'], quiet['que_imgs_info']
    assert torch.equal(qr['depth'], qr['true_depth']) and qr['depth'].data_ptr() != qr['true_depth'].data_ptr()
    c = qq['coords'][0].long()
    assert bool((qq['masks'][0, 0][c[:, 1], c[:, 0]] > 0).all())


# ---- 6. one training step --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_augmented_batch_trains_a_generalisation_step():
    """the sample is consumable: NeuralRayGenRenderer with render + depth loss on an augmented batch (the small configuration of
    tests/test_procedural.py's training test); no threshold"""
    from test_procedural import GEN_CFG
    from neuray_amd.loss import name2loss, total_loss
    from neuray_amd.network.renderer import NeuralRayGenRenderer
    dev = torch.device('cuda:0')
    stream = proc.ProceduralStream(dev, seed=5, h=64, w=96, rfn=2, extra_src=2, rays=64, augment=True)
    next(stream)
    batch = next(stream)
    ref = batch['ref_imgs_info']
    assert ref['depth'] is not ref['true_depth'] and ref['depth'].shape == ref['true_depth'].shape == (2, 1, 64, 96)
    assert tuple(batch['que_imgs_info']['coords'].shape) == (1, 64, 2) and batch['que_imgs_info']['coords'].device == dev
    torch.manual_seed(0)
    np.random.seed(0)
    model = NeuralRayGenRenderer(GEN_CFG).train().to(dev)
    losses = [name2loss['render']({'use_nr_fine_loss': True}), name2loss['depth']({})]
    out = model({k: dict(v) if isinstance(v, dict) else v for k, v in batch.items()})
    total, log = total_loss(losses, out, batch, 0)
    assert {'loss_rgb_nr', 'loss_rgb_nr_fine', 'loss_depth', 'loss_depth_fine'} <= set(log) and bool(torch.isfinite(total))
    assert float(log['loss_depth'].detach().float().mean()) > 0
    total.backward()
    grads = [p.grad for p in model.parameters() if p.requires_grad and p.grad is not None]
    assert len(grads) > 20 and all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
