"""The pair sites of the point kernel - the bilinear blends blend8 / blend_rgb, the scaled ELU of apply_act2 and the vector rows of
layer_vec (csrc/nr_device.h) - exist in a packed (v_pk_mul_f32 / v_pk_fma_f32) and in a scalar form (two v_mul_f32 / v_fma_f32 in the
same order), chosen per arithmetic by NR_PK_BLEND / NR_PK_ELU / NR_PK_VEC (csrc/nr_platform.h).  Each half of a
packed instruction is the IEEE result of the scalar operation, so whichever form a site takes the results stay what they were:

  * the self-test kernel evaluates every site in BOTH forms on the same inputs, one set per lane of a wave: equal bits for every lane
    and value (random, mixed magnitudes, cancellation, signed zeros, denormals, +-inf and NaN, mask 0 and 1) - on the CPU emulator
    build and, marked gpu, on the device;
  * the smallest render that runs every tile body of the point kernel (two-, one- and zero-slot, with 8 and with 7 views), under both
    arithmetics, against the emulator build of the same kernels with the gates tests/test_x3_arith.py / tests/test_render_parity.py
    hold between a render and its reference (the emulator itself is held to the numpy oracle with the same gates).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import load_weights
from emu_util import emu_lib
from test_render_parity import BACKENDS, TOL_HIT, TOL_PIXEL, make_renderer

N_IN, N_OUT = 67, 17
OUT_NAMES = ['blend8[%d]' % i for i in range(8)] + ['blend_rgb[%d]' % i for i in range(3)] + ['elu[0]', 'elu[1]'] + \
            ['vec_partial[0]', 'vec_partial[1]', 'vec[0]', 'vec[1]']


def inputs():
    """name -> x [67][64] (value-major: x[i][l] is input i of lane l; layout in csrc/nr_kernels.h pair_forms_selftest_kernel)"""
    g = torch.Generator().manual_seed(23)
    out = {}
    x = torch.randn(N_IN, 64, generator=g)
    x[32:36] = torch.rand(4, 64, generator=g)                       # bilinear weights
    x[36] = (torch.arange(64) % 3 != 0).float()                     # mask 0 and 1
    out['random'] = x
    x = torch.randn(N_IN, 64, generator=g) * torch.pow(10.0, torch.randint(-30, 31, (N_IN, 64), generator=g).float())
    x[36] = (torch.arange(64) % 2).float()
    x[37:39] = torch.randn(2, 64, generator=g) * torch.pow(10.0, torch.randint(-3, 3, (2, 64), generator=g).float())    # ELU arguments on both sides of exp2's range
    out['mixed'] = x
    # cancellation: the four taps / the row's products sum to almost nothing, so the last bits of every product and sum show
    x = torch.randn(N_IN, 64, generator=g)
    x[32:36] = 0.25
    x[36] = 1.0
    for i in range(4):                                              # taps 4..7 (float4 index) = -(taps 0..3) (1 + 2^-20)
        x[16 + 4 * i:20 + 4 * i] = -x[4 * i:4 * i + 4] * (1.0 + 2.0 ** -20)
    x[8:16] = -x[0:8] * (1.0 - 2.0 ** -21)
    x[59:63] = x[55:59]
    x[43:47] = -x[39:43] * (1.0 + 2.0 ** -22)                       # row 0: second tile's weights against the first's
    x[51:55] = -x[47:51] * (1.0 - 2.0 ** -19)
    out['cancel'] = x
    x = torch.randn(N_IN, 64, generator=g)
    x[32:36] = torch.rand(4, 64, generator=g)
    x[36] = (torch.arange(64) % 2).float()
    x[0:8, ::2] = 0.0
    x[8:16, ::3] = -0.0
    x[16:24] = torch.tensor(1.0e-41) * torch.randn(8, 64, generator=g)            # denormals
    x[24:32] = torch.tensor(3.0e-39) * torch.randn(8, 64, generator=g)
    x[33, ::4] = -0.0
    x[37] = torch.where(torch.arange(64) % 2 == 0, torch.tensor(0.0), torch.tensor(-0.0))
    x[38] = torch.tensor(2.0e-40) * torch.randn(64, generator=g)
    x[39:43, ::2] = -0.0
    x[55:59] = torch.tensor(5.0e-42) * torch.randn(4, 64, generator=g)
    x[47:51] = 1.0e30
    x[59:63] = 1.0e-38
    out['zeros_denormals'] = x
    x = torch.randn(N_IN, 64, generator=g)
    x[32:36] = torch.rand(4, 64, generator=g)
    x[36] = (torch.arange(64) % 2).float()
    inf, nan = float('inf'), float('nan')
    special = torch.tensor([inf, -inf, nan, 3.0e38, -3.0e38, 0.0, -0.0, 1.0])
    for i in range(N_IN):
        if i == 36:
            continue
        sel = (torch.arange(64) + 3 * i) % 11                       # a special value in some lanes of every input, in turn
        x[i] = torch.where(sel < 8, special[sel.clamp(max=7)], x[i])
    x[32:36, 48:] = torch.rand(4, 16, generator=g)                  # lanes 48..63: finite weights, special taps
    out['inf_nan'] = x
    return out


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', ['random', 'mixed', 'cancel', 'zeros_denormals', 'inf_nan'])
def test_packed_and_scalar_forms_agree_bit_for_bit(name, backend):
    from neuray_amd.engine import RenderEngine
    dev = 'cpu' if backend == 'emu' else 'cuda:0'
    eng = RenderEngine(dev, _test_lib=emu_lib() if backend == 'emu' else None)
    x = inputs()[name]
    assert x.shape == (N_IN, 64)
    xd, yd = x.to(dev).contiguous(), torch.full((2, N_OUT, 64), 12345.0, device=dev)
    assert eng.lib.neuray_pair_forms_selftest(xd.data_ptr(), yd.data_ptr(), eng._stream()) == 0
    if backend == 'hip':
        torch.cuda.synchronize()
    y = _bits(yd)
    assert not np.any(y == np.float32(12345.0).view(np.uint32)) or name == 'inf_nan', 'every value is written'
    nan = np.isnan(yd.cpu().numpy())
    assert np.array_equal(nan[0], nan[1])
    for i in range(N_OUT):                                          # bit patterns: -0.0, denormals, inf; NaN against NaN
        same = (y[0, i] == y[1, i]) | (nan[0, i] & nan[1, i])
        assert same.all(), '%s: lanes %s, packed %s scalar %s' % (OUT_NAMES[i], np.nonzero(~same)[0][:4], y[0, i][~same][:4], y[1, i][~same][:4])
    if name == 'random':                                            # and the values are the blends / rows they claim to be
        v = yd[0].cpu().double()
        xx = x.double()
        w = xx[32:36] * xx[36]
        taps = xx[0:32].view(8, 4, 64)                              # [float4 index][component][lane]
        for h in range(2):
            want = sum(taps[2 * k + h] * w[k] for k in range(4))    # q[h], q[2+h], q[4+h], q[6+h] with w00, w10, w01, w11
            assert torch.allclose(v[4 * h:4 * h + 4], want, atol=1e-5)
        want_rgb = sum(taps[k][:3] * w[k] for k in range(4))
        assert torch.allclose(v[8:11], want_rgb, atol=1e-5)
        log2e = 1.4426950408889634
        e = xx[37:39]
        assert torch.allclose(v[11:13], torch.where(e > 0, e, log2e * (torch.exp2(e) - 1.0)), atol=1e-5)
        rows = xx[39:55].view(2, 8, 64)                             # [row][feature][lane]
        part = (rows * xx[55:63][None]).sum(1)
        assert torch.allclose(v[13:15], part, atol=1e-5)
        gs = part.view(2, 4, 16).sum(1).repeat(1, 4) + xx[63:65]
        assert torch.allclose(v[15:17], gs, atol=1e-4)


# ---- the smallest render that runs every tile body ------------------------------------------------------------------------------------
RN, DN, FDN, SIZE = 40, 4, 4, 32
AWAY = (2, 3, 5)          # views moved sideways until nothing projects into their images: slots (tile, view) fully masked
CFG = {'use_hierarchical_sampling': True, 'dist_decoder_cfg': {'use_vis': False}, 'depth_sample_num': DN, 'fine_depth_sample_num': FDN,
       'agg_net_cfg': {'sample_num': DN}, 'fine_agg_net_cfg': {'sample_num': DN + FDN}}


def scene(rfn):
    """40 rays (two full 16-ray blocks and a partial one) on 32 x 32 images.  Waves hold the view pairs (0, 1), (2, 3), (4, 5), (6, 7 or
    padding): views 2, 3 and 5 see nothing, so every tile runs the two-slot body (wave 0; wave 3 with 8 views), the zero-slot body (wave 1)
    and the one-slot body (wave 2; wave 3 with 7 views, where slot 1 is the padding)."""
    from oracle import neuray_oracle as orc
    que, ref = orc.make_scene(SIZE, SIZE, rfn, seed=3)
    for v in AWAY:
        ref['poses'][v, 0, 3] += 50.0
    rng = np.random.RandomState(5)
    que['coords'] = (4.0 + rng.rand(1, RN, 2) * (SIZE - 9.0)).astype(np.float32)
    return que, ref


def render(rfn, arith, backend):
    """-> (outputs of render_impl as numpy, slot statistics (view slots run, view slots) of the two point-kernel launches)"""
    que, ref = scene(rfn)
    r, dev = make_renderer({**CFG, 'hip_arith': arith}, load_weights(False), backend)
    eng = r.engine(dev)
    tq = {k: torch.from_numpy(v).to(dev) for k, v in que.items()}
    tr = {k: torch.from_numpy(v).to(dev) for k, v in ref.items()}
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    eng.slot_stats = stats
    torch.manual_seed(1234)
    with torch.no_grad():
        got = r.render_impl(tq, tr, False)
    eng.slot_stats = None
    return {k: v.cpu().numpy() for k, v in got.items()}, tuple(int(v) for v in stats.cpu())


@functools.lru_cache(maxsize=None)
def emu_render(rfn, arith):
    return render(rfn, arith, 'emu')


def check_slots(stats, rfn):
    """every tile of every launch counted ran exactly the bodies scene() is built for: 2 + 0 + 1 + (2 or 1) of its 8 view slots"""
    run, slots = stats
    per_tile = {8: 2 + 0 + 1 + 2, 7: 2 + 0 + 1 + 1}[rfn]
    blocks = (RN + 15) // 16
    assert slots % (8 * blocks) == 0 and slots >= 8 * blocks * (DN + FDN), stats         # whole tiles; at least the merged fine launch
    assert run * 8 == slots * per_tile, stats


@pytest.mark.parametrize('arith', ['x3', 'f32'])
@pytest.mark.parametrize('rfn', [8, 7])
def test_emulator_render_runs_every_body_and_matches_the_oracle(rfn, arith):
    from oracle import neuray_oracle as orc
    got, stats = emu_render(rfn, arith)
    check_slots(stats, rfn)
    que, ref = scene(rfn)
    want = orc.render_impl(load_weights(False), dict(CFG, coarse_use_vis=False, fine_use_vis=True), que, ref)
    assert np.abs(got['pixel_colors_nr'] - want['pixel_colors_nr']).max() <= TOL_PIXEL
    assert np.abs(got['hit_prob_nr'] - want['hit_prob_nr']).max() <= TOL_HIT


@pytest.mark.gpu
@pytest.mark.parametrize('arith', ['x3', 'f32'])
@pytest.mark.parametrize('rfn', [8, 7])
def test_device_render_matches_the_emulator_build(rfn, arith):
    """the gates of tests/test_x3_arith.py::test_x3_render_matches_the_reference with the emulator build of the same kernels as the
    reference: coarse pass direct, fine pass chained (fine-sample placement amplifies fp32-level noise on near-empty rays)"""
    want, _ = emu_render(rfn, arith)
    got, stats = render(rfn, arith, 'hip')
    check_slots(stats, rfn)
    assert np.abs(got['pixel_colors_nr'] - want['pixel_colors_nr']).max() <= TOL_PIXEL
    assert np.abs(got['hit_prob_nr'] - want['hit_prob_nr']).max() <= TOL_HIT
    assert np.array_equal(got['ray_mask'], want['ray_mask'])
    err = np.max(np.abs(got['pixel_colors_nr_fine'] - want['pixel_colors_nr_fine']), -1)
    assert np.mean(err <= TOL_PIXEL) >= 0.95 and err.max() <= 5e-3, (float(np.mean(err <= TOL_PIXEL)), float(err.max()))
    assert np.array_equal(got['ray_mask_fine'], want['ray_mask_fine'])
