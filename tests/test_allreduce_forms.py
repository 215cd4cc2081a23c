"""The cross-view all-reduce of the point kernel exists in two forms (csrc/nr_device.h): block_allreduce - partial rows, barrier,
reduce-scatter, reduced rows, barrier, read back - and block_allreduce_1b - partial rows into one of two LDS banks, ONE barrier, then
every wave sums the nw partials of every row itself, in the same wave order.  The X3 instantiation takes the one-barrier form up to six
waves (csrc/nr_kernels.h point_one_barrier); NEURAY_POINT_ALLREDUCE=2 forces the two-barrier form from the same library.  Whichever
form a launch takes, the results stay what they were:

  * the self-test kernel runs the kernel's own sequence of a tile (12, 11, 11, 11 rows summed, 2 rows with row 0 the maximum, 12, 8
    rows summed) twice - 14 calls, the bank parity wraps across an odd count - in both forms on the same inputs, with nw = 4, 5, 6 and 2
    waves that idle for wave- and call-dependent times between the calls (fast waves run a whole all-reduce ahead of slow ones): equal
    bits in every wave and lane, equal to a host combination in wave order - on the CPU emulator build and, marked gpu, on the device;
  * the smallest render that runs the two-, one- and zero-slot bodies under X3 (the scene of tests/test_pair_forms.py) in both forms
    through the launcher hook: torch.equal on every returned tensor, and on the product against the per-view-record instantiation.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from conftest import load_weights
from emu_util import emu_lib
from test_pair_forms import CFG, check_slots, scene
from test_render_parity import BACKENDS, make_renderer

CALLS = [(12, 'sum'), (11, 'sum'), (11, 'sum'), (11, 'sum'), (2, 'max0'), (12, 'sum'), (8, 'sum')] * 2      # (rows, combination) of the 14 calls
RMAX = 12
SENTINEL = 12345.0


@contextlib.contextmanager
def allreduce_form(form):
    """form 2: the launcher's A/B hook forces two barriers; form 1: the launcher's own choice"""
    old = os.environ.pop('NEURAY_POINT_ALLREDUCE', None)
    if form == 2:
        os.environ['NEURAY_POINT_ALLREDUCE'] = '2'
    try:
        yield
    finally:
        os.environ.pop('NEURAY_POINT_ALLREDUCE', None)
        if old is not None:
            os.environ['NEURAY_POINT_ALLREDUCE'] = old


def inputs(nw):
    """name -> x [14][nw][12][64]"""
    g = torch.Generator().manual_seed(31 + nw)
    shape = (len(CALLS), nw, RMAX, 64)
    out = {'random': torch.randn(shape, generator=g)}
    out['mixed'] = torch.randn(shape, generator=g) * torch.pow(10.0, torch.randint(-30, 31, shape, generator=g).float())
    # cancelling pairs: wave 2 k + 1 holds -(wave 2 k) (1 + 2^-20) - the sum's last bits depend on the order of the waves
    x = torch.randn(shape, generator=g)
    for w in range(1, nw, 2):
        x[:, w] = -x[:, w - 1] * (1.0 + 2.0 ** -20)
    out['cancel'] = x
    x = torch.randn(shape, generator=g)
    x[:, :, :, ::2] = 0.0
    x[:, :, :, ::3] = -0.0
    x[:, ::2, :, 5::7] = -0.0                       # some rows: -0 in some waves, +0 in others
    out['signed_zeros'] = x
    x = torch.randn(shape, generator=g)
    inf = float('inf')
    special = torch.tensor([inf, -inf, 3.0e38, -3.0e38])
    sel = (torch.arange(64)[None, None, None, :] + 3 * torch.arange(RMAX)[None, None, :, None] + 5 * torch.arange(nw)[None, :, None, None] +
           torch.arange(len(CALLS))[:, None, None, None]) % 13
    out['inf'] = torch.where(sel < 4, special[sel.clamp(max=3)], x)        # +inf and -inf meet in some sums (NaN), overflow in others
    return out


def host_combination(x):
    """-> [14][12][64] fp32: the nw inputs of every row combined in wave order 0..nw-1 (rows beyond a call's count: NaN)"""
    xs = x.numpy()
    want = np.full((len(CALLS), RMAX, 64), np.nan, np.float32)
    with np.errstate(all='ignore'):
        for c, (rows, op) in enumerate(CALLS):
            for r in range(rows):
                s = xs[c, 0, r].copy()
                for w in range(1, xs.shape[1]):
                    s = np.maximum(s, xs[c, w, r]) if (op == 'max0' and r == 0) else (s + xs[c, w, r]).astype(np.float32)
                want[c, r] = s
    return want


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('nw', [4, 5, 6, 2])
def test_both_forms_agree_bit_for_bit_and_with_the_host(nw, backend):
    from neuray_amd.engine import RenderEngine
    dev = 'cpu' if backend == 'emu' else 'cuda:0'
    eng = RenderEngine(dev, _test_lib=emu_lib() if backend == 'emu' else None)
    for name, x in inputs(nw).items():
        xd = x.to(dev).contiguous()
        yd = torch.full((2, len(CALLS), nw, RMAX, 64), SENTINEL, device=dev)
        assert eng.lib.neuray_allreduce_selftest(xd.data_ptr(), yd.data_ptr(), nw, eng._stream()) == 0
        if backend == 'hip':
            torch.cuda.synchronize()
        y = yd.cpu().numpy()
        bits = y.view(np.uint32)
        want = host_combination(x)
        for c, (rows, op) in enumerate(CALLS):
            where = '%s, nw %d, call %d' % (name, nw, c)
            assert np.array_equal(bits[0, c, :, :rows], bits[1, c, :, :rows]), where + ': the two forms differ'
            assert np.all(y[:, c, :, rows:] == np.float32(SENTINEL)), where + ': a row beyond the count was written'
            for form in range(2):
                for w in range(nw):                                     # every wave holds the result
                    got = y[form, c, w, :rows]
                    if op == 'max0':                                    # (row 0, the maximum: by value - max(-0, +0) has no order)
                        assert np.array_equal(got[0], want[c, 0]), where
                        got, ref = got[1:], want[c, 1:rows]
                    else:
                        ref = want[c, :rows]
                    nan = np.isnan(ref)
                    assert np.array_equal(np.isnan(got), nan), where
                    assert np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]), '%s, form %d, wave %d' % (where, form, w)


# ---- the smallest render that runs every tile body, in both forms -----------------------------------------------------------------------
def render(rfn, backend, form):
    """-> (outputs of render_impl, slot statistics) of the X3 render of test_pair_forms.scene"""
    que, ref = scene(rfn)
    r, dev = make_renderer({**CFG, 'hip_arith': 'x3'}, load_weights(False), backend)
    eng = r.engine(dev)
    tq = {k: torch.from_numpy(v).to(dev) for k, v in que.items()}
    tr = {k: torch.from_numpy(v).to(dev) for k, v in ref.items()}
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    eng.slot_stats = stats
    torch.manual_seed(1234)
    with allreduce_form(form), torch.no_grad():
        got = r.render_impl(tq, tr, False)
        if backend == 'hip':
            torch.cuda.synchronize()
    eng.slot_stats = None
    return {k: v.cpu() for k, v in got.items()}, tuple(int(v) for v in stats.cpu())


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('rfn', [8, 7])
def test_render_is_bit_identical_in_both_forms(rfn, backend):
    one, stats1 = render(rfn, backend, 1)
    two, stats2 = render(rfn, backend, 2)
    check_slots(stats1, rfn)                                            # the two-, one- and zero-slot bodies all ran
    assert stats1 == stats2
    assert set(one) == set(two)
    for k in one:
        assert torch.equal(one[k], two[k]), k


@pytest.mark.parametrize('backend', BACKENDS)
def test_product_matches_the_record_instantiation_in_both_forms(backend):
    """slot skipping + transposed tiles (product) against every slot evaluated + tiles along the ray (per-view record), each in both forms"""
    que, ref = scene(8)
    r, dev = make_renderer({**CFG, 'hip_arith': 'x3'}, load_weights(False), backend)
    eng = r.engine(dev)
    tq = {k: torch.from_numpy(v).to(dev) for k, v in que.items()}
    tr = {k: torch.from_numpy(v).to(dev) for k, v in ref.items()}
    rn = que['coords'].shape[1]
    depth = eng.sample_coarse_depth(tq['depth_range'], rn, CFG['depth_sample_num'])
    qc, views = eng.prepare_query(tq), eng.prepare_views(tr)
    packed = r._packed_pass(eng, False)
    assert packed.dev_x3 is not None
    res = []
    for form in (1, 2):
        with allreduce_form(form):
            for dbg in (False, True):
                o = eng.render_pass(qc, views, tq['coords'][0], depth, packed, use_vis=False, want_dbg=dbg)
                if backend == 'hip':
                    torch.cuda.synchronize()
                res.append({k: o[k].cpu() for k in ('point_rec', 'pixel', 'hit_prob')})
    for o in res[1:]:
        for k in ('point_rec', 'pixel', 'hit_prob'):
            assert torch.equal(res[0][k], o[k]), k
