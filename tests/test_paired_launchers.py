"""Each *_det entry of the C ABI is its namesake's launcher with scratch (neuray_hip.hip): one host function per pair.

  1. both entries of the six pairs refuse the same bad calls, each under its own name;
  2. the deterministic ray backward at the gates of test_backward.test_rays_backward_matches_autograd, beyond 64 samples too (two samples
     per lane, an LDS accumulator per wave: a layout no other small test runs)."""
import ctypes as C

import pytest
import torch

import test_backward
from emu_util import emu_lib
from test_backward import BACKENDS
from neuray_amd import _lib
from neuray_amd.engine import RenderEngine


@pytest.mark.parametrize('backend', BACKENDS)
def test_paired_entries_refuse_the_same_calls_under_their_own_names(backend):
    """A missing array and a bad shape, on both entries of every pair: refused, and the message names the symbol that was called.  Host code
    only: every call returns before a launch, so one-element buffers stand for every array."""
    dev = 'cpu' if backend == 'emu' else 'cuda:0'
    eng = RenderEngine(dev, _test_lib=emu_lib() if backend == 'emu' else None)
    lib, s = eng.lib, eng._stream()
    P = torch.zeros(1, device=dev).data_ptr()

    def refused(name, rc):
        assert rc != 0, name
        assert lib.neuray_last_error().startswith(name.encode() + b':'), (name, lib.neuray_last_error())

    def pair(name, call, n_scratch=1):
        """call(fn, scratch, null, bad): fn with its arguments, one required array NULL if `null`, a bad shape if `bad`"""
        for sym, scratch in ((name, ()), (name + '_det', (P,) * n_scratch)):
            for null, bad in ((True, False), (False, True)):
                refused(sym, call(getattr(lib, sym), scratch, null, bad))

    def rays(fn, scratch, null, bad):
        a = _lib.NeurayRaysBwdArgs(*([P] * 9), 1, 2 if bad else 3, P)
        a.point_rec_dev = None if null else P
        return fn(C.byref(a), *scratch, s)

    def points(fn, scratch, null, bad):
        a = _lib.NeurayPointsBwdArgs(*([P] * 12), 2, 1, 2 if bad else 3, 8, 8, 2, 2, 0, 0, 0.05, P, P, P, P)
        a.coords_dev = None if null else P
        return fn(C.byref(a), *scratch, s)

    def self_hit(fn, scratch, null, bad):
        return fn(P, P, P, P, P, 0, 0, 0.05, None if null else P, 1, 2 if bad else 3, P, P, *scratch, s)

    def rows(fn, scratch, null, bad):
        return fn(None if null else P, P, P, 0 if bad else 1, 0, 0.05, P, P, P, None, P, P, *scratch, s)

    def norm_forward(fn, scratch, null, bad):          # (pad >= h)
        return fn(P, None if null else P, P, None, 0, 0, 0, 1, 1, 2, 2, 2 if bad else 1, 0, 1e-5, *scratch, P, P, P, 0, s)

    def norm_backward(fn, scratch, null, bad):
        return fn(P, P, 0, P, 0, None if null else P, P, 1, 1, 2, 2, 2 if bad else 1, 0, *scratch, P, P, None, None, None, s)

    pair('neuray_render_rays_backward', rays)
    pair('neuray_render_points_backward', points, n_scratch=3)          # partials, rows, keys
    pair('neuray_self_hit_prob_backward', self_hit)
    pair('neuray_dist_decoder_rows_backward', rows)
    pair('neuray_inorm_forward', norm_forward)
    pair('neuray_inorm_backward', norm_backward)


# one shape per samples-per-lane instantiation, and the first and the last dn of the two-samples one
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('rn,dn,with_aux', [(3, 7, True), (2, 65, True), (3, 128, True)])
def test_rays_backward_matches_autograd_deterministic(rn, dn, with_aux, backend, monkeypatch):
    """test_backward.test_rays_backward_matches_autograd itself - its inputs, its float64 autograd reference, its tolerances - with every
    ray backward it runs taken through neuray_render_rays_backward_det"""
    plain, calls = RenderEngine.render_rays_backward, []

    def deterministic(self, *a, **k):
        before = self.det_scratch_bytes
        out = plain(self, *a, deterministic=True, **k)
        calls.append(self.det_scratch_bytes - before)
        return out

    monkeypatch.setattr(RenderEngine, 'render_rays_backward', deterministic)
    test_backward.test_rays_backward_matches_autograd(rn, dn, with_aux, backend)
    assert len(calls) == 2 and min(calls) > 0          # (recomputed and saved attention statistics: both through the partials buffer)
