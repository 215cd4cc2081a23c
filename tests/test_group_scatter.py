"""The batched lane-group sums of the point kernel's narrow rows (neuray_amd/csrc/nr_platform.h nr_group_scatter4 / nr_group_gather4 and
their two-value forms): summing four partial-sum registers together and gathering the totals back must return, in every lane, exactly the
four nr_group_sum results - (g0 + g1) + (g2 + g3) bit for bit -, so that the two-slot tile body (batched) and the one-slot body and the
training forward (single sums) compute the same numbers.

Runs on the CPU emulator and, marked gpu, on the device (v_permlane16_swap / v_permlane32_swap exchanging DIFFERENT registers)."""
import numpy as np
import pytest
import torch

from emu_util import emu_lib

BACKENDS = ['emu', pytest.param('hip', marks=pytest.mark.gpu)]


def inputs():
    g = torch.Generator().manual_seed(11)
    out = {'randn': torch.randn(4, 64, generator=g)}
    # mixed signs and magnitudes: the order of the additions shows in the low bits (and in what survives cancellation)
    mag = torch.pow(10.0, torch.randint(-6, 7, (4, 64), generator=g).float())
    out['mixed'] = torch.randn(4, 64, generator=g) * mag
    x = torch.randn(4, 64, generator=g)
    x[:, 16:32] = -x[:, 0:16] * (1.0 + 2.0 ** -20)          # g0 + g1 cancels almost completely
    x[:, 32:48] *= 1e-7
    x[:, 48:64] *= 1e5
    out['cancel'] = x
    x = torch.randn(4, 64, generator=g)
    x[0] = 0.0
    x[1, ::3] = -0.0
    x[2] = torch.arange(64).float() * 2.0 ** -30 + 1.0
    x[3] = torch.where(torch.arange(64) % 2 == 0, torch.tensor(3.0e38), torch.tensor(-3.0e38))      # overflows in one order only
    out['special'] = x
    return out


def group_sum(x):
    """[n][64] -> [n][16]: (g0 + g1) + (g2 + g3) in fp32, the association of nr_group_sum"""
    g = x.view(-1, 4, 16)
    return (g[:, 0] + g[:, 1]) + (g[:, 2] + g[:, 3])


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', ['randn', 'mixed', 'cancel', 'special'])
def test_group_scatter_gather(name, backend):
    from neuray_amd.engine import RenderEngine
    dev = 'cpu' if backend == 'emu' else 'cuda:0'
    eng = RenderEngine(dev, _test_lib=emu_lib() if backend == 'emu' else None)
    x = inputs()[name]
    xd, yd = x.to(dev).contiguous(), torch.full((7, 64), float('nan'), device=dev)
    assert eng.lib.neuray_group_scatter_selftest(xd.data_ptr(), yd.data_ptr(), eng._stream()) == 0
    if backend == 'hip':
        torch.cuda.synchronize()
    y = yd.cpu()
    want = group_sum(x)                                   # [4][16]
    # the single-value form on the same inputs is the definition
    for j in range(4):
        sd = torch.zeros(64, device=dev)
        assert eng.lib.neuray_group_sum_selftest(xd[j].contiguous().data_ptr(), sd.data_ptr(), eng._stream()) == 0
        assert np.array_equal(sd.cpu().numpy().view(np.uint32), want[j].repeat(4).numpy().view(np.uint32)), 'nr_group_sum itself, value %d' % j
    bits = lambda t: t.contiguous().numpy().view(np.uint32)      # noqa: E731  (bit patterns: -0.0, inf)
    for j in range(4):                                    # four-value form + all-gather: every lane, every value
        assert np.array_equal(bits(y[j]), bits(want[j].repeat(4))), 'four-value form, value %d' % j
    for j in range(2):                                    # two-value form + its gather
        assert np.array_equal(bits(y[4 + j]), bits(want[j].repeat(4))), 'two-value form, value %d' % j
    assert np.array_equal(bits(y[6]), bits(want.reshape(64))), 'the scattered register: total j in lane group j'
