"""The fused InstanceNorm in the deterministic mode (fused_norm.DETERMINISTIC): the plane statistics of the forward and of
the backward are per-workgroup partials added in workgroup order instead of float atomics.  Three runs are bitwise equal, the result
stays inside the gates of tests/test_fused_norm.py against its float64 composition, and the statistics ARE the float32 sum of the kernel's
own block partials in block order."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from test_fused_norm import BACKENDS, composed, device      # noqa: F401  (the fixture)
from neuray_amd.network import fused_norm
from neuray_amd.network import render_ops as ro


@pytest.fixture(autouse=True)
def _switch(monkeypatch):
    monkeypatch.delenv('NEURAY_HIP_DETERMINISTIC', raising=False)
    fused_norm.DETERMINISTIC, fused_norm.RENDERER_DETERMINISTIC = True, False
    yield
    fused_norm.DETERMINISTIC = False


def _ordered_sum(part):
    """[planes, chunks, 2] -> [planes, 2]: float32 adds in chunk order"""
    s = part[:, 0].copy()
    for k in range(1, part.shape[1]):
        s = s + part[:, k]
    return s


# n * c = 9 * 32 planes: 200 x 200 (15 workgroups per plane), 50 x 50 (3), 30 x 30 (one workgroup per plane)
@pytest.mark.parametrize('device', BACKENDS, indirect=True)
@pytest.mark.parametrize('hw,chunks', [((200, 200), 15), ((50, 50), 3), ((30, 30), 1)])
def test_deterministic_norm_repeats_and_sums_its_partials_in_block_order(device, hw, chunks):
    n, c, (h, w), pad, act = 9, 32, hw, 1, 'relu'
    g = torch.Generator().manual_seed(h + w)
    bn = nn.InstanceNorm2d(c, affine=True, track_running_stats=False)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
    y0 = torch.randn(n, c, h, w, generator=g) * 2 + 3 * torch.randn(1, c, 1, 1, generator=g)
    dz = torch.randn(n, c, h + 2 * pad, w + 2 * pad, generator=g)
    eng = ro.engine_for(device)
    assert eng.lib.neuray_inorm_chunks(n, c, h, w) == chunks
    eng.keep_norm_partials = True

    runs = []
    mod = bn.to(device)
    for _ in range(3):
        for p_ in mod.parameters():
            p_.grad = None
        y = y0.clone().to(device).requires_grad_(True)
        out = fused_norm.norm_act(mod, y, act, pad, None)
        fwd = tuple(t.cpu().numpy().copy() for t in eng.norm_partials['forward'])
        (out * dz.to(device)).sum().backward()
        bwd = tuple(t.cpu().numpy().copy() for t in eng.norm_partials['backward'])
        runs.append((out.detach().cpu(), y.grad.cpu(), mod.weight.grad.cpu().clone(), mod.bias.grad.cpu().clone()))
        for part, raw in (fwd, bwd):
            assert part.shape == (n * c, chunks, 2) and raw.shape == (n * c, 2)
            assert np.array_equal(raw, _ordered_sum(part))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)

    # the gates of test_fused_norm.test_fused_norm_act_equals_the_pytorch_composition against the float64 composition
    mod64 = nn.InstanceNorm2d(c, affine=True, track_running_stats=False).double()
    mod64.load_state_dict({k: v.detach().cpu().double() for k, v in bn.state_dict().items()})
    y = y0.clone().double().requires_grad_(True)
    out64 = composed(mod64, y, act, pad, None)
    (out64 * dz.double()).sum().backward()
    o1, gy1, gw1, gb1 = runs[0]
    scale = lambda t: max(1.0, float(t.abs().max()))                      # noqa: E731
    assert float((o1 - out64.detach().float()).abs().max()) <= 2e-5
    assert float((gy1 - y.grad.float()).abs().max()) <= 2e-4 * scale(y.grad)
    assert float((gw1 - mod64.weight.grad.float()).abs().max()) <= 2e-4 * scale(mod64.weight.grad)
    assert float((gb1 - mod64.bias.grad.float()).abs().max()) <= 2e-4 * scale(mod64.bias.grad)


@pytest.mark.parametrize('device', BACKENDS, indirect=True)
def test_the_switch_off_takes_the_atomic_entry(device):
    fused_norm.DETERMINISTIC = False
    eng = ro.engine_for(device)
    eng.norm_partials.clear()
    eng.keep_norm_partials = True
    before = eng.det_scratch_bytes
    bn = nn.InstanceNorm2d(4, affine=True, track_running_stats=False).to(device)
    y = torch.randn(2, 4, 9, 11, device=device, requires_grad=True)
    fused_norm.norm_act(bn, y, 'elu', 1, None).sum().backward()
    assert eng.norm_partials == {} and eng.det_scratch_bytes == before
