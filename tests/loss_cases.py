"""Seeded inputs and a dtype-generic composition of the three training losses, shared by tests/golden/make_golden_loss.py (which runs
the reference's network/loss.py on these inputs), tests/test_loss*.py and tools/time_losses.py.

The composition is written from the definitions (network/loss.py:29-44, 57-77, 91-132; network/ops.py:14-34 and grid_sample's
bilinear / border / align_corners=True rules), not from the kernels: in float64 it is the expected value where the reference cannot
run, in float32 it measures what float32 arithmetic costs (`dev32`) and serves as the eager baseline of the timing tool."""
import hashlib

import numpy as np
import torch

THRESH = 0.02


# ---- the composition ------------------------------------------------------------------------------------------------------------
def render_terms(preds, gt, mask):
    """preds: list of [b, n, 3]; gt [b, n, 3]; mask [b, n] (any dtype) or None -> list of [b]"""
    out = []
    for pr in preds:
        l = torch.sum((pr - gt) ** 2, -1)
        if mask is not None:
            m = mask.float()                         # (float32 whatever the colours' dtype, and so is the denominator: loss.py:63-64)
            out.append(torch.sum(l * m, 1) / (torch.sum(m, 1) + 1e-3))
        else:
            out.append(torch.mean(l, 1))
    return out


def consist_terms(pairs):
    """pairs: list of (p0, p1) [qn, rn, dn] -> list of [qn]"""
    out = []
    for p0, p1 in pairs:
        p0 = p0.detach()
        ce = -p0 * torch.log(p1 + 1e-5) - (1 - p0) * torch.log(1 - p1 + 1e-5)
        out.append(torch.mean(torch.mean(ce, -1), 1))
    return out


def gather_border(maps, coords, use_grid_sample=False):
    """maps [rfn, 1, h, w], coords [rfn, pn, 2] as (x, y) in pixels -> [rfn, pn]: bilinear, border padding, align_corners=True"""
    rfn, _, h, w = maps.shape
    c = coords.to(maps.dtype)
    xn, yn = c[..., 0] / (w - 1) * 2 - 1, c[..., 1] / (h - 1) * 2 - 1
    if use_grid_sample:
        grid = torch.stack([xn, yn], -1).unsqueeze(1)
        return torch.nn.functional.grid_sample(maps, grid, mode='bilinear', padding_mode='border', align_corners=True)[:, 0, 0]
    ix = torch.clamp((xn + 1) / 2 * (w - 1), 0, w - 1)
    iy = torch.clamp((yn + 1) / 2 * (h - 1), 0, h - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = (x0 + 1) - ix, (y0 + 1) - iy
    x0i, y0i = x0.long(), y0.long()
    x1i, y1i = torch.clamp(x0i + 1, max=w - 1), torch.clamp(y0i + 1, max=h - 1)      # (their weights are 0 where clamped)
    flat = maps.reshape(rfn, h * w)
    tap = lambda yi, xi: torch.gather(flat, 1, yi * w + xi)                           # noqa: E731
    return tap(y0i, x0i) * (wx0 * wy0) + tap(y0i, x1i) * (wx1 * wy0) + tap(y1i, x0i) * (wx0 * wy1) + tap(y1i, x1i) * (wx1 * wy1)


def inv_depth(depth, depth_range):
    near, far = -1 / depth_range[:, 0:1], -1 / depth_range[:, 1:2]
    d = -1 / torch.clamp(depth, min=1e-5)
    return torch.clamp((d - near) / (far - near), min=0, max=1.0)


def depth_terms(preds, true_depth, noisy, coords, depth_range, loss_type='l2', beta=0.05, thresh=THRESH, use_grid_sample=False):
    """preds: list of [rfn, pn]; noisy: the gso scene's noisy map or None -> list of [rfn]"""
    gt = inv_depth(gather_border(true_depth, coords, use_grid_sample), depth_range)
    m = None
    if noisy is not None:
        m = (torch.abs(inv_depth(gather_border(noisy, coords, use_grid_sample), depth_range) - gt) < thresh).float()     # (loss.py:123)
    out = []
    for pr in preds:
        x = gt - pr
        if loss_type == 'l2':
            l = x ** 2
        else:
            z = torch.abs(x)
            l = torch.where(z < beta, 0.5 * z * z / beta, z - 0.5 * beta)
        out.append(torch.sum(l * m, 1) / (torch.sum(m, 1) + 1e-4) if m is not None else torch.mean(l, 1))
    return out


# ---- seeded inputs (numpy float32 / int64 / bool) ---------------------------------------------------------------------------------
def render_inputs(seed, b, rn, suffixes=('nr', 'dr', 'dr_fine', 'nr_fine')):
    rng = np.random.RandomState(seed)
    gt = rng.rand(b, rn, 3).astype(np.float32)
    d = {'pixel_colors_gt': gt, 'ray_mask': rng.rand(b, rn) < 0.8}
    for i, s in enumerate(suffixes):
        d['pixel_colors_' + s] = (gt + (0.05 + 0.03 * i) * rng.randn(b, rn, 3)).astype(np.float32)
    return d


def consist_inputs(seed, qn, rn, dn, fine=True):
    """hit probabilities: p0 a sub-stochastic distribution per ray, p1 in (0, 1) with ray 0 exactly 0 and ray 1 exactly 1"""
    rng = np.random.RandomState(seed)
    d = {}
    for sfx in ('', '_fine') if fine else ('',):
        e = rng.rand(qn, rn, dn) ** 4
        d['hit_prob_nr' + sfx] = (e / e.sum(-1, keepdims=True) * rng.rand(qn, rn, 1)).astype(np.float32)
        p1 = (rng.rand(qn, rn, dn) ** 3).astype(np.float32)
        p1[:, 0] = 0.0
        p1[:, 1] = 1.0
        d['hit_prob_self' + sfx] = p1
    d['ray_mask'] = rng.rand(1, rn) < 0.7
    return d


def depth_inputs(seed, rfn, pn, h, w, gso, int_coords, fine=True):
    """true_depth from a normalised inverse depth t in [0.1, 0.9]; the gso noisy map is built in the same domain, t +- {0.25, 4} x
    thresh per pixel, so no point's |aug - gt| lies near the threshold.  int64 coordinates are (row, col) pairs - used as (x, y) by the
    loss, so with h > w the first one runs past w - 1 and the border clamp is hit; float coordinates are random, partly outside."""
    rng = np.random.RandomState(seed)
    rng_ = np.stack([0.5 + 0.5 * rng.rand(rfn), 3.0 + 2.0 * rng.rand(rfn)], -1)
    near, far = -1.0 / rng_[:, 0], -1.0 / rng_[:, 1]

    def to_depth(t):
        return (-1.0 / (t * (far - near)[:, None, None, None] + near[:, None, None, None])).astype(np.float32)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
    f = rng.rand(rfn, 3)[:, :, None, None]
    t = 0.5 + 0.3 * np.sin(2 * np.pi * (f[:, 0] * xx + f[:, 1] * yy) + 6 * f[:, 2]) + 0.1 * (rng.rand(rfn, h, w) - 0.5)
    t = np.clip(t, 0.1, 0.9)[:, None]
    info = {'true_depth': to_depth(t), 'depth_range': rng_.astype(np.float32)}
    if gso:
        step = np.where(rng.rand(rfn, 1, h, w) < 0.7, 0.25, 4.0) * np.where(rng.rand(rfn, 1, h, w) < 0.5, -1.0, 1.0) * THRESH
        info['depth'] = to_depth(t + step)
    if int_coords:
        coords = np.stack([rng.randint(0, h, (rfn, pn)), rng.randint(0, w, (rfn, pn))], -1).astype(np.int64)
        t_at = t[np.arange(rfn)[:, None], 0, coords[..., 1].clip(max=h - 1), coords[..., 0].clip(max=w - 1)]
    else:
        coords = (np.stack([rng.rand(rfn, pn) * (w + 8) - 4, rng.rand(rfn, pn) * (h + 8) - 4], -1)).astype(np.float32)
        ci = np.rint(coords).astype(np.int64)
        t_at = t[np.arange(rfn)[:, None], 0, ci[..., 1].clip(0, h - 1), ci[..., 0].clip(0, w - 1)]
    pr = {}
    for sfx in ('', '_fine') if fine else ('',):
        # [rfn, pn, 2] like the dist decoder's mean read-out: depth_mean is its [..., 0] view
        pr['mean' + sfx] = np.clip(t_at[..., None] + 0.08 * rng.randn(rfn, pn, 2), 0, 1).astype(np.float32)
    return {'coords': coords, 'info': info, 'pr': pr, 'scene_name': 'gso/shoe' if gso else 'dtu_train/scan3'}


def digest(tree):
    """sha256 over every array of a nested dict, in sorted key order"""
    hsh = hashlib.sha256()

    def walk(x):
        if isinstance(x, dict):
            for k in sorted(x):
                hsh.update(k.encode())
                walk(x[k])
        elif isinstance(x, str):
            hsh.update(x.encode())
        else:
            a = np.ascontiguousarray(x)
            hsh.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    walk(tree)
    return hsh.hexdigest()


# ---- data_pr / data_gt as the loss objects take them ----------------------------------------------------------------------------
def as_torch(x, dtype=torch.float32, device='cpu'):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    return t.to(dtype) if t.is_floating_point() else t


def depth_data(case, dtype=torch.float32, device='cpu', float_coords=False):
    """-> (data_pr, data_gt, leaves): depth_mean[_fine] are [..., 0] views of leaf tensors [rfn, pn, 2] that require grad"""
    leaves = {k: as_torch(v, dtype, device).requires_grad_(True) for k, v in case['pr'].items()}
    coords = as_torch(case['coords'], dtype, device)
    if float_coords:
        coords = coords.to(dtype)
    data_pr = {'depth_coords': coords, 'pixel_colors_nr': torch.zeros(1, 4, 3, device=device)}
    for k, v in leaves.items():
        data_pr['depth_' + k] = v[..., 0]
    data_gt = {'ref_imgs_info': {k: as_torch(v, dtype, device) for k, v in case['info'].items()}, 'scene_name': case['scene_name']}
    return data_pr, data_gt, leaves


# the golden's cases: name -> (builder, arguments)
RENDER_CASES = {'render_mask': dict(seed=11, b=2, rn=150), 'render_nomask': dict(seed=12, b=2, rn=150)}
CONSIST_CASES = {'consist': dict(seed=21, qn=2, rn=40, dn=16)}
DEPTH_CASES = {
    'depth_l2_gso_int': dict(seed=31, rfn=4, pn=2100, h=150, w=100, gso=True, int_coords=True),
    'depth_sl1_gso_int': dict(seed=32, rfn=4, pn=600, h=150, w=100, gso=True, int_coords=True),
    'depth_l2_float': dict(seed=33, rfn=4, pn=600, h=150, w=100, gso=False, int_coords=False),
    'depth_sl1_float': dict(seed=34, rfn=4, pn=2100, h=150, w=100, gso=False, int_coords=False),
}
DEPTH_CFG = {'depth_l2_gso_int': 'l2', 'depth_sl1_gso_int': 'smooth_l1', 'depth_l2_float': 'l2', 'depth_sl1_float': 'smooth_l1'}
