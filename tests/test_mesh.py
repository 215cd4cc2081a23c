"""Mesh export (neuray_amd/mesh.py, csrc/nr_kernels_tsdf.h): the TSDF integration kernel against the float64 reference,
exact properties of the integration, the surface-nets kernels against the float32 reference on a shared state, topology on an analytic state,
fuse_mesh end to end against the true surface of procedural scenes, and the public surface (PLY, TSDFVolume, the command line, argument errors).

Cases: test_geometry's 5 views of 40 x 56 of three procedural scenes; the volume has origin (-1.5, -1.5, -1.2), vs = 0.1, dims (29, 26, 23) and
trunc = 0.3: no dimension is a multiple of 64 or 4, partial waves on every axis, more than one workgroup.

Near-threshold (view, lattice point) pairs: u + 0.5 or v + 0.5 within 2e-4 of an integer, |z| < 1e-4, |sdf +- trunc| < 1e-5.  A lattice point
with such a pair is left out of the integration's comparisons; at most 0.5 % of the pairs with z > 0 may be near a threshold (measured:
0.088 .. 0.091 % of 86 710 pairs per scene, 76 .. 79 of the 17 342 lattice points, and outside them the float32 reference differs from the
float64 one in no decision).

Tolerances.  They come from the reference alone: the float32 evaluation against the float64 evaluation of the same formulas on the three
scenes (test_reference_float32_agrees_with_float64 measures and asserts them on the CPU).  Worst values measured: Tsum 2.78e-6, Csum 4.18e-7;
with one shared float32 state, vertices 2.09e-7, normals 1.30e-7, colours 1.16e-7, all absolute.  The gates of the kernel tests are 4 x these.

End to end (test 6), fuse_mesh with filter=True on the 40 x 56 views, vs = 0.1, distance of the vertices to the true surface, median / 95th
percentile.  The float64 reference pipeline: generated7 0.0096 / 0.0497 (385 vertices), generated3 0.0083 / 0.0417 (502), hand 0.0093 / 0.0572
(329); the emulator and the MI355X gave the same vertex counts and the same values to the digits shown.  On the MI355X the kernels gave the
float32 reference's numbers in every case of tests 2 and 4 (worst Tsum 2.77e-6, Csum 4.17e-7, vertices 2.09e-7, normals 1.30e-7, colours 1.15e-7)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from test_geometry import BACKENDS, H, N, SCENES, W, cameras, engine_for, scene, views
from neuray_amd import geometry as geo, mesh
from neuray_amd.engine import RenderEngine

ORIGIN, VS, DIMS, TRUNC = (-1.5, -1.5, -1.2), 0.1, (29, 26, 23), 0.3
NX, NY, NZ = DIMS
MAX_LEFT_OUT = 0.005
REF_TSUM_ERR, REF_CSUM_ERR, REF_VERTEX_ERR, REF_NORMAL_ERR, REF_COLOUR_ERR = 2.78e-6, 4.18e-7, 2.09e-7, 1.30e-7, 1.16e-7    # float32 reference against float64 reference
TOL_TSUM, TOL_VERTEX, TOL_NORMAL, TOL_COLOUR = 4 * REF_TSUM_ERR, 4 * REF_VERTEX_ERR, 4 * REF_NORMAL_ERR, 4 * REF_COLOUR_ERR
TOL_CSUM = 4 * REF_CSUM_ERR
STATE_KEYS = ('tsum', 'w', 'csum', 'cw')


def frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(None)
def reference(name, dtype='float64'):
    """the five views integrated by the reference, computed once and read-only (float64: with the per-pair details)"""
    poses, Ks = cameras()
    depth, rgb = views(name)
    return frozen(mesh.integrate_numpy(depth, rgb, poses, Ks, ORIGIN, VS, DIMS, TRUNC, dtype=np.dtype(dtype), details=dtype == 'float64'))


def near_threshold(ref):
    """[nz,ny,nx] bool: lattice points with a near-threshold pair, and the share of the pairs with z > 0 that are near a threshold"""
    def near_int(a):
        return np.abs(a + 0.5 - np.round(a + 0.5)) < 2e-4
    with np.errstate(invalid='ignore'):
        front = ref['z'] > 0
        near = near_int(ref['u']) | near_int(ref['v']) | (np.abs(ref['z']) < 1e-4)
        near |= (np.abs(ref['sdf'] - TRUNC) < 1e-5) | (np.abs(ref['sdf'] + TRUNC) < 1e-5)
    return (near & (ref['z'] > -1e-4)).any(0), (near & front).sum() / max(front.sum(), 1), int(front.sum())


def compare_state(got, ref, what):
    """the gates of test 2 on one scene -> (worst Tsum error, worst Csum error); got: dict of numpy arrays"""
    near, left_out, pairs = near_threshold(ref)
    assert left_out <= MAX_LEFT_OUT, (what, left_out)
    keep = ~near
    assert np.array_equal(got['w'][keep], ref['w'][keep]) and np.array_equal(got['cw'][keep], ref['cw'][keep]), what
    assert all(np.all(np.isfinite(got[k])) for k in STATE_KEYS), what
    e_t = float(np.abs(got['tsum'] - ref['tsum'])[keep].max())
    e_c = float(np.abs(got['csum'] - ref['csum'])[:, keep].max())
    print('%s: near a threshold %.3f %% of %d pairs, %d of %d lattice points left out, Tsum %.2e, Csum %.2e'
          % (what, 100 * left_out, pairs, near.sum(), near.size, e_t, e_c))
    return e_t, e_c


def device_state(eng, state=None, colour=True):
    state = mesh.zero_state(DIMS, colour) if state is None else state
    return {k: torch.from_numpy(np.array(state[k], np.float32)).to(eng.device) for k in (STATE_KEYS if colour else STATE_KEYS[:2])}


def host_state(state):
    return {k: v.cpu().numpy() for k, v in state.items()}


def integrate(eng, name, ranges=((0, N),), colour=True, depth=None):
    poses, Ks = cameras()
    d, rgb = views(name)
    d = d if depth is None else depth
    state = device_state(eng, colour=colour)
    for r in ranges:
        eng.tsdf_integrate(state, ORIGIN, VS, TRUNC, DIMS, d, rgb, poses, Ks, r)
    return host_state(state)


@functools.lru_cache(None)
def kernel_state(backend, name):
    return frozen(integrate(engine_for(backend), name))


def extract(eng, state, min_weight=1.0):
    """the two extraction kernels on a host state -> dict of numpy arrays with the cell bytes"""
    dev = device_state(eng, state, colour='csum' in state)
    cells = eng.surface_cells(dev, DIMS, min_weight)
    out = {k: v.cpu().numpy() for k, v in eng.surface_emit(dev, ORIGIN, VS, DIMS, cells).items()}
    out['cells'] = cells.cpu().numpy()
    return out


# ---- 1. the reference against itself: where the tolerances come from -----------------------------------------------------------------
def test_reference_float32_agrees_with_float64():
    worst = {'tsum': 0.0, 'csum': 0.0, 'vertices': 0.0, 'normals': 0.0, 'colors': 0.0}
    for name in SCENES:
        ref, f32 = reference(name), reference(name, 'float32')
        assert f32['tsum'].dtype == np.float32
        e_t, e_c = compare_state(f32, ref, 'float32 reference %s' % name)
        worst['tsum'], worst['csum'] = max(worst['tsum'], e_t), max(worst['csum'], e_c)
        assert (ref['w'] > 0).mean() > 0.3 and (ref['tsum'] < 0).sum() > 200 and 0 < (ref['cw'] < ref['w']).sum()
        # one shared float32 state, extracted in both precisions: the same cells and faces, and the error of the float32 arithmetic
        a = mesh.surface_nets_numpy(f32['tsum'], f32['w'], f32['csum'], f32['cw'], ORIGIN, VS)
        b = mesh.surface_nets_numpy(f32['tsum'], f32['w'], f32['csum'], f32['cw'], ORIGIN, VS, dtype=np.float32)
        assert np.array_equal(a['cells'], b['cells']) and np.array_equal(a['faces'], b['faces']) and a['vertices'].shape[0] > 300
        for k in ('vertices', 'normals', 'colors'):
            assert b[k].dtype == np.float32
            worst[k] = max(worst[k], float(np.abs(a[k] - b[k]).max()))
    print('worst: Tsum %.3e, Csum %.3e, vertices %.3e, normals %.3e, colours %.3e' % tuple(worst[k] for k in ('tsum', 'csum', 'vertices', 'normals', 'colors')))
    # the gates are 4 x what was measured when they were written down; the measurement still holds
    assert worst['tsum'] <= REF_TSUM_ERR * 1.0001 and worst['csum'] <= REF_CSUM_ERR * 1.0001
    assert worst['vertices'] <= REF_VERTEX_ERR * 1.0001 and worst['normals'] <= REF_NORMAL_ERR * 1.0001 and worst['colors'] <= REF_COLOUR_ERR * 1.0001


# ---- 2. the integration kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', SCENES)
def test_integration_kernel_matches_the_float64_reference(name, backend):
    got = kernel_state(backend, name)
    assert got['tsum'].shape == (NZ, NY, NX) and got['csum'].shape == (3, NZ, NY, NX)
    e_t, e_c = compare_state(got, reference(name), 'kernel [%s] %s' % (backend, name))
    assert e_t <= TOL_TSUM and e_c <= TOL_CSUM


# ---- 3. exact properties of the integration --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_integration_is_exact_in_its_order_and_its_skips(backend):
    eng = engine_for(backend)
    whole = kernel_state(backend, 'generated7')
    split = integrate(eng, 'generated7', ((0, 2), (2, N)))
    again = integrate(eng, 'generated7')
    for k in STATE_KEYS:
        assert split[k].tobytes() == whole[k].tobytes(), k                # [0, 5) = [0, 2) then [2, 5), bit for bit
        assert again[k].tobytes() == whole[k].tobytes(), k                # two runs
    # a view whose depth map is all zero changes no bit: views 0, 1, 3, 4 with view 2 emptied = the same views without it
    depth = views('generated7')[0].copy()
    depth[2] = 0
    emptied = integrate(eng, 'generated7', depth=depth)
    without = integrate(eng, 'generated7', ((0, 2), (3, N)))
    for k in STATE_KEYS:
        assert emptied[k].tobytes() == without[k].tobytes(), k
    assert emptied['w'].sum() < whole['w'].sum()
    # no colour pointers: Tsum and W as before
    plain = integrate(eng, 'generated7', colour=False)
    assert set(plain) == {'tsum', 'w'} and plain['tsum'].tobytes() == whole['tsum'].tobytes() and plain['w'].tobytes() == whole['w'].tobytes()
    # an empty range is accepted and does nothing
    assert integrate(eng, 'generated7', ((3, 3),))['w'].sum() == 0


# ---- 4. the extraction, given the float32 reference's state ----------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', SCENES)
def test_extraction_kernels_match_the_reference_on_a_shared_state(name, backend):
    f32 = reference(name, 'float32')
    state = {k: f32[k] for k in STATE_KEYS}
    want = mesh.surface_nets_numpy(state['tsum'], state['w'], state['csum'], state['cw'], ORIGIN, VS, dtype=np.float32)
    want64 = mesh.surface_nets_numpy(state['tsum'], state['w'], state['csum'], state['cw'], ORIGIN, VS)
    got = extract(engine_for(backend), state)
    assert got['cells'].shape == (NZ - 1, NY - 1, NX - 1) and np.array_equal(got['cells'], want['cells'])
    assert got['vertices'].shape == want['vertices'].shape and got['vertices'].shape[0] > 300 and got['faces'].dtype == np.int32
    assert np.array_equal(got['faces'], want['faces']) and got['faces'].shape[0] > 500
    errs = {k: float(np.abs(got[k] - want64[k]).max()) for k in ('vertices', 'normals', 'colors')}
    print('extraction [%s] %s: %d vertices, %d faces, vertices %.2e, normals %.2e, colours %.2e'
          % (backend, name, got['vertices'].shape[0], got['faces'].shape[0], errs['vertices'], errs['normals'], errs['colors']))
    assert errs['vertices'] <= TOL_VERTEX and errs['normals'] <= TOL_NORMAL and errs['colors'] <= TOL_COLOUR
    assert all(np.abs(got[k] - want[k]).max() <= tol for k, tol in (('vertices', TOL_VERTEX), ('normals', TOL_NORMAL), ('colors', TOL_COLOUR)))
    # without colour state: grey, everything else the same bytes
    grey = extract(engine_for(backend), {k: state[k] for k in ('tsum', 'w')})
    assert np.all(grey['colors'] == 0.5) and all(grey[k].tobytes() == got[k].tobytes() for k in ('cells', 'vertices', 'normals', 'faces'))


# ---- 5. topology on an analytic state ---------------------------------------------------------------------------------------------------
CENTRE, RADIUS = (13.3, 12.1, 10.7), 8.4          # in voxels from the origin


def sphere_state(hole=False):
    iz, iy, ix = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing='ij')
    dist = np.sqrt((ix - CENTRE[0]) ** 2 + (iy - CENTRE[1]) ** 2 + (iz - CENTRE[2]) ** 2) - RADIUS
    w = np.ones(dist.shape, np.float32)
    if hole:                                               # nothing observed in the octant x >= 14, y >= 13, z >= 11
        w[11:, 13:, 14:] = 0
    return {'tsum': (dist * VS).astype(np.float32) * w, 'w': w}


def edge_counts(faces):
    f = faces.astype(np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    m = int(f.max()) + 1
    d_keys, d_counts = np.unique(directed[:, 0] * m + directed[:, 1], return_counts=True)
    u = np.sort(directed, 1)
    u_keys, u_counts = np.unique(u[:, 0] * m + u[:, 1], return_counts=True)
    return d_counts, u_keys, u_counts, m


@pytest.mark.parametrize('backend', ['numpy'] + BACKENDS)
def test_topology_of_a_sphere_and_of_a_sphere_with_an_unobserved_octant(backend):
    def run(state):
        if backend == 'numpy':
            return mesh.surface_nets_numpy(state['tsum'], state['w'], None, None, ORIGIN, VS, dtype=np.float32)
        return extract(engine_for(backend), state)
    got = run(sphere_state())
    V, F = got['vertices'].shape[0], got['faces'].shape[0]
    assert (V, F) == (1342, 2 * 1340)                      # (the prototype's counts)
    d_counts, _, u_counts, _ = edge_counts(got['faces'])
    assert np.all(u_counts == 2) and np.all(d_counts == 1)           # closed and consistently oriented
    assert V - u_counts.shape[0] + F == 2
    tri = got['vertices'].astype(np.float64)[got['faces']]
    assert np.einsum('ij,ij->i', tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6 > 0.9 * 4 / 3 * np.pi * (RADIUS * VS) ** 3
    centre = np.array(ORIGIN) + np.array(CENTRE) * VS
    radial = got['vertices'].astype(np.float64) - centre
    assert np.all(np.abs(np.linalg.norm(radial, axis=1) - RADIUS * VS) <= np.sqrt(3) * VS)
    nrm = got['normals'].astype(np.float64)
    length = np.linalg.norm(nrm, axis=1)
    assert np.all((length == 0) | (np.abs(length - 1) < 1e-5)) and (length > 0).mean() > 0.99
    assert np.all(np.einsum('ij,ij->i', nrm, radial)[length > 0] > 0)
    assert np.all(got['colors'] == 0.5)
    # W = 0 in one octant: no face names a cell with a corner in it, and the open edges are exactly those on its border
    holed = run(sphere_state(hole=True))
    cells = holed['cells']
    touching = np.zeros(cells.shape, bool)
    touching[10:, 12:, 13:] = True                         # cells with a corner in the octant
    assert not np.any(cells[touching]) and np.array_equal(cells[~touching] & 1, got['cells'][~touching] & 1)
    cell_of_vertex = np.flatnonzero(cells.reshape(-1) & 1)
    assert holed['vertices'].shape[0] == cell_of_vertex.shape[0] and holed['faces'].max() < cell_of_vertex.shape[0]
    assert 0 < holed['faces'].shape[0] < F
    d_counts, u_keys, u_counts, m = edge_counts(holed['faces'])
    assert np.all(d_counts == 1) and np.all(u_counts <= 2)
    open_edges = u_keys[u_counts == 1]
    assert open_edges.shape[0] > 0 and mesh.boundary_edges(holed['faces']) == open_edges.shape[0] and mesh.boundary_edges(got['faces']) == 0
    # a border vertex: its cell is next to a cell that touches the octant (in the 26-neighbourhood)
    grown = np.zeros(cells.shape, bool)
    grown[9:, 11:, 12:] = True
    on_border = (grown & ~touching).reshape(-1)[cell_of_vertex]
    assert np.all(on_border[open_edges // m]) and np.all(on_border[open_edges % m])
    # ... and every quad of the full sphere that is missing has a cell in the touched region: away from it nothing changed
    keep_faces = ~np.isin(np.flatnonzero(got['cells'].reshape(-1) & 1)[got['faces']], np.flatnonzero(touching.reshape(-1))).any(1)
    full_cells = np.flatnonzero(got['cells'].reshape(-1) & 1)[got['faces'][keep_faces]]
    assert np.array_equal(full_cells, cell_of_vertex[holed['faces']])


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def reference_pipeline(name):
    """filter_depth's float64 twin, then integrate_numpy + surface_nets_numpy in float64 on the same volume as fuse_mesh chooses"""
    poses, Ks = cameras()
    depth, rgb = views(name)
    nn = geo.nearest_sources(poses, 8)
    cons = geo.consistency_numpy(depth, poses, Ks, nn, 1.0, 0.01)
    filtered = np.where(cons['count'] >= 2, cons['fused_depth'], 0.0).astype(np.float32)
    lo, hi = mesh.depth_bounds(filtered, poses, Ks)
    return filtered, lo, hi


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', SCENES)
def test_fuse_mesh_lies_on_the_true_surface(name, backend):
    poses, Ks = cameras()
    depth, rgb = views(name)
    out = mesh.fuse_mesh(depth, rgb, poses, Ks, voxel_size=VS, engine=engine_for(backend))
    vol = out['volume']
    assert vol.trunc == pytest.approx(3 * VS) and all(torch.is_tensor(out[k]) for k in ('vertices', 'faces', 'colors', 'normals'))
    filtered, lo, hi = reference_pipeline(name)
    assert np.allclose(vol.origin, lo - 3 * VS, atol=1e-4)             # the box of the filtered depths, padded by trunc
    assert all(vol.origin[k] + (vol.dims[k] - 1) * VS >= hi[k] + 3 * VS - 1e-4 for k in range(3))
    st = mesh.integrate_numpy(filtered, rgb, poses, Ks, vol.origin, VS, vol.dims, vol.trunc)
    ref = mesh.surface_nets_numpy(st['tsum'], st['w'], st['csum'], st['cw'], vol.origin, VS)
    d_got = geo.surface_distance(scene(name), out['vertices'])
    d_ref = geo.surface_distance(scene(name), ref['vertices'])
    stats = [float(np.median(d_got)), float(np.percentile(d_got, 95)), float(np.median(d_ref)), float(np.percentile(d_ref, 95))]
    print('fuse_mesh [%s] %s: %d vertices (reference %d), %d faces, surface distance median %.4f p95 %.4f (reference %.4f / %.4f)'
          % (backend, name, d_got.shape[0], d_ref.shape[0], out['faces'].shape[0], *stats))
    assert d_got.shape[0] > 300 and out['faces'].shape[0] > 400 and int(out['faces'].max()) < d_got.shape[0]
    assert stats[0] < VS and stats[0] <= 1.1 * stats[2] and stats[1] <= 1.1 * stats[3]
    col = out['colors'].cpu().numpy()
    assert np.all((col >= 0) & (col <= 1)) and col.std() > 0.01


# ---- 7. the public surface ---------------------------------------------------------------------------------------------------------------
def test_mesh_ply_round_trip(tmp_path):
    rng = np.random.RandomState(0)
    pts, nrm, col = rng.randn(37, 3).astype(np.float32), rng.randn(37, 3).astype(np.float32), rng.rand(37, 3).astype(np.float32)
    faces = rng.randint(0, 37, (51, 3)).astype(np.int32)
    path = str(tmp_path / 'mesh.ply')
    mesh.write_mesh_ply(path, torch.from_numpy(pts), torch.from_numpy(faces), col, nrm)
    head = open(path, 'rb').read(500).decode('ascii', 'replace')
    assert head.startswith('ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\n')
    assert 'property uchar blue\nelement face 51\nproperty list uchar int vertex_indices\nend_header\n' in head
    assert os.path.getsize(path) == head.index('end_header\n') + len('end_header\n') + 37 * 27 + 51 * 13
    back = mesh.read_mesh_ply(path)
    assert back['vertices'].tobytes() == pts.tobytes() and back['normals'].tobytes() == nrm.tobytes() and np.array_equal(back['faces'], faces)
    assert back['faces'].dtype == np.int32 and np.array_equal(back['colors'], np.clip(col * 255, 0, 255).astype(np.uint8))
    mesh.write_mesh_ply(path, pts[:0], faces[:0])
    assert mesh.read_mesh_ply(path)['faces'].shape == (0, 3) and mesh.read_mesh_ply(path)['vertices'].shape == (0, 3)
    with pytest.raises(ValueError, match='names vertex'):
        mesh.write_mesh_ply(path, pts, np.array([[0, 1, 37]]))
    geo.write_ply(path, pts)                               # a point cloud is not a mesh
    with pytest.raises(ValueError):
        mesh.read_mesh_ply(path)


@pytest.mark.parametrize('backend', BACKENDS)
def test_tsdf_volume_on_numpy_and_on_the_device_agree(backend):
    poses, Ks = cameras()
    depth, rgb = views('hand')
    eng = engine_for(backend)
    dev = mesh.TSDFVolume(ORIGIN, VS, DIMS, engine=eng)
    assert dev.trunc == pytest.approx(TRUNC) and dev.integrate(depth, rgb, poses, Ks, (0, 3)).integrate(depth, rgb, poses, Ks, (3, N)) is dev
    assert all(torch.is_tensor(v) and v.device == eng.device for v in dev.state().values())
    e_t, e_c = compare_state(host_state(dev.state()), reference('hand'), 'TSDFVolume [%s]' % backend)
    assert e_t <= TOL_TSUM and e_c <= TOL_CSUM
    f = dev.tsdf().cpu().numpy()
    assert np.array_equal(np.isnan(f), reference('hand')['w'] == 0) and np.nanmax(f) <= 1 and np.nanmin(f) >= -1
    if not torch.cuda.is_available():                      # the path without a device: the float32 reference
        host = mesh.TSDFVolume(ORIGIN, VS, DIMS).integrate(depth, rgb, poses, Ks)
        assert host.engine is None and all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in host.state().values())
        compare_state(host.state(), reference('hand'), 'TSDFVolume numpy')
        assert np.array_equal(np.isnan(host.tsdf()), np.isnan(f))
        # extraction of one state on both: the rules of test 4
        a = host.extract()
        b = {k: v.cpu().numpy() for k, v in mesh.TSDFVolume(ORIGIN, VS, DIMS, engine=eng).integrate(depth, rgb, poses, Ks).extract().items()}
        assert set(a) == set(b) == {'vertices', 'faces', 'colors', 'normals'}
        if all(np.array_equal(host.state()[k], kernel_state(backend, 'hand')[k]) for k in STATE_KEYS):
            assert np.array_equal(a['faces'], b['faces'])
            assert np.abs(a['vertices'] - b['vertices']).max() <= TOL_VERTEX and np.abs(a['normals'] - b['normals']).max() <= TOL_NORMAL
            assert np.abs(a['colors'] - b['colors']).max() <= TOL_COLOUR
    grey = mesh.TSDFVolume(ORIGIN, VS, DIMS, colour=False, engine=eng).integrate(depth, None, poses, Ks)
    assert set(grey.state()) == {'tsum', 'w'} and torch.equal(grey.state()['tsum'], dev.state()['tsum'])
    assert bool((grey.extract(min_weight=2)['colors'] == 0.5).all()) and grey.extract(min_weight=2)['vertices'].shape[0] < dev.extract()['vertices'].shape[0]


def test_command_line_exports_a_procedural_database(tmp_path, capsys):
    from neuray_amd import export_mesh
    out, js = str(tmp_path / 'mesh.ply'), str(tmp_path / 'mesh.json')
    res = export_mesh.main(['--database', 'procedural/5/white_40', '--depth', 'database', '--voxel', '0.08', '--out', out, '--json', js])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.load(open(js)) and line['vertices'] == res['vertices'] and line['views'] == 48 and (line['h'], line['w']) == (40, 40)
    got = mesh.read_mesh_ply(out)
    assert got['vertices'].shape == (res['vertices'], 3) and got['faces'].shape == (res['faces'], 3) and res['vertices'] > 500 and res['faces'] > 1000
    assert res['boundary_edges'] == mesh.boundary_edges(got['faces']) and res['voxel_size'] == 0.08
    assert res['surface_distance']['median'] < 0.08 and res['surface_distance']['p95'] < 2 * 0.08
    dist = geo.surface_distance(scene_of(5), got['vertices'])
    assert abs(float(np.median(dist)) - res['surface_distance']['median']) < 1e-6
    with pytest.raises(SystemExit):
        export_mesh.main(['--depth', 'database', '--out', out])
    with pytest.raises(SystemExit):
        export_mesh.main(['--database', 'procedural/5/white_40', '--voxel', '0', '--out', out])


def scene_of(seed):
    from neuray_amd import procedural as proc
    return proc.make_scene(seed, 'white')


@pytest.mark.parametrize('backend', BACKENDS)
def test_the_entry_points_check_their_arguments(backend):
    import ctypes as C
    from neuray_amd import _lib
    eng = engine_for(backend)
    poses, Ks = cameras()
    depth, rgb = views('hand')

    def state(dims, colour=True):
        return {k: torch.from_numpy(v).to(eng.device) for k, v in mesh.zero_state(dims, colour).items()}
    for dims in ((1, 26, 23), (29, 0, 23), (29, 26, 1)):
        with pytest.raises(RuntimeError, match='bad dims'):
            eng.tsdf_integrate(state(dims), ORIGIN, VS, TRUNC, dims, depth, rgb, poses, Ks)
        with pytest.raises(RuntimeError, match='bad dims'):
            eng.surface_cells(state(dims), dims)
        with pytest.raises(ValueError):
            mesh.TSDFVolume(ORIGIN, VS, dims, engine=eng)
    for kw in ({'trunc': 0.0}, {'trunc': -1.0}, {'trunc': float('nan')}, {'voxel_size': 0.0}):
        args = {'voxel_size': VS, 'trunc': TRUNC, **kw}
        with pytest.raises(RuntimeError, match='must be positive'):
            eng.tsdf_integrate(state(DIMS), ORIGIN, args['voxel_size'], args['trunc'], DIMS, depth, rgb, poses, Ks)
        with pytest.raises(ValueError):
            mesh.integrate_numpy(depth, rgb, poses, Ks, ORIGIN, args['voxel_size'], DIMS, args['trunc'])
    with pytest.raises(ValueError):
        mesh.TSDFVolume(ORIGIN, VS, DIMS, trunc=0.0, engine=eng)
    # more than 2^30 lattice points: refused before anything is read (the pointers are null)
    for name, cls in (('neuray_tsdf_integrate', _lib.NeurayTsdfIntegrateArgs), ('neuray_surface_cells', _lib.NeuraySurfaceCellsArgs),
                      ('neuray_surface_emit', _lib.NeuraySurfaceEmitArgs)):
        with pytest.raises(RuntimeError, match='2\\^30'):
            eng._check(getattr(eng.lib, name)(C.byref(cls(nx=1025, ny=1024, nz=1024)), eng._stream()))
        with pytest.raises(RuntimeError, match='null args'):
            eng._check(getattr(eng.lib, name)(None, eng._stream()))
        with pytest.raises(RuntimeError, match='missing'):
            kw = {'neuray_tsdf_integrate': dict(n=N, h=H, w=W, v1=N, voxel_size=VS, trunc=TRUNC), 'neuray_surface_cells': dict(min_weight=1.0),
                  'neuray_surface_emit': dict(voxel_size=VS, n_vertices=1)}[name]
            eng._check(getattr(eng.lib, name)(C.byref(cls(nx=NX, ny=NY, nz=NZ, **kw)), eng._stream()))
    with pytest.raises(ValueError, match='2\\^30'):
        mesh.TSDFVolume(ORIGIN, VS, (1025, 1024, 1024), engine=eng)
    for r in ((-1, 2), (0, N + 1), (3, 2)):
        with pytest.raises(RuntimeError, match='views'):
            eng.tsdf_integrate(state(DIMS), ORIGIN, VS, TRUNC, DIMS, depth, rgb, poses, Ks, r)
        with pytest.raises(ValueError):
            mesh.integrate_numpy(depth, rgb, poses, Ks, ORIGIN, VS, DIMS, TRUNC, views=r)
    # mismatched shapes
    with pytest.raises(AssertionError):
        eng.tsdf_integrate(state(DIMS), ORIGIN, VS, TRUNC, DIMS, depth[:4], rgb, poses, Ks)
    with pytest.raises(AssertionError):
        eng.tsdf_integrate(state(DIMS), ORIGIN, VS, TRUNC, DIMS, depth, rgb[:, :, :-1], poses, Ks)
    with pytest.raises(AssertionError):
        eng.tsdf_integrate(state((28, 26, 23)), ORIGIN, VS, TRUNC, DIMS, depth, rgb, poses, Ks)
    with pytest.raises(AssertionError):
        eng.surface_emit(state(DIMS), ORIGIN, VS, DIMS, torch.zeros(NZ, NY, NX, dtype=torch.uint8, device=eng.device))
    with pytest.raises(ValueError):
        mesh.integrate_numpy(depth, rgb[:, :, :-1], poses, Ks, ORIGIN, VS, DIMS, TRUNC)
    with pytest.raises(ValueError):
        mesh.integrate_numpy(depth, rgb, poses[:4], Ks, ORIGIN, VS, DIMS, TRUNC)
    with pytest.raises(RuntimeError, match='go together'):
        a = _lib.NeurayTsdfIntegrateArgs(nx=NX, ny=NY, nz=NZ, n=N, h=H, w=W, v1=N, voxel_size=VS, trunc=TRUNC)
        s = state(DIMS)
        a.depth_dev = a.poses_dev = a.Ks_dev = a.tsum_dev = a.w_dev = a.csum_dev = s['tsum'].data_ptr()       # (refused before anything is read)
        eng._check(eng.lib.neuray_tsdf_integrate(C.byref(a), eng._stream()))
    for mw in (0.0, -1.0, float('nan')):
        with pytest.raises(RuntimeError, match='min_weight'):
            eng.surface_cells(state(DIMS), DIMS, mw)
        with pytest.raises(ValueError):
            mesh.cells_numpy(np.zeros((NZ, NY, NX)), np.zeros((NZ, NY, NX)), mw)
    with pytest.raises(ValueError):
        mesh.fuse_mesh(np.zeros_like(depth), rgb, poses, Ks, filter=False, engine=eng)                        # nothing to bound the volume with
    # an empty volume extracts an empty mesh
    empty = mesh.TSDFVolume(ORIGIN, VS, DIMS, engine=eng).extract()
    assert empty['vertices'].shape == (0, 3) and empty['faces'].shape == (0, 3)
    # a bf16 variant: the engine refuses, and so does the library
    if backend == 'emu':
        from emu_util import emu_lib_bf16
        bf = RenderEngine('cpu', _test_lib=emu_lib_bf16(), variant='bf16')
        assert bf.variant != 'fp32'
        with pytest.raises(NotImplementedError):
            bf.tsdf_integrate(state(DIMS), ORIGIN, VS, TRUNC, DIMS, depth, rgb, poses, Ks)
        with pytest.raises(NotImplementedError):
            bf.surface_cells(state(DIMS), DIMS)
        with pytest.raises(NotImplementedError):
            mesh.TSDFVolume(ORIGIN, VS, DIMS, engine=bf)
        for name, cls in (('neuray_tsdf_integrate', _lib.NeurayTsdfIntegrateArgs), ('neuray_surface_cells', _lib.NeuraySurfaceCellsArgs),
                          ('neuray_surface_emit', _lib.NeuraySurfaceEmitArgs)):
            with pytest.raises(RuntimeError, match='fp32 library'):
                bf._check(getattr(bf.lib, name)(C.byref(cls()), bf._stream()))
