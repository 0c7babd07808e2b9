"""The TSDF mesher's definitions on the host (no GPU): tests/tsdf_restated.py on the exact distance field of a sphere -- topology,
orientation, the radial error bound -- TsdfVolume.from_dense / to_dense, the mesh PLY, the wrappers' argument checks on the `meta`
device and the driver's option rules."""
import os

import numpy as np
import pytest
import torch

import tsdf_restated as R
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import mesh_fusion
from atvsnet_amd.tools import ply

H, RADIUS, CENTRE = 1.0, 10.3, np.array([15.7, 16.2, 15.1])


@pytest.fixture(scope='module')
def field():
    return R.sphere_field(32, H, RADIUS, tuple(CENTRE))


@pytest.fixture(scope='module')
def sphere(field):
    vol = ops.TsdfVolume.from_dense(field, np.ones_like(field), None, (0.0, 0.0, 0.0), H, 4.0 * H)
    return R.mesh(*vol.to_dense(), vol.origin, vol.voxel, with_edges=True)


def test_the_three_voxel_centres_on_the_sphere(field):
    # (5.5, 16.5, 16.5): 10.2^2 + 0.3^2 + 1.4^2 = 10.3^2
    assert field[16, 16, 5] == 0.0 and (field == 0.0).sum() >= 3


def test_the_sphere_is_closed_and_consistently_oriented(sphere):
    v, c, f, _ = sphere
    assert c is None and v.dtype == np.float32 and f.dtype == np.int32
    directed, undirected = R.edge_stats(f)
    assert (len(v), len(f)) == (5946, 11888)
    assert len(v) - len(undirected) + len(f) == 2
    assert all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())
    assert sorted(set(f.reshape(-1).tolist())) == list(range(len(v)))          # no unreferenced vertex
    assert (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all()              # the smallest index first


def test_the_sphere_lies_within_the_derived_bound_and_is_inscribed(sphere):
    v, _, f, _ = sphere
    v = v.astype(np.float64)
    radial = np.linalg.norm(v - CENTRE, axis=1) - RADIUS
    # linear interpolation of a field that is convex along an edge of length <= sqrt(3) h
    assert np.abs(radial).max() <= 3.0 * H * H / (8.0 * (RADIUS - np.sqrt(3.0) * H)) + 1e-5
    assert radial.max() <= 1e-5
    volume = np.einsum('ij,ij->i', v[f[:, 0]] - CENTRE, np.cross(v[f[:, 1]] - CENTRE, v[f[:, 2]] - CENTRE)).sum() / 6.0
    assert 0.0 < volume <= 4.0 / 3.0 * np.pi * RADIUS ** 3
    assert volume > 0.99 * 4.0 / 3.0 * np.pi * RADIUS ** 3


def test_zero_area_faces_are_kept_and_all_edge_types_occur(sphere):
    v, _, f, edges = sphere
    v = v.astype(np.float64)
    area = np.abs(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])).max(axis=1)
    assert (area == 0.0).sum() >= 1
    assert sorted({kind for _, kind in edges}) == list(range(7))
    # ordered by owning voxel (blocks ascending, x fastest), then edge type
    keys = [(R._order_key(a, 4, 4), kind) for a, kind in edges]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_a_box_that_clips_the_sphere_leaves_an_open_surface_with_its_boundary_on_the_clip(field):
    weight = np.ones_like(field)
    weight[:, :, 20:] = 0                                # voxels x >= 20 are not valid: the cubes at x = 19 are not meshed
    v, _, f = R.mesh(field, weight, None, (0.0, 0.0, 0.0), H)
    directed, undirected = R.edge_stats(f)
    assert max(undirected.values()) <= 2 and max(directed.values()) == 1
    boundary = [e for e, n in undirected.items() if n == 1]
    assert len(boundary) > 20
    # every boundary edge lies in the face between a meshed cube and one with an invalid corner: the plane of the voxels x = 19
    assert all(v[a, 0] == np.float32(19.5) and v[b, 0] == np.float32(19.5) for a, b in boundary)
    assert v[:, 0].max() == np.float32(19.5)
    assert sorted(set(f.reshape(-1).tolist())) == list(range(len(v)))


def test_min_weight_above_every_weight_gives_empty_arrays(field):
    v, c, f = R.mesh(field, np.ones_like(field), np.zeros(field.shape + (3,), np.float32), (0.0, 0.0, 0.0), H, min_weight=2.0)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    empty = ops.TsdfVolume.from_dense(field, np.zeros_like(field), None, (0.0, 0.0, 0.0), H, 4.0)
    assert empty.num_blocks == 0 and tuple(empty.tsdf.shape) == (0, 8, 8, 8)


def test_from_dense_to_dense_round_trip():
    rng = np.random.RandomState(3)
    f = rng.uniform(-1, 1, (11, 17, 9)).astype(np.float32)
    w = (rng.uniform(0, 1, f.shape) > 0.5).astype(np.float32) * rng.randint(1, 4, f.shape)
    w[:, 8:16, :] = 0                                    # a whole layer of blocks without weight: absent
    c = rng.uniform(0, 255, f.shape + (3,)).astype(np.float32)
    vol = ops.TsdfVolume.from_dense(f, w, c, (1.5, -2.0, 0.25), 0.1, 0.4)
    assert vol.dims == (2, 3, 2) and vol.voxel == 0.1 and vol.trunc == 0.4 and vol.origin.tolist() == [1.5, -2.0, 0.25]
    blocks = vol.blocks.numpy()
    assert 0 < vol.num_blocks < 12 and not (blocks[:, 1] == 1).any()
    lin = (blocks[:, 2] * 3 + blocks[:, 1]) * 2 + blocks[:, 0]
    assert (np.diff(lin) > 0).all()
    assert bool((vol.weight.reshape(vol.num_blocks, -1) > 0).any(dim=1).all())
    fd, wd, cd = vol.to_dense()
    assert fd.shape == (16, 24, 16) and cd.shape == (16, 24, 16, 3)
    present = np.zeros((16, 24, 16), bool)
    for x, y, z in blocks:
        present[z * 8:z * 8 + 8, y * 8:y * 8 + 8, x * 8:x * 8 + 8] = True
    sub = (slice(0, 11), slice(0, 17), slice(0, 9))
    assert np.array_equal(wd[sub], w) and wd.sum() == w.sum()
    assert np.array_equal(fd[sub][present[sub]], f[present[sub]]) and np.array_equal(cd[sub][present[sub]], c[present[sub]])
    assert not fd[~present].any() and not wd[~present].any()
    # voxel [z][y][x] of a block
    x, y, z = blocks[0]
    assert vol.tsdf[0, 1, 2, 3] == fd[z * 8 + 1, y * 8 + 2, x * 8 + 3]
    again = ops.TsdfVolume.from_dense(fd, wd, cd, vol.origin, vol.voxel, vol.trunc)
    assert torch.equal(again.blocks, vol.blocks) and torch.equal(again.tsdf, vol.tsdf) and torch.equal(again.color, vol.color)
    with pytest.raises(ValueError):
        ops.TsdfVolume.from_dense(f, w[:5], None, (0, 0, 0), 0.1, 0.4)
    with pytest.raises(ValueError):
        ops.TsdfVolume.from_dense(f, w, None, (0, 0, 0), 0.0, 0.4)


def test_mesh_ply_round_trip_and_its_vertices_read_as_a_cloud(tmp_path, sphere):
    v, _, f, _ = sphere
    colors = (np.arange(len(v) * 3) % 251).astype(np.uint8).reshape(-1, 3)
    path = str(tmp_path / 'mesh.ply')
    ply.write_mesh(path, v, colors, f)
    with open(path, 'rb') as fh:
        head = fh.read(400).split(b'end_header\n')[0].decode('ascii').split('\n')
    assert head[:3] == ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % len(v)]
    assert head[3:9] == ['property float x', 'property float y', 'property float z', 'property uchar red', 'property uchar green',
                         'property uchar blue']
    assert head[9:11] == ['element face %d' % len(f), 'property list uchar int vertex_indices']
    assert os.path.getsize(path) == len('\n'.join(head)) + len('end_header\n') + 15 * len(v) + 13 * len(f)
    gv, gc, gf = ply.read_mesh(path)
    assert np.array_equal(gv, v) and np.array_equal(gc, colors) and np.array_equal(gf, f) and gf.dtype == np.int32
    assert np.array_equal(ply.read_ply_points(path), v)
    pv, pc = ply.read_ply(path)                           # the face element's property is not a vertex property
    assert np.array_equal(pv, v) and np.array_equal(pc, colors) and not ply.has_normals(path)
    white = str(tmp_path / 'white.ply')
    ply.write_mesh(white, v[:3], None, f[:0])
    wv, wc, wf = ply.read_mesh(white)
    assert np.array_equal(wv, v[:3]) and (wc == 255).all() and wf.shape == (0, 3)
    with pytest.raises(ValueError, match='face index'):
        ply.write_mesh(white, v[:3], None, np.array([[0, 1, 3]]))
    cloud = str(tmp_path / 'cloud.ply')
    ply.write_ply(cloud, v, colors)
    with pytest.raises(ValueError, match='not a mesh'):
        ply.read_mesh(cloud)


def _meta(shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device='meta')


def test_the_wrappers_argument_errors():
    d, c, im = _meta((3, 5, 7)), _meta((3, 16), torch.float64), _meta((3, 5, 7, 4))
    ok = dict(voxel=0.1, trunc=0.4, origin=(0, 0, 0), dims=(2, 2, 2))
    vol = ops.tsdf_integrate(d, c, images=im, **ok)                              # the host checks alone: nothing is launched
    assert vol.num_blocks == 0 and vol.device.type == 'meta' and vol.dims == (2, 2, 2)
    assert [tuple(t.shape) for t in ops.tsdf_mesh(vol)] == [(0, 3), (0, 3), (0, 3)]
    for bad in (dict(voxel=0.0), dict(voxel=float('nan')), dict(trunc=0.0), dict(trunc=float('inf')), dict(origin=(0, 0)),
                dict(origin=(0, float('nan'), 0)), dict(dims=(2, 2)), dict(dims=(0, 2, 2)), dict(dims=(2.5, 2, 2)),
                dict(dims=(1 << 10, 1 << 10, 1 << 7)), dict(pixel_centre=float('inf')), dict(max_blocks=0)):
        with pytest.raises(ValueError):
            ops.tsdf_integrate(d, c, images=im, **dict(ok, **bad))
    with pytest.raises(ValueError, match='cams'):
        ops.tsdf_integrate(d, _meta((2, 16), torch.float64), **ok)
    with pytest.raises(TypeError, match='cams'):
        ops.tsdf_integrate(d, _meta((3, 16)), **ok)
    with pytest.raises(TypeError, match='depths'):
        ops.tsdf_integrate(_meta((3, 5, 7), torch.float64), c, **ok)
    with pytest.raises(ValueError, match='depths'):
        ops.tsdf_integrate(_meta((3, 5, 7, 1)), c, **ok)
    with pytest.raises(ValueError, match='images'):
        ops.tsdf_integrate(d, c, images=_meta((3, 5, 7, 2)), **ok)
    with pytest.raises(ValueError, match='images'):
        ops.tsdf_integrate(d, c, images=_meta((3, 5, 8, 3)), **ok)
    with pytest.raises(ValueError, match='contiguous'):
        ops.tsdf_integrate(_meta((3, 7, 5)).transpose(1, 2), c, **ok)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.tsdf_integrate(torch.zeros(3, 5, 7), torch.zeros(3, 16, dtype=torch.float64), **ok)
    with pytest.raises(TypeError, match='TsdfVolume'):
        ops.tsdf_mesh(None)
    with pytest.raises(ValueError, match='min_weight'):
        ops.tsdf_mesh(vol, min_weight=float('nan'))
    host = ops.TsdfVolume.from_dense(np.ones((8, 8, 8)), np.ones((8, 8, 8)), None, (0, 0, 0), 1.0, 4.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.tsdf_mesh(host)
    with pytest.raises(ValueError, match='tsdf'):
        ops.TsdfVolume((0, 0, 0), 1.0, 4.0, (1, 1, 1), host.blocks, host.tsdf.reshape(1, 512), host.weight)


def test_the_c_abi_refuses_bad_arguments_without_a_launch():
    L = ops._lib.lib()
    import ctypes
    n = ctypes.c_long(0)
    assert L.atvs_tsdf_scan_scratch_size(5000, ctypes.byref(n)) == 0 and n.value >= 12
    assert L.atvs_tsdf_scan_scratch_size(-1, ctypes.byref(n)) == -2 and L.atvs_tsdf_scan_scratch_size(8, None) == -1
    org = (ctypes.c_double * 3)(0, 0, 0)
    assert L.atvs_tsdf_mark(None, None, 1, 4, 4, 0.1, 0.4, org, 2, 2, 2, 0.0, None, None, None) == -1
    assert L.atvs_tsdf_mark(None, None, 0, 4, 4, 0.1, 0.4, org, 2, 2, 2, 0.0, None, None, None) == -2
    assert L.atvs_tsdf_mark(8, 8, 1, 4, 4, 0.1, 0.4, org, 1 << 10, 1 << 10, 1 << 7, 0.0, 8, 8, None) == -2
    assert L.atvs_tsdf_mark(8, 8, 1, 4, 4, 0.0, 0.4, org, 2, 2, 2, 0.0, 8, 8, None) == -3
    assert L.atvs_tsdf_mark(8, 8, 1, 4, 4, 0.1, 0.0, org, 2, 2, 2, 0.0, 8, 8, None) == -3
    assert L.atvs_tsdf_integrate(8, 8, 2, 8, 1, 4, 4, 0.1, 0.4, org, 2, 2, 2, 0.0, 8, 8, 1, 8, 8, 8, 8, None) == -2      # two channels
    assert L.atvs_tsdf_integrate(8, None, 0, 8, 1, 4, 4, 0.1, 0.4, org, 2, 2, 2, 0.0, 8, 8, 9, 8, 8, None, 8, None) == -2   # 9 of 8 blocks
    assert L.atvs_tsdf_mesh_count(None, 1, 1, 1, 1, None, None, 1.0, None, None, None, None, None) == -1
    assert L.atvs_tsdf_mesh_count(8, 2, 1, 1, 1, 8, 8, 1.0, 8, 8, 8, 8, None) == -2                                   # two blocks in a box of one
    assert L.atvs_tsdf_mesh_count(8, 1, 1, 1, 1, 8, 8, float('nan'), 8, 8, 8, 8, None) == -3
    assert L.atvs_tsdf_mesh_emit(8, 1, 1, 1, 1, 0.1, org, 8, None, 8, 8, 8, 7 * 512 + 1, 0, 8, None, 8, None) == -2


def test_box_of_and_depth_bounds():
    origin, dims = mesh_fusion.box_of((0.0, 0.0, 0.0), (1.0, 2.0, 0.0), 0.125, 0.5)          # padded by trunc + one block = 1.5
    assert origin.tolist() == [-1.5, -1.5, -1.5] and dims == (4, 5, 3)
    origin, dims = mesh_fusion.box_of((0.0, 0.0, 0.0), (1.0, 2.0, 0.0), 0.05, 0.2)
    assert (origin + np.array(dims) * 0.4 >= np.array([1.0, 2.0, 0.0]) + 0.6).all() and dims[0] == 6
    with pytest.raises(ValueError):
        mesh_fusion.box_of((0, 0, 0), (1, -1, 1), 0.05, 0.2)
    cam = np.zeros(16)
    cam[[0, 4, 8]] = 1.0
    cam[9:12] = (0.5, 0.0, -1.0)
    cam[12:] = (10.0, 10.0, 2.0, 1.0)
    depth = np.zeros((1, 3, 5), np.float32)
    depth[0, 1, 2] = 2.0                                 # the principal point: on the axis
    depth[0, 1, 4] = 4.0
    lo, hi = mesh_fusion.depth_bounds(depth, cam[None])
    assert np.allclose(lo, (-0.5, 0.0, 3.0)) and np.allclose(hi, (0.3, 0.0, 5.0))
    assert mesh_fusion.depth_bounds(np.zeros((1, 3, 5), np.float32), cam[None]) == (None, None)
    for bad in (dict(voxel=0.0), dict(voxel=0.1, trunc_voxels=0.5), dict(voxel=0.1, min_weight=0.0), dict(voxel=0.1, max_blocks=0)):
        with pytest.raises(ValueError):
            mesh_fusion.check_options(**bad)


def test_mesh_report_counts(field):
    weight = np.ones_like(field)
    weight[:, :, 20:] = 0
    vol = ops.TsdfVolume.from_dense(field, weight, None, (0.0, 0.0, 0.0), H, 4.0)
    v, _, f = R.mesh_of_volume(vol)
    report = mesh_fusion.mesh_report(vol, (torch.from_numpy(v), None, torch.from_numpy(f)), 1.0, {'extract': 0.5})
    _, undirected = R.edge_stats(f)
    assert report['vertices'] == len(v) and report['faces'] == len(f) and report['blocks'] == vol.num_blocks
    assert report['boundary_edges'] == sum(1 for n in undirected.values() if n == 1) > 0
    assert report['valid_voxels'] == 32 * 32 * 20 and report['zero_area_faces'] >= 1 and report['seconds'] == {'extract': 0.5}


def test_mesh_needs_fuse_alike_in_run_eval_pc_and_cli(capsys):
    base = len(E._option_rules())
    fuse = dict(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2)
    assert len(E._option_rules(fuse=fuse)) == base                                # unchanged when mesh is not given
    rules = E._option_rules(fuse=fuse, mesh=dict(voxel=0.05))
    assert len(rules) == base + 2 and not any(b for b, _ in rules)
    broken = [m for b, m in E._option_rules(mesh=dict(voxel=0.05)) if b]
    assert len(broken) == 1 and '--mesh_voxel' in broken[0] and 'need --fuse' in broken[0]
    with pytest.raises(ValueError) as e:
        E.run_eval_pc('out', [], mesh=dict(voxel=0.05))
    assert str(e.value) == broken[0]
    with pytest.raises(SystemExit) as x:
        E.cli(['--mesh_voxel', '0.05'])
    assert x.value.code == 2 and broken[0] in ' '.join(capsys.readouterr().err.split())
    with pytest.raises(SystemExit) as x:
        E.cli(['--fuse', '--mesh_min_weight', '3'])
    assert x.value.code == 2 and 'need --mesh_voxel' in ' '.join(capsys.readouterr().err.split())
    with pytest.raises(SystemExit) as x:
        E.cli(['--fuse', '--mesh_voxel', '-1'])
    assert x.value.code == 2 and 'voxel must be positive' in ' '.join(capsys.readouterr().err.split())
    with pytest.raises(ValueError, match='min_weight'):
        E.run_eval_pc('out', [], fuse=fuse, mesh=dict(voxel=0.05, min_weight=0))
    # without the option nothing of it is passed on
    import argparse
    assert 'mesh' not in E._run_options(argparse.Namespace(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2, fuse=True))
    assert E._run_options(argparse.Namespace(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2, fuse=True, mesh_voxel=0.1,
                                             mesh_max_blocks=7))['mesh'] == dict(voxel=0.1, max_blocks=7)
    assert not os.path.exists('out')
