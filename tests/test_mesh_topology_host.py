"""The mesh topology feature on the host (no GPU): the ABI version and symbols, the C ABI's refusals without a launch, the wrappers'
argument checks on the `meta` device, clean_mesh's criteria through the restatement, the three command lines' parser errors, and
mesh_report on host tensors as it was."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import clean_mesh, eval_pointcloud, mesh_fusion
from atvsnet_amd.tools import ply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_topology_cases as MC  # noqa: E402
import mesh_topology_restated as T  # noqa: E402
import tsdf_restated as R  # noqa: E402

NAMES = ('atvs_mesh_components_scratch_size', 'atvs_mesh_components', 'atvs_mesh_select_scratch_size', 'atvs_mesh_select',
         'atvs_mesh_edge_census_scratch_size', 'atvs_mesh_edge_census')


def test_abi_version_and_symbols():
    L = _lib.lib()
    assert _lib.header_abi_version() >= 60 and L.atvs_abi_version() == _lib.header_abi_version()
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(L, name)
    assert ops.MESH_TOPOLOGY_MAX_FACES == _lib.header_macro('ATVS_MESH_TOPOLOGY_MAX_FACES') == 1 << 28
    assert ops.MESH_CENSUS_MIN_SLOTS == _lib.header_macro('ATVS_MESH_CENSUS_MIN_SLOTS')
    assert ops.MESH_CENSUS_WORDS == T.CENSUS_WORDS
    assert MC.VERTEX_LIMIT == ops.CLOUD_MAX_POINTS                  # the limit ops.mesh_render places on vertices


def test_the_c_abi_refuses_bad_arguments_without_a_launch():
    L = _lib.lib()
    n = ctypes.c_long(0)
    big_f, big_v = (1 << 28) + 1, (1 << 30) + 1
    assert L.atvs_mesh_components_scratch_size(100, 50, ctypes.byref(n)) == 0 and n.value >= 12 * 100
    assert L.atvs_mesh_components_scratch_size(0, 0, ctypes.byref(n)) == 0 and n.value > 0
    assert L.atvs_mesh_components_scratch_size(100, 50, None) == -1
    assert L.atvs_mesh_components_scratch_size(-1, 50, ctypes.byref(n)) == -2
    assert L.atvs_mesh_components_scratch_size(big_v, 50, ctypes.byref(n)) == -2
    assert L.atvs_mesh_components_scratch_size(100, big_f, ctypes.byref(n)) == -2
    assert L.atvs_mesh_components_scratch_size(1 << 30, 1 << 28, ctypes.byref(n)) == 0 and n.value >= 12 << 30
    assert L.atvs_mesh_components(None, 1, 3, 8, 1 << 20, 8, 8, 8, 8, 8, None) == -1          # faces
    assert L.atvs_mesh_components(8, 1, 3, None, 1 << 20, 8, 8, 8, 8, 8, None) == -1          # scratch
    assert L.atvs_mesh_components(8, 1, 3, 8, 1 << 20, 8, 8, 8, 8, None, None) == -1          # info
    assert L.atvs_mesh_components(8, -1, 3, 8, 1 << 20, 8, 8, 8, 8, 8, None) == -2
    assert L.atvs_mesh_components(8, 1, big_v, 8, 1 << 40, 8, 8, 8, 8, 8, None) == -2
    assert L.atvs_mesh_components(8, big_f, 3, 8, 1 << 40, 8, 8, 8, 8, 8, None) == -2
    assert L.atvs_mesh_components(8, 1, 3, 8, 16, 8, 8, 8, 8, 8, None) == -2                  # a short scratch

    assert L.atvs_mesh_select_scratch_size(100, 50, ctypes.byref(n)) == 0 and n.value >= 4 * 150
    assert L.atvs_mesh_select_scratch_size(100, 50, None) == -1
    assert L.atvs_mesh_select_scratch_size(100, -1, ctypes.byref(n)) == -2
    assert L.atvs_mesh_select_scratch_size(big_v, 1, ctypes.byref(n)) == -2
    assert L.atvs_mesh_select(None, None, 3, 8, 8, 1, 8, 1 << 20, 8, None, 8, 8, 8, None) == -1            # vertices
    assert L.atvs_mesh_select(8, 8, 3, 8, 8, 1, 8, 1 << 20, 8, None, 8, 8, 8, None) == -1                  # colors without colors_out
    assert L.atvs_mesh_select(8, None, 3, 8, None, 1, 8, 1 << 20, 8, None, 8, 8, 8, None) == -1            # keep
    assert L.atvs_mesh_select(8, None, 3, 8, 8, big_f, 8, 1 << 40, 8, None, 8, 8, 8, None) == -2
    assert L.atvs_mesh_select(8, None, 3, 8, 8, 1, 8, 16, 8, None, 8, 8, 8, None) == -2                    # a short scratch

    assert L.atvs_mesh_edge_census_scratch_size(0, ctypes.byref(n)) == 0 and n.value == 16 * ops.MESH_CENSUS_MIN_SLOTS
    assert L.atvs_mesh_edge_census_scratch_size(1000, ctypes.byref(n)) == 0 and n.value == 16 * 8192          # 6000 -> 2^13 slots
    assert L.atvs_mesh_edge_census_scratch_size(1 << 28, ctypes.byref(n)) == 0 and n.value == 16 << 31
    assert L.atvs_mesh_edge_census_scratch_size(1000, None) == -1
    assert L.atvs_mesh_edge_census_scratch_size(-1, ctypes.byref(n)) == -2
    assert L.atvs_mesh_edge_census_scratch_size(big_f, ctypes.byref(n)) == -2
    assert L.atvs_mesh_edge_census(None, 1, 3, 8, 1 << 20, 8, None) == -1
    assert L.atvs_mesh_edge_census(8, 1, 3, 8, 1 << 20, None, None) == -1
    assert L.atvs_mesh_edge_census(8, 1, big_v, 8, 1 << 20, 8, None) == -2
    assert L.atvs_mesh_edge_census(8, big_f, 3, 8, 1 << 40, 8, None) == -2
    assert L.atvs_mesh_edge_census(8, 1000, 3000, 8, 16 * 8192 - 1, 8, None) == -2                          # a short scratch


def _meta(shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device='meta')


def test_the_wrappers_argument_errors():
    v, c, f, k = _meta((5, 3)), _meta((5, 3), torch.uint8), _meta((2, 3), torch.int32), _meta((2,), torch.uint8)
    vc, fc, nf, nv = ops.mesh_components(f, 5)                        # the host checks alone run on `meta`
    assert tuple(vc.shape) == (5,) and tuple(fc.shape) == (2,) and vc.dtype == fc.dtype == nf.dtype == nv.dtype == torch.int32
    ov, oc, of, vm = ops.mesh_select(v, c, f, k)
    assert tuple(ov.shape) == (5, 3) and oc.dtype == torch.uint8 and of.dtype == torch.int32 and tuple(vm.shape) == (5,)
    assert ops.mesh_select(v, None, f, k)[1] is None
    assert ops.mesh_edge_census(f, 5) == dict.fromkeys(T.CENSUS_WORDS, 0)
    for fn in (ops.mesh_components, ops.mesh_edge_census):
        with pytest.raises(TypeError, match='faces'):
            fn(f.long(), 5)
        with pytest.raises(ValueError, match='faces'):
            fn(_meta((2, 4), torch.int32), 5)
        with pytest.raises(ValueError, match='faces'):
            fn(_meta((3, 2, 3), torch.int32)[:, 0], 5)              # not contiguous
        with pytest.raises(ValueError, match='num_vertices'):
            fn(f, -1)
        with pytest.raises(ValueError, match='num_vertices'):
            fn(f, (1 << 30) + 1)
        with pytest.raises(ValueError, match='num_vertices'):
            fn(f, 5.0)
        with pytest.raises(TypeError, match='faces'):
            fn(np.zeros((2, 3), np.int32), 5)
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(torch.zeros((2, 3), dtype=torch.int32), 5)
    with pytest.raises(TypeError, match='vertices'):
        ops.mesh_select(v.double(), c, f, k)
    with pytest.raises(TypeError, match='colors'):
        ops.mesh_select(v, c.float(), f, k)
    with pytest.raises(ValueError, match='colors'):
        ops.mesh_select(v, _meta((4, 3), torch.uint8), f, k)
    with pytest.raises(TypeError, match='keep'):
        ops.mesh_select(v, c, f, k.bool())
    with pytest.raises(ValueError, match='keep'):
        ops.mesh_select(v, c, f, _meta((3,), torch.uint8))
    with pytest.raises(ValueError, match='keep'):
        ops.mesh_select(v, c, f, _meta((2, 1), torch.uint8))
    with pytest.raises(TypeError, match='faces'):
        ops.mesh_select(v, c, f.long(), k)
    with pytest.raises(RuntimeError, match='faces'):
        ops.mesh_select(v, c, torch.zeros((2, 3), dtype=torch.int32), k)
    with pytest.raises(RuntimeError, match='keep'):
        ops.mesh_select(v, c, f, torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.mesh_select(torch.zeros(5, 3), None, torch.zeros((2, 3), dtype=torch.int32), torch.zeros(2, dtype=torch.uint8))


def test_the_criteria():
    counts = [5, 100, 25, 100, 1, 25]
    keep = clean_mesh.keep_components
    assert keep(counts, min_faces=25).tolist() == [False, True, True, True, False, True]
    assert keep(counts, min_faces=26).tolist() == [False, True, False, True, False, False]
    # min_ratio exactly at the boundary: 25 * 4 >= 1 * 100 holds, and a ratio one part in 10^30 above 1/4 does not
    assert keep(counts, min_ratio=0.25).tolist() == [False, True, True, True, False, True]
    assert keep(counts, min_ratio='0.25').tolist() == keep(counts, min_ratio=Fraction(1, 4)).tolist() == keep(counts, min_ratio=0.25).tolist()
    assert keep(counts, min_ratio=Fraction(1, 4) + Fraction(1, 10 ** 30)).tolist() == [False, True, False, True, False, False]
    assert keep([3, 30], min_ratio='0.1').tolist() == [True, True]             # the string is 1/10 ...
    assert keep([3, 30], min_ratio=0.1).tolist() == [False, True]              # ... the float 0.1 is a little more
    assert keep(counts, min_ratio=0).all() and keep(counts, min_ratio=1).tolist() == [False, True, False, True, False, False]
    # keep_largest: ties go to the lower id
    assert keep(counts, keep_largest=1).tolist() == [False, True, False, False, False, False]
    assert keep(counts, keep_largest=2).tolist() == [False, True, False, True, False, False]
    assert keep(counts, keep_largest=3).tolist() == [False, True, True, True, False, False]
    assert keep(counts, keep_largest=99).all()
    # ANDed
    assert keep(counts, min_faces=25, keep_largest=3, min_ratio=1).tolist() == [False, True, False, True, False, False]
    assert keep(counts, min_faces=101, keep_largest=3).tolist() == [False] * 6
    assert keep([], keep_largest=1).tolist() == []
    with pytest.raises(ValueError, match='at least one of min_faces, min_ratio, keep_largest'):
        keep(counts)
    with pytest.raises(ValueError, match='at least one'):
        clean_mesh.clean(np.zeros((3, 3), np.float32), None, np.zeros((1, 3), np.int32))      # before anything touches a GPU
    for bad in (dict(min_faces=0), dict(min_faces=2.5), dict(min_faces=True), dict(keep_largest=0), dict(keep_largest=1.5),
                dict(min_ratio=-0.1), dict(min_ratio=1.5), dict(min_ratio=float('nan')), dict(min_ratio='a tenth')):
        with pytest.raises(ValueError, match=list(bad)[0]):
            keep(counts, **bad)


def test_the_criteria_through_the_restatement():
    vertices, faces, of_sphere = MC.sphere_and_shells()
    _, face_component, face_count, _ = T.components(faces, len(vertices))
    for criterion in (dict(min_faces=9), dict(min_ratio='1/100'), dict(keep_largest=1)):
        flags = clean_mesh.keep_components(face_count, **criterion)
        assert np.array_equal(flags[face_component], of_sphere)
        v, _, f, _ = T.clean(vertices, None, faces, flags)
        assert (len(v), len(f)) == (5946, 11888)
    assert clean_mesh.keep_components(face_count, min_faces=8).all()


def test_command_lines_refuse(capsys, tmp_path):
    def refused(cli, argv, text):
        with pytest.raises(SystemExit) as e:
            cli(argv)
        assert e.value.code == 2 and text in ' '.join(capsys.readouterr().err.split())

    mesh, maps = tmp_path / 'mesh.ply', tmp_path / 'maps'
    maps.mkdir()
    ply.write_mesh(str(mesh), np.zeros((3, 3), np.float32), None, np.array([[0, 1, 2]], np.int32))
    io = ['--in', str(mesh), '--out', str(tmp_path / 'out.ply')]
    refused(clean_mesh.cli, io, 'nothing to do: give at least one of --min_faces, --min_ratio, --keep_largest')
    refused(clean_mesh.cli, io + ['--min_faces', '0'], '--min_faces must be a positive integer')
    refused(clean_mesh.cli, io + ['--min_ratio', '2'], '--min_ratio must be a number in 0..1')
    refused(clean_mesh.cli, io + ['--min_ratio', 'much'], '--min_ratio must be a number in 0..1')
    refused(clean_mesh.cli, io + ['--keep_largest', '-1'], '--keep_largest must be a positive integer')
    refused(clean_mesh.cli, ['--in', str(tmp_path / 'none.ply'), '--out', 'x.ply', '--keep_largest', '1'], 'no such file')
    (tmp_path / 'broken.ply').write_bytes(b'ply\nformat ascii 1.0\nelement vertex 1\n')
    refused(clean_mesh.cli, ['--in', str(tmp_path / 'broken.ply'), '--out', 'x.ply', '--keep_largest', '1'], 'broken.ply')
    fusion = ['--maps', str(maps), '--voxel', '0.1', '--out', str(tmp_path / 'm.ply')]
    refused(mesh_fusion.cli, fusion + ['--clean_keep_largest', '1'], 'they need --clean_out')
    refused(mesh_fusion.cli, fusion + ['--clean_out', str(tmp_path / 'c.ply')], '--clean_out needs one of')
    refused(mesh_fusion.cli, fusion + ['--clean_out', 'c.ply', '--clean_min_faces', '0'], '--clean_min_faces must be a positive integer')
    refused(eval_pointcloud.cli, ['--fuse', '--mesh_clean_keep_largest', '1'], '--mesh_clean_keep_largest need --mesh_voxel')
    refused(eval_pointcloud.cli, ['--fuse', '--mesh_voxel', '0.1', '--mesh_clean_min_ratio', '7'], '--mesh_clean_min_ratio must be')
    refused(eval_pointcloud.cli, ['--mesh_voxel', '0.1', '--mesh_clean_min_faces', '5'], 'need --fuse')
    for parser, prefix in ((clean_mesh.make_parser(), ''), (mesh_fusion.make_parser(), 'clean_')):
        text = ' '.join(parser.format_help().split())
        for name in ('min_faces', 'min_ratio', 'keep_largest'):
            assert '--%s%s' % (prefix, name) in text
        assert text.count('(no default)') == 3                       # no threshold has a default


def test_the_consistency_table_gains_its_row_only_with_the_option():
    E = eval_pointcloud
    fuse = dict(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2)
    base = len(E._option_rules(fuse=fuse, mesh=dict(voxel=0.05)))
    rules = E._option_rules(fuse=fuse, mesh=dict(voxel=0.05, clean=dict(keep_largest=1)))
    assert len(rules) == base + 1 and not any(b for b, _ in rules)
    broken = [m for b, m in E._option_rules(fuse=fuse, mesh=dict(clean=dict(keep_largest=1))) if b]
    assert '--mesh_clean_keep_largest need --mesh_voxel' in broken[0]
    with pytest.raises(ValueError, match='mesh_clean'):
        E.run_eval_pc('out', [], fuse=fuse, mesh=dict(clean=dict(keep_largest=1)))
    with pytest.raises(ValueError, match='keep_largest'):
        E.run_eval_pc('out', [], fuse=fuse, mesh=dict(voxel=0.05, clean=dict(keep_largest=0)))
    import argparse
    flags = argparse.Namespace(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2, fuse=True, mesh_voxel=0.1)
    assert E._run_options(flags)['mesh'] == {'voxel': 0.1}            # without the options nothing of them is passed on
    flags.mesh_clean_min_ratio = '0.05'
    assert E._run_options(flags)['mesh'] == {'voxel': 0.1, 'clean': {'min_ratio': '0.05'}}


def test_scene_mesh_checks_its_criteria_without_a_gpu():
    with pytest.raises(ValueError, match='min_faces'):
        mesh_fusion.check_options(0.1, clean=dict(min_faces=0))
    with pytest.raises(ValueError, match='at least one'):
        mesh_fusion.check_options(0.1, clean={})
    assert mesh_fusion.check_options(0.1, clean=dict(min_ratio='1/3')) == mesh_fusion.check_options(0.1)


def test_mesh_report_on_host_tensors_is_unchanged():
    field = R.sphere_field(32, MC.H, MC.RADIUS, MC.CENTRE)
    weight = np.ones_like(field)
    weight[:, :, 20:] = 0
    vol = ops.TsdfVolume.from_dense(field, weight, None, (0.0, 0.0, 0.0), MC.H, 4.0)
    v, f = MC._sphere(clipped=True)
    report = mesh_fusion.mesh_report(vol, (torch.from_numpy(v), None, torch.from_numpy(f)), 1.0, {'extract': 0.5})
    census = T.edge_census(f, len(v))
    _, undirected = R.edge_stats(f)
    assert report['boundary_edges'] == census['boundary'] == sum(1 for n in undirected.values() if n == 1) == 130
    assert report['boundary_edges'] == mesh_fusion.host_boundary_edges(f.astype(np.int64), len(v))
    assert sorted(report) == ['blocks', 'boundary_edges', 'dims', 'faces', 'min_weight', 'origin', 'seconds', 'trunc', 'valid_voxels',
                              'vertices', 'voxel', 'zero_area_faces']
    assert report['seconds'] == {'extract': 0.5} and report['zero_area_faces'] >= 1 and report['faces'] == len(f)


def test_clean_mesh_reads_both_kinds_of_file(tmp_path):
    v = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25]], np.float32)
    ply.write_mesh(str(tmp_path / 'own.ply'), v, np.array([[1, 2, 3]] * 3, np.uint8), np.array([[0, 1, 2]], np.int32))
    gv, gc, gf = clean_mesh.read_mesh(str(tmp_path / 'own.ply'))
    assert np.array_equal(gv, v) and gc.tolist() == [[1, 2, 3]] * 3 and gf.tolist() == [[0, 1, 2]]
    (tmp_path / 'other.ply').write_text('ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n'
                                        'element face 1\nproperty list uchar int vertex_index\nend_header\n'
                                        '0 0 0\n1 0 0.5\n0 1 0.25\n3 0 1 2\n')
    gv, gc, gf = clean_mesh.read_mesh(str(tmp_path / 'other.ply'))
    assert np.array_equal(gv, v) and gc is None and gf.tolist() == [[0, 1, 2]]
