"""ops.mesh_sample_counts and ops.mesh_sample_points held to their buffers: their rows of the buffer contract
(tests/mesh_sample_contract_rows.py, which registers them in tests/buffer_contract_rows.py's table) run as
tests/test_gpu_buffer_contract.py runs its rows, at every size of that table's meshes (around the 256-lane workgroup, the 1024-slot
tables and the 2048-counter scan tile, with NaN and inf vertices); and both ops at the plane of tests/mesh_sample_cases.py (9522 faces:
more than a workgroup and a scan tile; at spacing 0.05 the face search runs in global memory across long runs of empty faces, at
0.01 in LDS), under tests/guarded_alloc.py: run plain, then with every torch.empty turned into a guarded allocation filled with
0x00, then with 0xFF.  No guard byte may move, the results must have the same bits under both fills (an element a kernel skipped,
or scratch it read before writing it, differs), and both entry points must have run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_contract_rows as BR  # noqa: E402
import guarded_alloc as GA  # noqa: E402
import mesh_sample_cases as C  # noqa: E402
import mesh_sample_contract_rows as MR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name,size', MR.cases(), ids=['%s[%s]' % c for c in MR.cases()])
def test_the_rows_of_the_buffer_contract(cuda, name, size):
    from atvsnet_amd import ops
    row = BR.ROWS[name]
    p = row.sizes[size]
    what = '%s at %s' % (name, size)
    with GA.recording_lib() as calls:
        done = GA.run_contract(lambda d, place: row.run(ops, d, place), row.build(p), row.select, cuda, names=row.names,
                               writable=row.writable, what=what)
    missing = [e for e in row.required(size) if e not in set(calls)]
    assert not missing, '%s: never reached %s (reached: %s)' % (what, missing, sorted(set(calls)))
    assert len(done.selected) == len(row.names), (what, len(done.selected), row.names)
    for fill, g in done.guards.items():
        made = [a.code for a in g.allocations if a.kind != 'input' and '/ops/' in a.site]
        if row.launches(p):
            for piece in row.outputs + row.scratch:
                assert any(piece in code for code in made), '%s, fill 0x%02X: no guarded allocation from a line with %r; made: %s' % (
                    what, fill, piece, made)
    assert torch.empty is GA._ORIGINAL['empty']


@pytest.mark.parametrize('spacing', [0.05, 0.01])
def test_both_ops_keep_to_their_buffers_at_the_plane(cuda, spacing):
    from atvsnet_amd import ops
    v, c, f = C.mesh('plane')
    want = C.restated('plane', spacing)
    inputs = {'vertices': torch.from_numpy(v), 'colors': torch.from_numpy(c), 'faces': torch.from_numpy(f)}

    def run(d, place):
        counts, areas, info = ops.mesh_sample_counts(d['vertices'], d['faces'], C.density(spacing), C.SEED)
        samples = ops.mesh_sample_points(d['vertices'], d['colors'], d['faces'], place(counts), C.SEED, normals=True)
        return [counts, areas, torch.tensor([info[k] for k in sorted(info)])] + list(samples)

    names = ('counts', 'areas', 'info', 'points', 'colors', 'normals', 'face')
    with GA.recording_lib() as calls:
        done = GA.run_contract(run, inputs, list, cuda, names=names, what='mesh_sample at the plane, spacing %g' % spacing)
    assert {'atvs_mesh_sample_counts', 'atvs_mesh_sample_offsets', 'atvs_mesh_sample_place'} <= set(calls)
    for fill, g in done.guards.items():
        made = [a.code for a in g.allocations if a.kind != 'input' and '/ops/' in a.site]
        for piece in ('counts = torch.empty', 'areas = torch.empty', 'words = torch.empty', 'scratch = torch.empty', 'offsets = torch.empty',
                      'points = torch.empty', 'face = torch.empty', 'colors_out = ', 'normals_out = torch.empty', 'info = torch.empty'):
            assert any(piece in code for code in made), (fill, piece, made)
    selected = dict(zip(names, done.selected))
    assert np.array_equal(selected['counts'].numpy(), want['counts']['counts'])
    assert np.array_equal(selected['points'].numpy().view(np.uint32), want['samples']['points'].view(np.uint32))
    assert np.array_equal(selected['face'].numpy(), want['samples']['face']) and np.array_equal(selected['colors'].numpy(), want['samples']['colors'])
    assert torch.empty is GA._ORIGINAL['empty']
