"""The ops of ops/mesh_smooth.py held to their buffers: their rows of the buffer contract (tests/mesh_smooth_contract_rows.py, which
registers them in tests/buffer_contract_rows.py's table) run as tests/test_gpu_buffer_contract.py runs its rows, at every size of
that table's meshes (around the 256-lane workgroup, the 1024-slot tables and the 2048-counter scan tile, with NaN and inf vertices,
a repeated index and a doubled face); and the whole smoothing and the normals at the fan (a hub of valence 300) and at sphere4 of
tests/mesh_smooth_cases.py, under tests/guarded_alloc.py: run plain, then with every torch.empty turned into a guarded allocation
filled with 0x00, then with 0xFF.  No guard byte may move, the results must have the same bits under both fills (an element a kernel
skipped, or scratch it read before writing it, differs), and every entry point must have run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_contract_rows as BR  # noqa: E402
import guarded_alloc as GA  # noqa: E402
import mesh_smooth_cases as C  # noqa: E402
import mesh_smooth_contract_rows as MR  # noqa: E402

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


@pytest.mark.parametrize('name', ['fan', 'sphere4'])
def test_the_whole_smoothing_and_the_normals_keep_to_their_buffers(cuda, name):
    from atvsnet_amd import ops
    v, f = C.mesh(name)
    want = C.restated(name, True)
    inputs = {'vertices': torch.from_numpy(np.array(v)), 'faces': torch.from_numpy(np.array(f))}           # (copies: the cases' arrays are read-only)

    def run(d, place):
        out, _ = ops.mesh_smooth(d['vertices'], d['faces'], C.ITERATIONS, C.TAUBIN[0], C.TAUBIN[1], pin_boundary=True)
        sums, incidences = ops.mesh_vertex_normal_sums(d['vertices'], d['faces'], want['extent']['max_extent'])
        return [out, sums, incidences, ops.mesh_normals_from_sums(place(sums))]

    names = ('vertices_out', 'sums', 'incidences', 'normals')
    with GA.recording_lib() as calls:
        done = GA.run_contract(run, inputs, list, cuda, names=names, what='mesh_smooth and the normals at %s' % name)
    assert set(MR._SMOOTH + MR._NORMALS[1:]) <= set(calls)
    selected = dict(zip(names, done.selected))
    assert np.array_equal(selected['vertices_out'].numpy().view(np.uint32), want['out'].view(np.uint32))
    assert np.array_equal(selected['incidences'].numpy(), want['incidences'])
    assert torch.empty is GA._ORIGINAL['empty']
