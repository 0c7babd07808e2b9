"""ops.mesh_grid and ops.mesh_nearest held to their buffers: their rows of the buffer contract (tests/mesh_distance_contract_rows.py,
which registers them in tests/buffer_contract_rows.py's table) run as tests/test_gpu_buffer_contract.py runs its rows, at every size
of that table's meshes (around the 256-lane workgroup, the 4096-cell grid and the 2048-counter scan tile, with NaN and inf
vertices), with the least reference budget (several builds into one buffer) and with 0, 1 and 255 | 256 | 257 queries, under
tests/guarded_alloc.py: run plain, then with every torch.empty turned into a guarded allocation filled with 0x00, then with 0xFF.
No guard byte may move, the results must have the same bits under both fills (an element a kernel skipped, or scratch it read
before writing it, differs), and every entry point must have run."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_contract_rows as BR  # noqa: E402
import guarded_alloc as GA  # noqa: E402
import mesh_distance_contract_rows as MR  # noqa: E402

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
