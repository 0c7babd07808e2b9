"""Every ops function that takes caller-owned buffers after the network, held to its buffers (tests/buffer_contract_rows.py has
the rows, tests/guarded_alloc.py the guard): run plain, then with every torch.empty it makes turned into a guarded allocation
filled with 0x00, then with 0xFF.  No guard or round-up byte may move, no input may change, the specified part of the result must
have the same bits in the three runs (an element a kernel skipped, or scratch it read before writing it, differs between the
fills), every entry point the row names must have run, and every output and scratch the row lists must have been handed out under
the guard.  Each case prints what it covered: run with -s for the record."""
import pytest
import torch

import buffer_contract_rows as BR
import guarded_alloc as GA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops(cuda):
    from atvsnet_amd import ops as o
    return o


def test_the_guard_on_the_device(cuda):
    """What tests/test_guarded_alloc_host.py holds on the CPU, where it can be held without a stray write: the layout, the fills
    and a clean check on the device the rows run on."""
    with GA.guarded(cuda, 0xFF) as g:
        out = torch.empty((5, 3), dtype=torch.float32, device=cuda)
        words = torch.empty(7, dtype=torch.int64, device='cuda')
        none = torch.empty((0, 3), dtype=torch.int32, device=cuda)
        z = torch.zeros(9, dtype=torch.float64, device=cuda)
        host = torch.empty(4)
        placed = g.place(torch.arange(6, dtype=torch.float32, device=cuda))
        assert [a.kind for a in g.allocations] == ['empty', 'empty', 'empty', 'zeros', 'input'] and host.device.type == 'cpu'
        assert all(t.data_ptr() % 256 == 0 and t.is_contiguous() and t.device == cuda for t in (out, words, z, placed))
        assert bool(torch.isnan(out).all()) and words.tolist() == [-1] * 7 and none.shape == (0, 3) and not z.any()
        b = g._buffers[0]
        assert b.guard == GA.GUARD and len(b.raw[b.start - b.guard:b.start].unique()) == 256
        out.copy_(torch.ones(5, 3))
        words.zero_()
        g.check()
    with GA.guarded(cuda, 0x00) as g:
        assert torch.empty(3, dtype=torch.float32, device=cuda).tolist() == [0.0] * 3
    assert torch.empty is GA._ORIGINAL['empty']


@pytest.mark.parametrize('name,size', BR.cases(), ids=['%s[%s]' % c for c in BR.cases()])
def test_buffer_contract(ops, cuda, name, size):
    row = BR.ROWS[name]
    p = row.sizes[size]
    inputs = row.build(p)
    what = '%s at %s' % (name, size)
    with GA.recording_lib() as calls:
        done = GA.run_contract(lambda d, place: row.run(ops, d, place), inputs, row.select, cuda, names=row.names,
                               writable=row.writable, what=what)
    reached = sorted(set(calls))
    missing = [e for e in row.required(size) if e not in reached]
    assert not missing, '%s: never reached %s (reached: %s)' % (what, missing, reached)
    assert len(done.selected) == len(row.names), (what, len(done.selected), row.names)
    for fill, g in done.guards.items():
        made = [a for a in g.allocations if a.kind != 'input' and ('/ops/' in a.site or a.site.endswith('buffer_contract_rows.py'))]
        count, nbytes = len(made), sum(a.nbytes for a in made)
        if row.launches(p):
            for piece in row.outputs + row.scratch:
                assert any(piece in a.code for a in made), '%s, fill 0x%02X: no guarded allocation from a line with %r; made: %s' % (
                    what, fill, piece, [a.code for a in made])
    compared = ', '.join('%s %s' % (n, 'None' if t is None else '%s (%d of %d elements not 0)' % (
        tuple(t.shape), int((GA.bits(t) != 0).sum()), t.numel())) for n, t in zip(row.names, done.selected))
    print('\n%s: %d guarded allocations of %d bytes by the ops (and %d placed inputs); reached %s; compared %s' % (
        what, count, nbytes, sum(a.kind == 'input' for a in g.allocations), ', '.join(reached) or 'no entry point (nothing to launch)',
        compared))
    assert torch.empty is GA._ORIGINAL['empty']
