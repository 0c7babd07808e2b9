"""Every ops function behind the network held to its buffers (tests/network_contract_rows.py has the rows, tests/guarded_alloc.py the
guard), the body of tests/test_gpu_buffer_contract.py: run plain, then with every torch.empty the op makes turned into a guarded
allocation filled with 0x00, then with 0xFF.  No guard or round-up byte may move, no input may change, no element outside the
channel slice (or the planes) an op is given to write may change, the specified part of the result must have the same bits in the
three runs, every entry point the size names must have run, every output and scratch the row lists must have been handed out under
the guard, the arranged weights lie under the guard too, and no pooled device word may be made inside a block.  Then the two
networks once, eager, under the guard.  Each case prints what it covered: run with -s for the record.

The guard is at least as large as its payload, so a stray store lands in pattern bytes and is reported: nothing here makes a kernel
fault."""
import time

import pytest
import torch

import guarded_alloc as GA
import network_contract_rows as NR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops(cuda):
    from atvsnet_amd import ops as o
    return o


def pools(ops):
    """[(name, tensor)] of every device buffer the ops make on first use and keep."""
    return [('nonfinite_flag[%s]' % k, t) for k, t in ops._flag_pool.items()] + \
        [('_fin_counter[%s]' % k, ent[0]) for k, ent in ops._fin_pool.items()]


def warm(ops, device):
    ops.nonfinite_flag(device)
    ops._fin_counter(device)
    for i in range(3):
        ops._side_stream(device, i)


@pytest.mark.parametrize('name,size', NR.cases(), ids=['%s[%s]' % c for c in NR.cases()])
def test_network_contract(ops, cuda, name, size):
    row = NR.ROWS[name]
    p = row.sizes[size]
    inputs = row.build(p)
    what = '%s at %s' % (name, size)
    writable = dict({k: True for k in row.writable}, **row.slices(p))
    with GA.recording_lib() as calls:
        done = GA.run_contract(lambda d, place: row.run(ops, d, place), inputs, row.select, cuda, names=row.names, writable=writable, what=what,
                               warm=lambda: warm(ops, cuda), pools=lambda: pools(ops), around=lambda place: GA.weights_under(place, ops, **p['cfg']))
    reached = sorted(set(calls))
    missing = [e for e in row.required(size) if e not in reached]
    assert not missing, '%s: never reached %s (reached: %s)' % (what, missing, reached)
    assert len(done.selected) <= len(row.names), (what, len(done.selected), row.names)
    wanted = row.outputs(p) if callable(row.outputs) else row.outputs
    for fill, g in done.guards.items():
        made = [a for a in g.allocations if a.kind != 'input' and '/ops/' in a.site]
        weights = [a for a in g.allocations if a.kind == 'input' and a.site.endswith('packing.py')]
        for piece in tuple(wanted) + row.scratch:
            assert any(piece in a.code for a in made), '%s, fill 0x%02X: no guarded allocation from a line with %r; made: %s' % (
                what, fill, piece, [a.code for a in made])
    compared = ', '.join('%s %s' % (n, 'None' if t is None else '%s (%d of %d elements not 0)' % (
        tuple(t.shape), int((GA.bits(t) != 0).sum()), t.numel())) for n, t in zip(row.names, done.selected))
    print('\n%s: %d guarded allocations of %d bytes by the ops, %d arranged-weight tensors of %d bytes and %d placed inputs under the guard '
          '(%d with a slice mask); reached %s; compared %s' % (
              what, len(made), sum(a.nbytes for a in made), len(weights), sum(a.nbytes for a in weights),
              sum(a.kind == 'input' for a in g.allocations) - len(weights), len(row.slices(p)), ', '.join(reached), compared))
    assert torch.empty is GA._ORIGINAL['empty'] and len(pools(ops)) >= 2
    if p['cfg'].get('fused_finalize'):
        assert done.selected[3] is not None and not bool(done.selected[3].any()), '%s: an arrival ticket was not left at zero' % what


# ----------------------------------------------------------------------------------------------------- the whole network, eager
def _whole(ops, cuda, views, D, infer, volumes):
    from atvsnet_amd import synthetic
    imgs, cams = synthetic.make_inputs(views, 128, 160, D)
    inputs = {'imgs': torch.from_numpy(imgs), 'cams': torch.from_numpy(cams)}
    names = ['depth map'] + list(volumes)

    def run(d, place):
        G = {}
        depth = infer(d['imgs'], d['cams'], D, G)
        return [depth] + [G[k] for k in volumes]
    t0 = time.time()
    with GA.recording_lib() as calls:
        done = GA.run_contract(run, inputs, list, cuda, names=names, what='%d views, 128 x 160, D = %d' % (views, D), warm=lambda: warm(ops, cuda),
                               pools=lambda: pools(ops), around=lambda place: GA.weights_under(place, ops))
    seconds = time.time() - t0
    g = done.guards[0xFF]
    made = [a for a in g.allocations if a.kind != 'input']
    print('\n%d views at 128 x 160, D = %d, eager, three runs in %.1f s: %d guarded allocations of %.1f MB, %d placed tensors (images, cameras, '
          'arranged weights); %d launches of %d entry points; compared %s' % (
              views, D, seconds, len(made), sum(a.nbytes for a in made) / 1e6, len(g.allocations) - len(made), len(calls), len(set(calls)), ', '.join(names)))
    assert tuple(done.selected[0].shape) == (1, 128, 160, 1) and bool(torch.isfinite(done.selected[0]).all())
    assert len(set(calls)) > 20 and len(made) > 100
    return done


def test_the_two_view_network_eager_under_the_guard(ops, cuda, weights):
    from atvsnet_amd.atvsnet import example as ex
    assert ops.cfg.side_streams
    _whole(ops, cuda, 2, 32, lambda imgs, cams, D, G: ex.infer_twoview(imgs, cams, D), ())


MULTIVIEW_VOLUMES = ('depth_agg_init', 'cost_volume_agg', 'prob_volume_agg', 'refined_cost_volume_agg', 'refined_prob_volume_agg')


def test_the_three_view_network_eager_under_the_guard(ops, cuda, weights):
    from atvsnet_amd.atvsnet import example as ex
    assert ops.cfg.side_streams
    _whole(ops, cuda, 3, 32, lambda imgs, cams, D, G: ex.infer_multiview(imgs, cams, D, G), MULTIVIEW_VOLUMES)
