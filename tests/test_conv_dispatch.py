"""No GPU: which kernel family every convolution of the two pipelines gets, and whether a lazy input (a pending batch norm or
skip sum) is formed on load, on meta tensors -- against tests/golden/conv_dispatch.json.

Each case records one event per call, in call order: 'conv:<family>' for every ops.conv (ops.conv_plan's family, '+' when the
lazy input is formed on load) and the name of every other convolution entry point and materialising pass (bn_apply, bn_add)
of the host layer.  The table holds what the dispatch chose when it was recorded; a difference is a change of the kernels a
layer gets (the outputs may stay right and only the speed change, which no other test sees)."""
import contextlib
import json
import os
import sys

import pytest
import torch

from atvsnet_amd import ops, variables
from atvsnet_amd.atvsnet import example as ex

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'conv_dispatch.json')
SHAPES = {'160x128_D32': (128, 160, 32), '640x512_D192': (512, 640, 192)}
CASES = ([(s, p, {'split16': on}) for s in SHAPES for p in ('multiview', 'twoview') for on in (True, False)]
         + [('160x128_D32', 'multiview', {k: False}) for k in ('sum_on_load', 'head_sum', 'prologue')])
COUNTED = ('bn_apply', 'bn_add', 'conv_siblings', 'conv_split_into_plane', 'conv3d_transpose_s2', 'conv3d_8to1',
           'refine_stems', 'bottleneck', 'conv2d_tail', 'aanet_fused', 'aanet_combine')


def case_id(shape, pipeline, switches):
    return '%s/%s/%s' % (shape, pipeline, ','.join('%s=%d' % kv for kv in sorted(switches.items())))


@contextlib.contextmanager
def _replaced(orig, wrapper):
    """Replace the function `orig` by `wrapper` under every name the package holds it by."""
    mods = [m for n, m in list(sys.modules.items()) if n.startswith('atvsnet_amd') and m is not None]
    hits = [(m, k) for m in mods for k, v in list(vars(m).items()) if v is orig]
    for m, k in hits:
        setattr(m, k, wrapper)
    try:
        yield
    finally:
        for m, k in hits:
            setattr(m, k, orig)


def _counting(events, name):
    orig = getattr(ops, name)

    def wrapper(*a, **k):
        events.append(name)
        return orig(*a, **k)
    return _replaced(orig, wrapper)


@contextlib.contextmanager
def _conv_families(events):
    """One event per ops.conv, when it returns (after the passes it may run first): the plan it launched.  Only ops.conv's
    own name for conv_plan is wrapped (the norm_on_load_*_ok predicates reach it through theirs)."""
    from atvsnet_amd.ops import convolution
    plan, conv, plans = convolution.conv_plan, convolution.conv, []

    def planned(*a, **k):
        plans.append(plan(*a, **k))
        return plans[-1]

    def recorded(*a, **k):
        y = conv(*a, **k)
        p = plans.pop()
        events.append('conv:%s%s' % (p.family, '+' if p.on_load else ''))
        return y
    convolution.conv_plan = planned
    try:
        with _replaced(conv, recorded):
            yield
    finally:
        convolution.conv_plan = plan


def record(shape, pipeline, switches, conv_families=_conv_families):
    """The event list of one case (see the module docstring)."""
    H, W, D = SHAPES[shape]
    views = 5 if pipeline == 'multiview' else 2
    imgs = torch.empty((1, views, H, W, 3), dtype=torch.float32, device='meta')
    cams = torch.empty((1, views, 2, 4, 4), dtype=torch.float32, device='meta')
    variables.default_store().init_synthetic(1234)
    events = []
    with contextlib.ExitStack() as stack:
        for name in COUNTED:
            stack.enter_context(_counting(events, name))
        stack.enter_context(conv_families(events))
        stack.enter_context(ops.configure(clear_pack_cache=True, **switches))
        if pipeline == 'multiview':
            ex.infer_multiview(imgs, cams, D, view_streams=False)
        else:
            ex.infer_twoview(imgs, cams, D)
    return events


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('shape,pipeline,switches', CASES, ids=[case_id(*c) for c in CASES])
def test_every_convolution_gets_the_recorded_kernel(shape, pipeline, switches):
    want = _golden()[case_id(shape, pipeline, switches)].split()
    got = record(shape, pipeline, switches)
    assert got == want


def test_the_table_covers_the_lazy_forms():
    """The cases exercise what they are there for: the fp32 path and each switch turned off materialise more lazy inputs
    (bn_apply / bn_add passes) than the default."""
    def passes(case):
        ev = _golden()[case].split()
        return ev.count('bn_apply'), ev.count('bn_add')
    assert passes('640x512_D192/multiview/split16=1') == (13, 8)
    assert passes('640x512_D192/multiview/split16=0') == (27, 14)
    assert passes('160x128_D32/multiview/split16=1') == (23, 8)
    assert passes('160x128_D32/multiview/sum_on_load=0') == (25, 15)
    assert passes('160x128_D32/multiview/head_sum=0') == (23, 9)
    assert passes('160x128_D32/multiview/prologue=0') == (27, 14)


def test_norm_on_load_predicates_ask_the_plan():
    """network.py asks norm_on_load_*_ok before it hands ops.conv a lazy input; both answers come from ops.conv_plan."""
    G, D, H, W = 2, 8, 16, 32
    meta = lambda *s: torch.empty(s, dtype=torch.float32, device='meta')       # noqa: E731
    pend3 = ops.PendingBN(meta(G, D, H, W, 16), meta(G, 3, 16), True)
    pend2 = ops.PendingBN(meta(G, H, W, 64), meta(G, 3, 64), True)
    with ops.configure(split16=True):
        assert ops.norm_on_load_3d_ok(pend3, 3, 16) and ops.norm_on_load_3d_ok(pend3, 3, 32, stride=2)
        assert ops.conv_plan((D, H, W), 3, 16, 16, lazy='bn')[:2] == ('c16b_sum', True)
        assert ops.conv_plan((D, H, W), 3, 16, 16, lazy='sum')[:2] == ('c16b_sum', True)
        assert ops.conv_plan((D, H, W), 3, 16, 32, stride=2, lazy='bn')[:2] == ('s2b_norm', True)
        assert ops.norm_on_load_2d_ok(pend2, 3, 64) and ops.norm_on_load_2d_ok(pend2, 1, 64)
        assert ops.conv_plan((H, W), 3, 64, 64, lazy='bn')[:2] == ('conv2d_lds', True)
    with ops.configure(split16=False):
        assert not ops.norm_on_load_3d_ok(pend3, 3, 16)
        assert ops.conv_plan((D, H, W), 3, 16, 16, lazy='bn')[:2] == ('c16', False)
        assert ops.conv_plan((H, W), 3, 64, 64, lazy='bn')[:2] == ('conv2d_lds', False)
        assert not ops.norm_on_load_2d_ok(pend2, 3, 64)
