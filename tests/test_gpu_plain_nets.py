"""-m gpu: the four networks written in the reference's layer vocabulary only (tests/plain_nets.py) as WHOLE networks on the
MI355X -- the code of cnn_wrapper/network.py a reference-style definition runs: conv_bn / deconv_bn ending in a materialised
batch norm, adds and concats that are formed, the stems and the first convolutions of every stack as launches of their own,
a plain conv_bn handed an ops.SplitVolume.

Reference: oracle/nets.py in float64 (weights .double(), inputs .double(), as tests/golden/make_truth64_golden.py does).
Bars: the project's own of test_gpu_pipeline.py -- 2e-4 * max|ref| + 1e-6 for the tower layers, 1e-3 * max|ref| + 1e-6 for the
U-Net and refinement layers.  The float32 oracle sits 7.0e-6 (tower), 5.9e-6 (U-Net), 6.9e-7 (refinement) of max|ref| from
the float64 one at these shapes (maximum over the layers), i.e. the reference alone is inside the bars by a factor >= 28.

Every case also runs the PRODUCT definition (cnn_wrapper/atvsnet.py) on the same inputs against the same bars -- a red test
then says whether the plain path or both are wrong -- prints max|plain - product| / max|ref|, and counts launches
(ops.watch('*'): the convolutions; ops.launches(): every kind) to prove that the plain definition really ran unfused.

Shapes are the smallest at which these paths can go wrong, not the workload's: images 128 x 160 and 132 x 268 (a 33 x 67
feature map, ragged against every tile; pooled maps 1x2, 2x3, 3x5, 5x9), volumes (8,16,24) (one 1x2x3 cell at 1/8) and
(16,24,40).
"""
import pytest
import torch

from oracle import nets

import plain_nets

pytestmark = pytest.mark.gpu

TOWER_BAR, VOLUME_BAR = 2e-4, 1e-3
TOWER_CHECKED = ('conv1_x', 'conv3_x', 'branch_0', 'branch_1', 'branch_2', 'branch_3', 'fusion0', 'fusion1')
REFINE_CHECKED = ('global_refine_concat', 'global_refine_3dconv6_1')

_ref_cache = {}


def _cached(key, fn):
    """A float64 reference computed once per session and shared (never modified) by the cases that need it."""
    if key not in _ref_cache:
        _ref_cache[key] = fn()
    return _ref_cache[key]


@pytest.fixture(scope='module')
def weights64(weights):
    return {k: v.double() for k, v in weights.items()}


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _run(cls, inputs, G):
    """Build (= run) a network under the launch watch -> (net, convolution launches, launches of every kind)."""
    from atvsnet_amd import ops
    ops.watch('*')
    try:
        net = cls(inputs, is_training=True, independent_samples=G > 1)
        every = ops.launches()
    finally:
        convs = ops.watch(None)
    return net, len(convs), every


class _Tally(object):
    """Worst error / max|ref| per network over the checked layers; asserts every layer against its bar."""

    def __init__(self, bar):
        self.bar, self.worst, self.gap = bar, {'plain': (0.0, None), 'product': (0.0, None)}, (0.0, None)

    def check(self, name, ref, plain, product):
        """ref (G, ...) float64 = the oracle run on each sample alone; plain / product: the layer on the device."""
        plain, product = plain.cpu().double(), product.cpu().double()
        assert tuple(plain.shape) == tuple(ref.shape) == tuple(product.shape), name
        failures = []
        for b in range(ref.shape[0]):
            scale = float(ref[b].abs().max())
            for who, got in (('plain', plain), ('product', product)):
                err = float((got[b] - ref[b]).abs().max())
                if not err <= self.bar * scale + 1e-6:          # (also catches NaN)
                    failures.append('%s %s sample %d: max err %.3e > %.1e * %.3e + 1e-6' % (who, name, b, err, self.bar, scale))
                if scale > 0 and err / scale > self.worst[who][0]:
                    self.worst[who] = (err / scale, name)
            gap = float((plain[b] - product[b]).abs().max())
            if scale > 0 and gap / scale > self.gap[0]:
                self.gap = (gap / scale, name)
        return failures

    def report(self, what, launches):
        (cp, ap), (cq, aq) = launches
        print('%s: plain vs float64 oracle %.2e (%s), product vs oracle %.2e (%s), bar %.0e; max|plain - product| / max|ref| '
              '%.2e (%s); launches plain %d (%d convolutions), product %d (%d convolutions)'
              % (what, self.worst['plain'][0], self.worst['plain'][1], self.worst['product'][0], self.worst['product'][1],
                 self.bar, self.gap[0], self.gap[1], ap, cp, aq, cq))


def _stack(refs, name):
    return torch.cat([r[name] for r in refs])


# ------------------------------------------------------------------------------------------------ the feature towers
def _tower_ref(H, W, i, weights64):
    def make():
        L = {}
        L['out'] = nets.resnet_ds2_spp(_randn(100 + i, 1, H, W, 3).double(), weights64, L)
        return L
    return _cached(('tower', H, W, i), make)


@pytest.mark.parametrize('H,W,G', [(128, 160, 1), (132, 268, 1), (132, 268, 2)])
def test_plain_feature_tower(cuda, weights, weights64, H, W, G):
    from atvsnet_amd.cnn_wrapper.atvsnet import ResNetDS2SPP
    refs = [_tower_ref(H, W, i, weights64) for i in range(G)]
    x = torch.cat([_randn(100 + i, 1, H, W, 3) for i in range(G)]).to(cuda)
    plain, cp, ap = _run(plain_nets.PlainResNetDS2SPP, {'data': x.clone()}, G)
    prod, cq, aq = _run(ResNetDS2SPP, {'data': x.clone()}, G)
    tally, failures = _Tally(TOWER_BAR), []
    for name in TOWER_CHECKED:
        failures += tally.check(name, _stack(refs, name), plain.get_output_by_name(name), prod.get_output_by_name(name))
    failures += tally.check('output', _stack(refs, 'out'), plain.get_output(), prod.get_output())
    tally.report('tower %dx%d G=%d' % (H, W, G), ((cp, ap), (cq, aq)))
    assert not failures, '\n'.join(failures)
    # the concat really is the concat of the network's own six parts (a dense copy here, slices written in place there)
    for net in (plain, prod):
        parts = [net.get_output_by_name(n) for n in ('conv1_x', 'conv3_x', 'branch_0', 'branch_1', 'branch_2', 'branch_3')]
        cat = net.get_output_by_name('concat_feature')
        assert tuple(cat.shape) == (G, H // 4, W // 4, 320)
        assert torch.equal(cat, torch.cat(parts, -1))
    assert plain.get_output() is plain.layers['fusion1']
    # unfused: the same convolutions (the tower's extensions fuse glue only: batch norms applied on load, a concat that is never
    # copied), strictly more launches
    assert cp >= cq and ap > aq, ((cp, ap), (cq, aq))


def _shallow_ref(H, W, i, weights64):
    return _cached(('shallow', H, W, i),
                   lambda: nets.resnet_ds2_spp_shallow_f16(_randn(200 + i, 1, H, W, 3).double(), weights64))


@pytest.mark.parametrize('H,W,G', [(128, 160, 1), (132, 268, 1), (132, 268, 2)])
def test_plain_shallow_tower(cuda, weights, weights64, H, W, G):
    from atvsnet_amd.cnn_wrapper.atvsnet import ResNetDS2SPP_shallow_f16
    ref = torch.cat([_shallow_ref(H, W, i, weights64) for i in range(G)])
    x = torch.cat([_randn(200 + i, 1, H, W, 3) for i in range(G)]).to(cuda)
    plain, cp, ap = _run(plain_nets.PlainResNetDS2SPP_shallow_f16, {'data': x.clone()}, G)
    prod, cq, aq = _run(ResNetDS2SPP_shallow_f16, {'data': x.clone()}, G)
    tally = _Tally(TOWER_BAR)
    failures = tally.check('output', ref, plain.get_output(), prod.get_output())
    tally.report('shallow tower %dx%d G=%d' % (H, W, G), ((cp, ap), (cq, aq)))
    assert not failures, '\n'.join(failures)
    # the product's definition of this network uses no extension: the two are one path, launch for launch
    assert (cp, ap) == (cq, aq) and torch.equal(plain.get_output(), prod.get_output())


# ------------------------------------------------------------------------------------------------ the regulariser
def _unet_ref(key, data64, weights64):
    def make():
        L = {}
        out, _ = nets.stacked_unet_prob(data64(), weights64, L)
        del L['data']
        L['out'] = out
        return L
    return _cached(('unet',) + key, make)


@pytest.mark.parametrize('form', ['dense', 'two_samples', 'split'])
@pytest.mark.parametrize('D,h,w', [(8, 16, 24), (16, 24, 40)])
def test_plain_stacked_unet(cuda, weights, weights64, D, h, w, form):
    """form: dense -- data (1,D,h,w,64); two_samples -- (2,D,h,w,64) with independent_samples=True, each sample against the
    oracle run on it alone; split -- data as the ops.SplitVolume model.build_cost_volume(lazy=True) makes (var (D,h,w,32),
    const (h,w,32), channels [const | var]), against the oracle on its materialised form."""
    from atvsnet_amd import ops
    from atvsnet_amd.cnn_wrapper.atvsnet import StackedUNet_prob
    if form == 'split':
        G = 1
        var, const = _randn(31, D, h, w, 32).to(cuda), _randn(32, h, w, 32).to(cuda)
        data = lambda: ops.SplitVolume(var, const, [('c', i) for i in range(32)] + [('v', i) for i in range(32)])   # noqa: E731
        dense = data().materialize()
        assert tuple(dense.shape) == (1, D, h, w, 64)
        assert torch.equal(dense[0, ..., 32:], var) and torch.equal(dense[0, 0, ..., :32], const) \
            and torch.equal(dense[0, D - 1, ..., :32], const)
        refs = [_unet_ref((D, h, w, 'split'), lambda: dense.cpu().double(), weights64)]
    else:
        G = 2 if form == 'two_samples' else 1
        sample = lambda i: _randn(300 + i, 1, D, h, w, 64)                                                          # noqa: E731
        refs = [_unet_ref((D, h, w, i), (lambda i=i: sample(i).double()), weights64) for i in range(G)]
        x = torch.cat([sample(i) for i in range(G)]).to(cuda)
        data = lambda: x.clone()                                                                                    # noqa: E731
    plain, cp, ap = _run(plain_nets.PlainStackedUNet_prob, {'data': data()}, G)
    prod, cq, aq = _run(StackedUNet_prob, {'data': data()}, G)
    tally, failures = _Tally(VOLUME_BAR), []
    assert set(refs[0]) == set(plain_nets.UNET_LAYERS) | {'out'}
    for name in refs[0]:
        if name == 'out':
            failures += tally.check('output', _stack(refs, name), plain.get_output(), prod.get_output())
        else:
            failures += tally.check(name, _stack(refs, name), plain.get_output_by_name(name), prod.get_output_by_name(name))
    tally.report('U-Net (%d,%d,%d) %s' % (D, h, w, form), ((cp, ap), (cq, aq)))
    assert not failures, '\n'.join(failures)
    # unfused: two launches where the product issues the siblings as one (every stack), formed adds, materialised batch norms
    assert cp > cq and ap > aq, ((cp, ap), (cq, aq))


# ------------------------------------------------------------------------------------------------ the refinement
def _refine_ref(dense64, weights64):
    L = {}
    L['out'], _ = nets.cost_vol_refine_net(*dense64, weights64, L)
    return L


@pytest.mark.parametrize('form', ['dense', 'split_two_samples'])
@pytest.mark.parametrize('D,h,w', [(8, 16, 24), (16, 24, 40)])
def test_plain_refinement(cuda, weights, weights64, D, h, w, form):
    """form: dense -- photo / geo / prob / hull with 48 / 19 / 1 / 1 channels; split_two_samples -- G = 2 with
    independent_samples=True, photo_group and geo_group as the ops.SplitVolumes model._refine_net builds for chan = 16 (photo:
    16 D-varying + 32 tiled channels; geo: [v0 | v1 sixteen times | c0 | c1] = 19 channels), each sample against the oracle on
    its materialised inputs alone."""
    from atvsnet_amd import ops
    from atvsnet_amd.cnn_wrapper.atvsnet import CostVolRefineNet
    chan = 16
    G = 2 if form == 'split_two_samples' else 1
    prob = torch.rand(G, D, h, w, 1, generator=torch.Generator().manual_seed(41)).to(cuda)
    hull = (torch.rand(G, D, h, w, 1, generator=torch.Generator().manual_seed(42)) > 0.4).float().to(cuda)
    if form == 'dense':
        photo_d, geo_d = _randn(43, G, D, h, w, 3 * chan).to(cuda), _randn(44, G, D, h, w, chan + 3).to(cuda)
        inputs = lambda: {'photo_group': photo_d.clone(), 'geo_group': geo_d.clone(), 'prob_vol': prob.clone(),    # noqa: E731
                          'vis_hull': hull.clone()}
    else:
        pv, pc = _randn(45, G, D, h, w, chan).to(cuda), _randn(46, G, h, w, 2 * chan).to(cuda)
        gv, gc = _randn(47, G, D, h, w, 2).to(cuda), _randn(48, G, h, w, 2).to(cuda)
        pmap = [('v', i) for i in range(chan)] + [('c', i) for i in range(2 * chan)]
        gmap = [('v', 0)] + [('v', 1)] * chan + [('c', 0), ('c', 1)]
        inputs = lambda: {'photo_group': ops.SplitVolume(pv, pc, pmap), 'geo_group': ops.SplitVolume(gv, gc, gmap),   # noqa: E731
                          'prob_vol': prob.clone(), 'vis_hull': hull.clone()}
        photo_d, geo_d = (inputs()[k].materialize() for k in ('photo_group', 'geo_group'))
        assert tuple(photo_d.shape) == (G, D, h, w, 48) and tuple(geo_d.shape) == (G, D, h, w, 19)
        assert torch.equal(geo_d[..., 1:17], gv[..., 1:2].expand(G, D, h, w, chan))         # the 16-fold replicated channel
        assert torch.equal(geo_d[..., 0], gv[..., 0]) and torch.equal(geo_d[:, D - 1, ..., 17:], gc)
        assert torch.equal(photo_d[..., :chan], pv) and torch.equal(photo_d[:, 0, ..., chan:], pc)
    refs = [_refine_ref([t[b:b + 1].cpu().double() for t in (photo_d, geo_d, prob, hull)], weights64) for b in range(G)]
    plain, cp, ap = _run(plain_nets.PlainCostVolRefineNet, inputs(), G)
    prod, cq, aq = _run(CostVolRefineNet, inputs(), G)
    tally, failures = _Tally(VOLUME_BAR), []
    for name in REFINE_CHECKED:
        failures += tally.check(name, _stack(refs, name), plain.get_output_by_name(name), prod.get_output_by_name(name))
    failures += tally.check('output', _stack(refs, 'out'), plain.get_output(), prod.get_output())
    tally.report('refinement (%d,%d,%d) %s' % (D, h, w, form), ((cp, ap), (cq, aq)))
    assert not failures, '\n'.join(failures)
    # unfused: four stems and two first convolutions as launches of their own
    assert cp > cq and ap > aq, ((cp, ap), (cq, aq))
