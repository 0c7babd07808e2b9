"""CPU: tests/plain_nets.py -- the networks in the reference's layer vocabulary -- on meta tensors (the host code of
cnn_wrapper/network.py without launches; needs the built library, like test_host_api.py).

* the file keeps to the reference's calls and keyword arguments (parsed, not trusted);
* every layer of SURVEY.md Appendix A exists in the plain and in the product network, with equal shapes, and the plain
  network's layers are dense tensors (nothing pending, nothing split);
* each plain network touches exactly the variables (names and shapes) its product counterpart touches.
"""
import ast
import os

import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import ops, variables
from atvsnet_amd.cnn_wrapper import atvsnet as product

import plain_nets

ALLOWED_CALLS = {'feed', 'conv', 'conv_bn', 'deconv_bn', 'add', 'concat', 'res_block', 'avg_pool', 'image_resize',
                 'get_shape_by_name'}
ALLOWED_KEYWORDS = {'kernel_size', 'filters', 'strides', 'name', 'relu', 'center', 'padding', 'biased', 'rate', 'num_block',
                    'stride', 'size', 'method', 'align_corners', 'axis', 'pool_size'}
ALLOWED_FUNCTIONS = {'range', 'enumerate'}           # plain functions the definitions may call (loops over stacks / branches)
CLASSES = {'PlainResNetDS2SPP', 'PlainResNetDS2SPP_shallow_f16', 'PlainStackedUNet_prob', 'PlainCostVolRefineNet'}


def meta(*shape):
    return torch.empty(shape, dtype=torch.float32, device='meta')


def _vocabulary_faults(source):
    """Everything in `source` that leaves the reference's vocabulary, as a list of strings."""
    tree = ast.parse(source)
    bad = []
    for node in ast.walk(tree):
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            names = [a.name for a in node.names]
            if not (isinstance(node, ast.ImportFrom) and node.module == 'atvsnet_amd.cnn_wrapper.network'
                    and names == ['Network']):
                bad.append('line %d: import of %s' % (node.lineno, names))
        elif isinstance(node, ast.ClassDef):
            if [getattr(b, 'id', None) for b in node.bases] != ['Network']:
                bad.append('line %d: class %s does not derive from Network alone' % (node.lineno, node.name))
            for item in node.body:
                if isinstance(item, ast.FunctionDef) and item.name != 'setup':
                    bad.append('line %d: %s.%s (only setup may be defined)' % (item.lineno, node.name, item.name))
        elif isinstance(node, ast.Call):
            f = node.func
            if isinstance(f, ast.Attribute):
                # a call on `self` or on a chained result (feed(...).conv_bn(...)); any other receiver is refused too: the file
                # needs none, and `ops.anything(...)` or `net.refine_stems(...)` must not slip through
                on_self = isinstance(f.value, ast.Name) and f.value.id == 'self'
                chained = isinstance(f.value, ast.Call)
                if not (on_self or chained) or f.attr not in ALLOWED_CALLS:
                    bad.append('line %d: call of .%s' % (node.lineno, f.attr))
            elif isinstance(f, ast.Name):
                if f.id not in ALLOWED_FUNCTIONS:
                    bad.append('line %d: call of %s()' % (node.lineno, f.id))
            else:
                bad.append('line %d: call of a computed function' % node.lineno)
            for kw in node.keywords:
                if kw.arg not in ALLOWED_KEYWORDS:          # kw.arg is None for **mapping
                    bad.append('line %d: keyword %s' % (node.lineno, kw.arg))
    return bad


def test_plain_nets_keep_to_the_reference_vocabulary():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'plain_nets.py')
    with open(path) as fh:
        source = fh.read()
    assert _vocabulary_faults(source) == []
    classes = {n.name for n in ast.parse(source).body if isinstance(n, ast.ClassDef)}
    assert classes == CLASSES
    # the guard itself: each of the product's extensions is caught
    for line in ("self.feed('a').conv_bn(3, 8, 1, name='b', defer_bn=True)",
                 "self.feed('a').conv_bn_siblings(dict(name='b'), dict(name='c'))",
                 "self.refine_stems('c', [])",
                 "self.concat_buffer('c', self.layers['a'], 32)",
                 "self.feed('a').image_resize(size=(2, 2), name='b', out_slice=('c', 0))",
                 "self.feed('a', 'b').add(name='c', defer=True)",
                 "self.feed('a', 'b').add(name='c', plus='d', keep_sum=False)",
                 "self.feed('a').conv_bn(3, 8, 1, **extra)",
                 "getattr(self, 'refine_stems')('c', [])",
                 "ops.conv(x, 'k', w)",
                 "import atvsnet_amd.ops"):
        assert _vocabulary_faults(line), line


def _pairs(H, W, D, G=1):
    """(plain class, product class, inputs, Appendix-A layer names) of the four networks at one size, dense meta inputs."""
    h, w = H // 4, W // 4
    vol = lambda c: meta(G, D, h, w, c)                                # noqa: E731
    return [
        (plain_nets.PlainResNetDS2SPP, product.ResNetDS2SPP, {'data': meta(G, H, W, 3)}, plain_nets.TOWER_LAYERS),
        (plain_nets.PlainResNetDS2SPP_shallow_f16, product.ResNetDS2SPP_shallow_f16, {'data': meta(G, H, W, 3)},
         plain_nets.SHALLOW_LAYERS),
        (plain_nets.PlainStackedUNet_prob, product.StackedUNet_prob, {'data': vol(64)}, plain_nets.UNET_LAYERS),
        (plain_nets.PlainCostVolRefineNet, product.CostVolRefineNet,
         {'photo_group': vol(48), 'geo_group': vol(19), 'prob_vol': vol(1), 'vis_hull': vol(1)}, plain_nets.REFINE_LAYERS),
    ]


@pytest.mark.parametrize('H,W,D', [(128, 160, 32), (512, 640, 192), (480, 928, 256), (132, 268, 32)])
def test_plain_and_product_layers_have_equal_shapes(H, W, D):
    """The three sizes of test_shapes_of_every_network, and the ragged tower size 132 x 268 (33 x 67 features: the towers only --
    the 3-level U-Nets take volumes whose sides are multiples of 8)."""
    cases = _pairs(H, W, D)
    if H % 32 or W % 32:
        cases = cases[:2]
    for plain_cls, product_cls, inputs, names in cases:
        p = plain_cls(dict(inputs), is_training=True)
        q = product_cls(dict(inputs), is_training=True)
        for name in names:
            assert name in p.layers, (plain_cls.__name__, name)
            assert name in q.layers, (product_cls.__name__, name)
            assert p.get_shape_by_name(name) == q.get_shape_by_name(name), name
            assert tuple(p.get_output_by_name(name).shape) == tuple(q.get_output_by_name(name).shape), name
        assert tuple(p.get_output().shape) == tuple(q.get_output().shape)
        # dense inputs -> every layer of the plain network is a formed, dense tensor
        for name, t in p.layers.items():
            assert isinstance(t, torch.Tensor), (plain_cls.__name__, name, type(t))
            assert not isinstance(t, ops.LAZY + (ops.SplitVolume,)), name


def test_plain_networks_also_take_independent_samples_on_the_host():
    for plain_cls, product_cls, inputs, names in _pairs(128, 160, 32, G=2):
        with pytest.raises(ValueError, match='batch size must be 1'):
            plain_cls(dict(inputs), is_training=True)
        p = plain_cls(dict(inputs), is_training=True, independent_samples=True)
        q = product_cls(dict(inputs), is_training=True, independent_samples=True)
        for name in names:
            assert p.get_shape_by_name(name) == q.get_shape_by_name(name) and p.get_shape_by_name(name)[0] == 2, name


def test_plain_networks_touch_the_variables_of_their_product_counterparts():
    store = variables.default_store()
    saved = dict(store.host)
    store.clear()
    try:
        seen_all = {}
        for plain_cls, product_cls, inputs, _ in _pairs(128, 160, 32):
            touched = []
            for cls in (plain_cls, product_cls):
                store.clear()
                cls(dict(inputs), is_training=True)
                touched.append({k: tuple(v.shape) for k, v in store.host.items()})
            assert touched[0], plain_cls.__name__
            assert set(touched[0]) == set(touched[1]), (plain_cls.__name__, set(touched[0]) ^ set(touched[1]))
            assert touched[0] == touched[1], plain_cls.__name__
            seen_all.update(touched[0])
        # ... and all of them are rows of the variable table
        spec = dict(variables.variable_specs())
        assert set(seen_all) <= set(spec)
        assert all(seen_all[k] == tuple(spec[k]) for k in seen_all)
    finally:
        store.clear()
        store.host.update(saved)
