"""No GPU: argument refusals of the summing 8 -> 1 head and of atvs_bn_add_plus without the sum, and the shapes of the pipelines'
stage functions when the caller asks for fewer outputs (meta tensors)."""
import ctypes

import pytest
import torch

from atvsnet_amd import _lib

ERR_NULL, ERR_SHAPE, ERR_ARG = -1, -2, -3


def _fake(n=8):
    """Distinct non-null addresses: the refusals return before anything is dereferenced or launched."""
    return [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(n)]


def test_conv3d_8to1_bn2_refuses_bad_arguments():
    L = _lib.lib()
    x0, p0, x1, p1, w, y = _fake(6)
    null = ctypes.c_void_p(0)
    s = ctypes.c_void_p(0)
    f = L.atvs_conv3d_8to1_bn2
    for args in [(null, p0, x1, p1), (x0, null, x1, p1), (x0, p0, null, p1), (x0, p0, x1, null)]:
        assert f(*args, 0, w, y, 1, 4, 4, 4, s) == ERR_NULL
    assert f(x0, p0, x1, p1, 0, null, y, 1, 4, 4, 4, s) == ERR_NULL
    assert f(x0, p0, x1, p1, 0, w, null, 1, 4, 4, 4, s) == ERR_NULL
    assert f(x0, p0, x1, p1, 4, w, y, 1, 4, 4, 4, s) == ERR_ARG
    assert f(x0, p0, x1, p1, -1, w, y, 1, 4, 4, 4, s) == ERR_ARG
    for G, D, H, W in [(0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0)]:
        assert f(x0, p0, x1, p1, 3, w, y, G, D, H, W, s) == ERR_SHAPE
    # 31-bit halo-relative offsets, the plain head's own limit
    assert f(x0, p0, x1, p1, 3, w, y, 1, 1024, 512, 512, s) == ERR_SHAPE
    assert L.atvs_conv3d_8to1(x0, w, y, 1, 1024, 512, 512, s) == ERR_SHAPE


def test_bn_add_plus_takes_a_null_sum_but_not_a_null_plus():
    L = _lib.lib()
    x0, p0, x1, p1, y, base, y2 = _fake(7)
    null = ctypes.c_void_p(0)
    s = ctypes.c_void_p(0)
    f = L.atvs_bn_add_plus
    assert f(x0, p0, x1, p1, null, null, y, base, null, 1, ctypes.c_long(16), 8, 0, s) == ERR_NULL
    assert f(x0, p0, x1, p1, null, null, y, null, y2, 1, ctypes.c_long(16), 8, 0, s) == ERR_NULL
    # y == NULL passes the checks: the shape refusal comes next
    assert f(x0, p0, x1, p1, null, null, null, base, y2, 1, ctypes.c_long(16), 6, 0, s) == ERR_SHAPE


def _meta(*shape):
    return torch.empty(shape, dtype=torch.float32, device='meta')


@pytest.mark.parametrize('H,W,D', [(128, 160, 32), (192, 96, 40)])
def test_stage_functions_return_what_is_asked_for(H, W, D):
    from atvsnet_amd import variables
    from atvsnet_amd.atvsnet import model
    variables.default_store().init_synthetic(1234)
    h, w = H // 4, W // 4
    feats = _meta(3, h, w, 32)
    cams = _meta(1, 3, 2, 4, 4)
    ds, di = _meta(1), _meta(1)
    filt, prob, depth, dview = model.base_stage_batch(feats, cams, D, ds, di, fwd=[1, 2], rev=[1, 2], fwd_prob=False)
    assert prob is None and depth is None and tuple(filt.shape) == (2, D, h, w, 8)
    assert sorted(dview) == [1, 2] and tuple(dview[1].shape) == (1, h, w, 1)
    filt, prob, depth, dview = model.base_stage_batch(feats, cams, D, ds, di, fwd=[1], rev=[2], filtered=False)
    assert filt is None and tuple(prob.shape) == (1, D, h, w) and tuple(depth.shape) == (1, h, w, 1)
    assert sorted(dview) == [2]
    shallow = _meta(3, h, w, 16)
    dviews = {1: _meta(1, h, w, 1), 2: _meta(1, h, w, 1)}
    base = _meta(1, D, h, w, 8)
    c, p, r = model.refinement_batch(_meta(1, h, w, 1), dviews, _meta(1, D, h, w), cams, D, ds, di, [1, 2], shallow,
                                     residual_base=base, cost=False, prob=False)
    assert c is None and p is None and tuple(r.shape) == (2, D, h, w, 8)
    # the head reads the sum: with residual_base and the probability wanted, the residual is formed for it
    c, p, r = model.refinement_batch(_meta(1, h, w, 1), dviews, _meta(1, D, h, w), cams, D, ds, di, [1, 2], shallow,
                                     residual_base=base, cost=False)
    assert c is None and tuple(p.shape) == (2, D, h, w) and tuple(r.shape) == (2, D, h, w, 8)
    c, p = model.refinement_batch(_meta(1, h, w, 1), dviews, _meta(1, D, h, w), cams, D, ds, di, [1, 2], shallow, cost=False)
    assert c is None and tuple(p.shape) == (2, D, h, w)
    c, p = model.refinement_batch(_meta(1, h, w, 1), dviews, _meta(1, D, h, w), cams, D, ds, di, [1, 2], shallow, prob=False)
    assert p is None and tuple(c.shape) == (2, D, h, w, 8)
