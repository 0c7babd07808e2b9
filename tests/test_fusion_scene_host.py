"""CPU: the host side of the in-run scene fusion (depth_fusion.SceneFusion, ops.fusion_stage / ops.fusibile_scene) -- the camera rows
it derives in memory against the files of the two-step pipeline, the camera order, and argument validation before any launch."""
import os

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import depth_fusion as DF
from atvsnet_amd.atvsnet import preprocess as P


def _cam(seed):
    """A (2,4,4) float32 camera as eval_pointcloud holds it: values whose float32 str() is not their float64 cast (0.1f prints as
    '0.1', its float64 value is 0.10000000149011612)."""
    rng = np.random.default_rng(seed)
    ang = 0.1 + 0.05 * seed
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0, :3, :3] = R
    cam[0, :3, 3] = rng.uniform(-1, 1, 3)
    cam[0, 3, 3] = 1
    cam[1, :3, :3] = [[0.1 * 583 + seed, 0, 55.3], [0, 58.31, 30.7], [0, 0, 1]]
    cam[1, 3] = (0.1, 0.0123, 16, 2.3)
    return cam


def test_camera_rows_are_those_of_the_gipuma_files(tmp_path):
    """write_cam (as _write_map calls it) -> atvsnet_to_gipuma -> read_p_file -> pack_cameras, against camera_row, bitwise."""
    from PIL import Image
    dense = str(tmp_path)
    depth_folder = os.path.join(dense, 'depths_atvsnet')
    os.makedirs(depth_folder)
    cams = [_cam(i) for i in range(3)]
    for i, cam in enumerate(cams):
        stem = os.path.join(depth_folder, '%08d' % i)
        P.write_cam(stem + '.txt', cam)
        Image.fromarray(np.zeros((4, 5, 3), np.uint8)).save(stem + '.jpg')
        P.write_pfm(stem + '_prob_filtered.pfm', np.ones((4, 5), np.float32))
    point_folder = os.path.join(dense, 'points_atvsnet')
    DF.atvsnet_to_gipuma(dense, point_folder)
    for i, cam in enumerate(cams):
        want = DF.pack_cameras([DF.read_p_file(os.path.join(point_folder, 'cams', '%08d.jpg.P' % i))])[0]
        got = DF.camera_row(cam)
        assert got.dtype == np.float32 and got.shape == (28,)
        assert got.tobytes() == want.tobytes(), i
        # the case bites: the .P file holds other float64 values than the float64 cast of the float32 camera would give
        p_file = DF.read_p_file(os.path.join(point_folder, 'cams', '%08d.jpg.P' % i))
        assert not np.array_equal(p_file, DF.projection_matrix(cam.astype(np.float64)))


def test_cam_text_is_write_cams_bytes(tmp_path):
    cam = _cam(4)
    path = str(tmp_path / 'c.txt')
    P.write_cam(path, cam)
    with open(path) as f:
        assert f.read() == P.cam_text(cam)


def _maps(rows, cols, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.1, 1, (1, rows, cols, 1)).astype(np.float32), rng.uniform(0, 1, (1, rows, cols, 1)).astype(np.float32),
            rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8))


def test_out_of_order_adds_fuse_in_out_index_order():
    """Cameras are fused by out_index ascending (depth_map_fusion's sorted 2333__%08d folders), not in submission order."""
    f = DF.SceneFusion(4, 6, 7, device='meta')
    order = [3, 0, 7, 2]
    for k in order:
        d, p, img = _maps(6, 7, k)
        f.add(k, d, p, img, _cam(k))
    got = f.cams[f.order()]
    want = np.stack([DF.camera_row(_cam(k)) for k in sorted(order)])
    assert np.array_equal(got, want)
    assert [f.index[s] for s in f.order()] == sorted(order)


def test_scene_fusion_rejects_bad_arguments():
    with pytest.raises(RuntimeError):
        DF.SceneFusion(2, 6, 7, device='cpu')                    # no CPU fallback
    with pytest.raises(ValueError):
        DF.SceneFusion(0, 6, 7, device='meta')
    f = DF.SceneFusion(2, 6, 7, device='meta')
    d, p, img = _maps(6, 7)
    d2, p2, img2 = _maps(8, 7)
    with pytest.raises(RuntimeError):                            # ragged maps: depth_map_fusion's kind of error
        f.add(0, d2, p2, img2, _cam(0))
    with pytest.raises(RuntimeError):
        f.add(0, d, p, img2, _cam(0))                            # image of another size than the maps
    with pytest.raises(RuntimeError):
        f.add(0, d, p2, img, _cam(0))
    with pytest.raises(TypeError):
        f.add(0, d.astype(np.float64), p, img, _cam(0))
    with pytest.raises(TypeError):
        f.add(0, d, p, img.astype(np.float32), _cam(0))
    assert f.index == []                                         # nothing was staged
    f.add(5, d, p, img, _cam(0))
    with pytest.raises(ValueError):
        f.add(5, d, p, img, _cam(0))                             # the same map twice
    f.add(1, d, p, img, _cam(1))
    with pytest.raises(ValueError):
        f.add(2, d, p, img, _cam(2))                             # more maps than slots
    assert f.index == [5, 1]


@pytest.fixture
def no_launch(monkeypatch):
    from atvsnet_amd.ops import aanet
    calls = []
    monkeypatch.setattr(aanet, '_call', lambda *a: calls.append(a))
    yield calls
    assert calls == [], 'a launch was issued'


def test_ops_fusion_stage_validates_before_launch(no_launch):
    r, c = 6, 7
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32)        # noqa: E731
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)           # noqa: E731
    good = dict(depth=f32(r, c), prob=f32(r, c), bgr=u8(r, c, 3), nd_out=f32(r, c, 4), img_out=f32(r, c, 4))
    call = lambda **kw: ops.fusion_stage(kw['depth'], kw['prob'], kw['bgr'], True, 0.8, kw['nd_out'], kw['img_out'])  # noqa: E731
    with pytest.raises(RuntimeError):
        call(**good)                                             # CPU tensors: no fallback
    for name, bad, exc in [('depth', f32(r, c).double(), TypeError), ('prob', f32(r, c + 1), ValueError),
                           ('bgr', f32(r, c, 3), TypeError), ('bgr', u8(r, c, 4), ValueError),
                           ('nd_out', f32(r, c, 3), ValueError), ('img_out', f32(c, r, 4).transpose(0, 1), ValueError),
                           ('depth', f32(1, r, c), ValueError)]:
        kw = dict(good, **{name: bad})
        with pytest.raises(exc):
            call(**kw)
    meta = {k: v.to('meta') for k, v in good.items()}
    call(**meta)                                                 # meta: shapes only, no launch
    with pytest.raises(RuntimeError):
        call(**dict(meta, prob=good['prob']))                    # meta mixed with another device


def test_ops_fusibile_scene_validates_before_launch(no_launch):
    n, r, c = 3, 6, 7
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32)        # noqa: E731
    good = dict(cams=f32(n, 28), nd=f32(n, r, c, 4), img=f32(n, r, c, 4))
    call = lambda **kw: ops.fusibile_scene(kw['cams'], kw['nd'], kw['img'], 0.01, 6.28, 2)      # noqa: E731
    with pytest.raises(RuntimeError):
        call(**good)
    for name, bad, exc in [('cams', f32(n, 27), ValueError), ('cams', f32(n + 1, 28), ValueError),
                           ('nd', f32(n, r, c, 4).double(), TypeError), ('img', f32(n, r, c + 1, 4), ValueError),
                           ('img', torch.zeros((n, r, c, 4), dtype=torch.uint8), TypeError), ('nd', f32(r, c, 4), ValueError)]:
        with pytest.raises(exc):
            call(**dict(good, **{name: bad}))
    with pytest.raises(RuntimeError):
        call(**{k: v.to('meta') for k, v in good.items()})       # the count needs a launch


def test_ops_fusibile_validates_before_launch(no_launch):
    n, r, c = 3, 6, 7
    call = lambda **kw: ops.fusibile(kw['cams'], kw['nd'], kw['img'], kw['ref'], 0.01, 6.28, 2)      # noqa: E731
    goods = {}
    for dev in ('cpu', 'meta'):                                  # refused on any device, before the device is looked at
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)        # noqa: E731
        u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)           # noqa: E731
        good = goods[dev] = dict(cams=f32(n, 28), nd=f32(n, r, c, 4), img=f32(n, r, c, 4), ref=1)
        for name, bad, exc in [('cams', f32(n, 27), ValueError), ('cams', f32(n + 1, 28), ValueError), ('cams', f32(n * 28), ValueError),
                               ('img', f32(n - 1, r, c, 4), ValueError), ('img', f32(n + 1, r, c, 4), ValueError),
                               ('img', f32(n, r, c + 1, 4), ValueError), ('img', f32(n, r, c, 3), ValueError),
                               ('nd', f32(r, c, 4), ValueError), ('nd', f32(n, r, c, 3), ValueError),
                               ('nd', f32(n, c, r, 4).transpose(1, 2), ValueError),
                               ('img', f32(n, r, c, 8)[..., ::2], ValueError), ('cams', f32(n, 56)[:, ::2], ValueError),
                               ('nd', f32(n, r, c, 4).double(), TypeError), ('img', f32(n, r, c, 4).double(), TypeError),
                               ('cams', f32(n, 28).double(), TypeError), ('nd', u8(n, r, c, 4), TypeError),
                               ('img', u8(n, r, c, 4), TypeError), ('nd', np.zeros((n, r, c, 4), np.float32), ValueError),
                               ('ref', -1, ValueError), ('ref', n, ValueError)]:
            if torch.is_tensor(bad) and name in ('nd', 'img', 'cams') and bad.dim() in (2, 4) and bad.dtype == torch.float32 \
                    and tuple(bad.shape) == tuple(good[name].shape):
                assert not bad.is_contiguous()
            with pytest.raises(exc):
                call(**dict(good, **{name: bad}))
    with pytest.raises(RuntimeError):
        call(**goods['cpu'])                                     # CPU tensors: no fallback
    meta = goods['meta']
    coord, normal, tex, created = call(**meta)                   # meta: shapes only, no launch
    assert all(t.device.type == 'meta' and t.dtype == torch.float32 for t in (coord, normal, tex, created))
    assert tuple(coord.shape) == tuple(normal.shape) == tuple(tex.shape) == (r, c, 4) and tuple(created.shape) == (r, c)
    with pytest.raises(RuntimeError):
        call(**dict(meta, cams=goods['cpu']['cams']))            # meta mixed with another device
