"""Scene mode on the host (no GPU): the view preparation's integer resize formula on the host taps, the scene cache (key, LRU by bytes,
weight invalidation), missing-source substitution, the driver's host camera path, and the --eager --scene_cache refusal."""
import os

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS, ops, variables
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import preprocess as P
from atvsnet_amd.atvsnet import scene as S


@pytest.fixture
def flags():
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


def _crop_ref(img, max_h, max_w):
    """scale_image + crop_mvs_input of one view, as load_data does it."""
    old = (FLAGS.view_num, FLAGS.max_h, FLAGS.max_w)
    FLAGS.view_num, FLAGS.max_h, FLAGS.max_w = 1, max_h, max_w
    try:
        cams = [np.zeros((2, 4, 4))]
        out, _ = P.crop_mvs_input([img], cams, base_image_size=32)
        return out[0]
    finally:
        FLAGS.view_num, FLAGS.max_h, FLAGS.max_w = old


def test_host_taps_and_the_kernel_formula_are_scale_image(flags):
    """~50 random (size, scale, crop): the kernel's integer formula on the host taps (only the rows / columns of the crop window)
    equals scale_image + crop_mvs_input, and its 1/4 image scale_image(cropped, 0.25)."""
    rng = np.random.default_rng(7)
    checked = 0
    for case in range(60):
        h, w = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        scale = float(rng.choice([1.0, 0.98, 0.5, 0.25, rng.uniform(0.2, 1.0)]))
        if min(int(np.rint(h * scale)), int(np.rint(w * scale))) < 1:
            continue
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        H, W = P.scaled_size(h, w, scale)
        if min(H, W) < 2:
            continue
        # a window inside the resized image, as the driver's adaptive scale guarantees (a crop on both axes; down to one row)
        max_h, max_w = int(rng.integers(1, H)), int(rng.integers(1, W))
        FLAGS.max_h, FLAGS.max_w = max_h, max_w
        crop = P.crop_window(H, W)
        want = _crop_ref(P.scale_image(img, scale), max_h, max_w)
        assert want.shape[:2] == (crop[2], crop[3])
        checked += 1
        (my, mx), quarter = ops.prepare_taps(h, w, scale, crop)
        got = ops.resize_u8_host(img, my, mx)
        assert np.array_equal(got, want), (case, h, w, scale, crop)
        if min(int(np.rint(want.shape[0] * 0.25)), int(np.rint(want.shape[1] * 0.25))) >= 1:
            qy, qx = quarter
            assert np.array_equal(ops.resize_u8_host(got, qy, qx), P.scale_image(want, 0.25)), (case, h, w, scale)
    assert checked >= 40


def test_scale_image_is_unchanged_by_the_shared_taps():
    """resize_taps_u8 is the weight rule scale_image always had: rint((1 - t) * 2048), rint(t * 2048) of float32 t."""
    left, right, a0, a1 = P.resize_taps_u8(37, 50, 50 / 37.)
    _, _, frac = P._resize_taps(37, 50, 50 / 37.)
    assert np.array_equal(a1, np.rint(frac * 2048).astype(np.int64))
    assert np.array_equal(a0, np.rint((1.0 - frac) * 2048).astype(np.int64))
    assert ((a0 + a1) == 2048).all() and left.min() >= 0 and right.max() <= 49


def test_cache_key_and_lru_eviction_by_bytes():
    k = S.view_key('a.jpg', 0.98, (1, 2, 480, 896))
    assert k == ('a.jpg', 0.98, (1, 2, 480, 896))
    assert S.view_key('a.jpg', 0.98, (1, 2, 480, 896)) != S.view_key('a.jpg', 0.5, (1, 2, 480, 896))
    t = torch.empty((10, 10), dtype=torch.float32, device='meta')
    assert S.tensor_bytes(t, t) == 800
    c = S.ViewCache(max_bytes=1000)
    c.put('a', 1, 400)
    c.put('b', 2, 400)
    assert c.get('a') == 1                 # a is now the most recent
    c.put('c', 3, 400)                     # over the bound: the least recently used (b) goes
    assert 'b' not in c and 'a' in c and 'c' in c and c.bytes == 800 and c.evictions == 1
    c.put('d', 4, 5000)                    # alone above the bound: kept, everything else evicted
    assert list(c.items) == ['d'] and c.bytes == 5000
    c.drop('d')
    assert len(c) == 0 and c.bytes == 0


def test_cache_is_cleared_when_the_weights_change():
    store = variables.default_store()
    c = S.ViewCache(1 << 20)
    c.check_generation(store.generation)
    c.put('a', 1, 10)
    assert not c.check_generation(store.generation) and 'a' in c
    name = 'conv0_0/weights'
    saved = store.host.get(name)
    store.set(name, np.zeros((3, 3, 3, 8), np.float32) if saved is None else saved)
    try:
        assert c.check_generation(store.generation) and len(c) == 0
    finally:
        if saved is None:
            store.host.pop(name, None)


def test_missing_sources_are_the_reference():
    assert S.pad_views(['r', 's1'], 4) == ['r', 's1', 'r', 'r']
    assert S.pad_views(['r', 's1', 's2', 's3', 's4'], 3) == ['r', 's1', 's2']


def test_adaptive_scale_is_load_datas(flags):
    FLAGS.max_h, FLAGS.max_w = 480, 896
    assert S.adaptive_scale([(490, 940), (600, 1000)]) == max(480 / 490., 896 / 940.)
    assert S.adaptive_scale([(400, 940)]) is None
    FLAGS.adaptive_scaling = False
    assert S.adaptive_scale([(400, 940)]) == 1


def _write_cams(root, n, rng):
    os.makedirs(os.path.join(root, 'cams'))
    paths = []
    for v in range(n):
        cam = np.zeros((2, 4, 4))
        cam[0] = np.eye(4)
        cam[0, 0, 3] = 0.1 * v
        cam[1, :3, :3] = [[300.0, 0, 150], [0, 300.0, 90], [0, 0, 1]]
        cam[1, 3] = (2.0, 0.05, 0, 0.0)
        p = os.path.join(root, 'cams', '%08d_cam.txt' % v)
        P.write_cam(p, cam)
        paths.append(p)
    return paths


def test_load_cams_matches_load_data(flags, tmp_path):
    """The scene driver's host camera path writes the cameras load_data forms (two image sizes, a missing source)."""
    from PIL import Image
    rng = np.random.default_rng(3)
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'images'))
    cams = _write_cams(root, 3, rng)
    sizes = [(150, 190), (170, 200), (150, 190)]
    imgs = []
    for v, (h, w) in enumerate(sizes):
        p = os.path.join(root, 'images', '%08d.jpg' % v)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        imgs.append(p)
    FLAGS.view_num, FLAGS.max_h, FLAGS.max_w, FLAGS.max_d = 4, 128, 160, 16
    data = [imgs[0], cams[0], imgs[1], cams[1], imgs[2], cams[2]]          # 3 of 4 views: the last is the reference
    want = E.load_data([data], 0)[2]
    shapes = [E._Decoder.shape(imgs[v if v < 3 else 0]) for v in range(4)]
    got, scale = E.load_cams(data, shapes)
    assert np.array_equal(got, want)
    assert scale == S.adaptive_scale(shapes)


def test_eager_and_scene_cache_are_refused(flags, capsys):
    with pytest.raises(SystemExit):
        E.cli(['--eager', '--scene_cache', '--synthetic_weights', '--scenes', 'none'])
    assert '--scene_cache' in capsys.readouterr().err
