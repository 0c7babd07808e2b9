"""Undistortion, host side (no GPU): the forward models and their Newton inverse, the output camera against the test's own
restatement (tests/undistort_restated.py), read_model(allow_distorted), the command line's two input forms, the argument checks
in front of the kernels and the library's new entry points."""
import ctypes
import os

import numpy as np
import pytest

import atvsnet_amd  # noqa: F401
from atvsnet_amd import _lib, ops
from atvsnet_amd.atvsnet import colmap, colmap_scene
from atvsnet_amd.atvsnet import undistort as U

import undistort_restated as R
from colmap_model import write_binary, write_text

_W, _H = 301, 203
_DISTORTED = sorted(R.NPARAMS)
_PINHOLES = {'PINHOLE': (240.0, 242.0, 150.4, 100.9), 'SIMPLE_PINHOLE': (240.0, 150.4, 100.9)}


def _params(model, strength=1.0):
    return _PINHOLES[model] if model in _PINHOLES else R.test_camera(model, _W, _H, strength)


@pytest.mark.parametrize('model', _DISTORTED + sorted(_PINHOLES))
def test_undistort_then_distort_returns_the_start(model):
    """A grid of pixels inside the image, as distorted rays: the inverse's forward image is the start to 1e-9 (normalised units)."""
    p = _params(model, 1.8)
    (fx, fy, cx, cy), _ = U.split_params(model, p)
    ys, xs = np.meshgrid(np.linspace(0.5, _H - 0.5, 23), np.linspace(0.5, _W - 0.5, 31), indexing='ij')
    ud, vd = (xs - cx) / fx, (ys - cy) / fy
    u, v = U.undistort_points(model, p, ud, vd)
    assert u.shape == ud.shape
    bu, bv = U.distort(model, p, u, v)
    assert max(np.abs(bu - ud).max(), np.abs(bv - vd).max()) <= 1e-9
    if model not in _PINHOLES:
        assert np.abs(u - ud).max() > 1e-3                               # the cameras do distort
        ru, rv = R.forward(model, p, u, v)                               # and the product's forward model is the restatement's
        assert np.array_equal(ru, bu) and np.array_equal(rv, bv)


@pytest.mark.parametrize('b', [0.0, 0.5, 1.0])
@pytest.mark.parametrize('model', _DISTORTED)
def test_undistorted_camera_is_the_restatement(model, b):
    for size, strength in (((_W, _H), 1.0), ((67, 45), 1.8)):
        p = R.test_camera(model, size[0], size[1], strength)
        want = R.output_camera(model, p, size[0], size[1], b)            # asserts its 1e-6 margin from a truncation edge
        got = U.undistorted_camera(model, p, size[0], size[1], blank_pixels=b)
        assert got == want
        assert got[0][:2] == tuple(R.intrinsics(model, p)[:2])           # focal lengths unchanged


@pytest.mark.parametrize('model', _DISTORTED)
def test_barrel_distortion_keeps_more_with_blank_pixels(model):
    p = _params(model, 1.8)
    (w0, h0), (w1, h1) = U.undistorted_camera(model, p, _W, _H, 0.0)[1], U.undistorted_camera(model, p, _W, _H, 1.0)[1]
    assert w1 >= w0 and h1 >= h0 and (w1, h1) != (w0, h0)


@pytest.mark.parametrize('model', _DISTORTED)
def test_zero_coefficients_give_the_same_camera(model):
    p = list(_params(model))
    n = 3 if R.NPARAMS[model] in (4, 5) else 4
    p[n:] = [0.0] * (len(p) - n)
    for b in (0.0, 1.0):
        K, size = U.undistorted_camera(model, p, _W, _H, b)
        assert size == (_W, _H) and K == tuple(R.intrinsics(model, p)[:4])


def test_scale_bounds_and_a_lens_past_a_pinhole():
    p = R.test_camera('SIMPLE_RADIAL', _W, _H, 1.8)
    assert U.undistorted_camera('SIMPLE_RADIAL', p, _W, _H, 1.0, max_scale=1.05)[1] == (int(1.05 * _W), int(1.05 * _H))
    # k = -0.6: r + k r^3 never reaches the corner's distorted radius
    with pytest.raises(ValueError, match='camera 7'):
        U.undistorted_camera('SIMPLE_RADIAL', (0.8 * _W, 150.0, 100.0, -0.6), _W, _H, camera='camera 7')
    with pytest.raises(ValueError, match='FOV'):
        U.undistorted_camera('FOV', (100.0, 100.0, 50.0, 50.0, 0.9), _W, _H)
    with pytest.raises(ValueError, match='blank_pixels'):
        U.undistorted_camera('SIMPLE_RADIAL', p, _W, _H, 1.5)


def _model(cameras, n_images=4):
    images = [(10 - i, (1.0, 0.01 * i, 0.0, 0.0), (0.1 * i, 0.0, 0.0), cameras[i % len(cameras)][0], 'im%d.jpg' % i,
               [(1.0, 2.0, 1), (3.0, 4.0, -1)]) for i in range(n_images)]
    points = [(1, (0.0, 0.0, 5.0), [(10 - i, 0) for i in range(n_images)])]
    return images, points


def test_read_model_default_still_refuses_distorted_cameras(tmp_path):
    cams = [(1, 'OPENCV', _W, _H, R.test_camera('OPENCV', _W, _H))]
    write_text(str(tmp_path / 't'), cams, *_model(cams))
    write_binary(str(tmp_path / 'b'), cams, *_model(cams))
    for d in ('t', 'b'):
        with pytest.raises(ValueError, match='colmap image_undistorter'):
            colmap.read_model(str(tmp_path / d))


@pytest.mark.parametrize('binary', [False, True])
def test_read_model_allow_distorted_gives_the_undistorted_cameras(tmp_path, binary):
    cams = [(1, 'OPENCV', _W, _H, R.test_camera('OPENCV', _W, _H)), (2, 'PINHOLE', 80, 60, (70.0, 71.0, 40.0, 30.0)),
            (5, 'THIN_PRISM_FISHEYE', 67, 45, R.test_camera('THIN_PRISM_FISHEYE', 67, 45, 1.8))]
    images, points = _model(cams, 6)
    sparse = str(tmp_path / 's')
    write_text(sparse, cams, images, points)
    if binary:
        write_binary(sparse, [cams[0], cams[1]], images, points)
        R.write_cameras_binary(os.path.join(sparse, 'cameras.bin'), cams)
        for name in ('cameras.txt', 'images.txt', 'points3D.txt'):
            os.remove(os.path.join(sparse, name))
    m = colmap.read_model(sparse, allow_distorted=True, blank_pixels=0.5)
    by_id = {c[0]: c for c in cams}
    assert m.image_ids.tolist() == sorted(r[0] for r in images)
    for k, cid in enumerate(m.camera_ids.tolist()):
        _, model, w, h, p = by_id[cid]
        K, size = ((p, (w, h)) if model == 'PINHOLE' else R.output_camera(model, p, w, h, 0.5))
        assert tuple(m.intrinsics[k]) == tuple(K) and tuple(m.size[k]) == size
        assert m.models[k] == model and m.params[k] == tuple(p) and tuple(m.source_size[k]) == (w, h)
    assert colmap.read_model(sparse, allow_distorted=True).size[m.camera_ids == 1][0].tolist() != m.size[m.camera_ids == 1][0].tolist()


def test_fov_is_refused_in_both_modes(tmp_path):
    cams = [(3, 'FOV', _W, _H, (240.0, 240.0, 150.0, 100.0, 0.9))]
    images, points = _model(cams)
    write_text(str(tmp_path / 't'), cams, images, points)
    write_text(str(tmp_path / 'b'), cams, images, points)
    R.write_cameras_binary(str(tmp_path / 'b' / 'cameras.bin'), cams)
    write_binary(str(tmp_path / 'b2'), [(3, 'PINHOLE', _W, _H, (240.0, 240.0, 150.0, 100.0))], images, points)
    for name in ('images.bin', 'points3D.bin'):
        os.rename(str(tmp_path / 'b2' / name), str(tmp_path / 'b' / name))
    for d in ('t', 'b'):
        with pytest.raises(ValueError, match='camera 3 has the FOV model'):
            colmap.read_model(str(tmp_path / d))
        with pytest.raises(ValueError, match='camera 3 has the FOV model'):
            colmap.read_model(str(tmp_path / d), allow_distorted=True)


@pytest.mark.parametrize('argv', [['--out', 'x'], ['--out', 'x', '--dense_folder', 'd', '--sparse', 's', '--image_path', 'i'],
                                  ['--out', 'x', '--sparse', 's'], ['--out', 'x', '--image_path', 'i'],
                                  ['--out', 'x', '--dense_folder', 'd', '--image_path', 'i']])
def test_colmap_scene_wants_exactly_one_input_form(argv, capsys):
    with pytest.raises(SystemExit) as e:
        colmap_scene.main(argv)
    assert e.value.code == 2 and '--dense_folder' in capsys.readouterr().err


def test_make_scene_wants_exactly_one_input_form():
    for args, kw in (((None, 'x'), {}), (('d', 'x'), dict(sparse='s', image_path='i')), ((None, 'x'), dict(sparse='s')),
                     ((None, 'x'), dict(image_path='i'))):
        with pytest.raises(ValueError, match='either dense_folder'):
            colmap.make_scene(*args, **kw)


def test_link_with_a_distorted_camera_raises(tmp_path):
    cams = [(1, 'RADIAL', _W, _H, R.test_camera('RADIAL', _W, _H))]
    write_text(str(tmp_path / 's'), cams, *_model(cams))
    with pytest.raises(ValueError, match='--link'):
        colmap.make_scene(None, str(tmp_path / 'out'), sparse=str(tmp_path / 's'), image_path=str(tmp_path), link=True)


def test_an_image_of_another_size_than_its_camera_raises():
    p = R.test_camera('RADIAL', 67, 45)
    with pytest.raises(ValueError, match='66 x 45 pixels.*67 x 45'):
        U.undistort_image(np.zeros((45, 66, 3), np.uint8), 'RADIAL', p, 67, 45)
    with pytest.raises(ValueError, match='uint8'):
        U.undistort_image(np.zeros((45, 67, 3), np.float32), 'RADIAL', p, 67, 45)


def test_wrapper_argument_checks():
    p = R.test_camera('OPENCV', 67, 45)
    cam = ((50.0, 50.0, 33.0, 22.0), (67, 45))
    with pytest.raises(ValueError, match='FOV'):
        ops.undistort_map('FOV', p, 67, 45, cam)
    with pytest.raises(ValueError, match='8 parameters'):
        ops.undistort_map('OPENCV', p[:5], 67, 45, cam)
    with pytest.raises(ValueError, match='finite'):
        ops.undistort_map('OPENCV', p[:7] + (float('nan'),), 67, 45, cam)
    with pytest.raises(ValueError, match='int32 pixel index'):
        ops.undistort_map('OPENCV', p, 67, 45, (cam[0], (65536, 32768)))
    with pytest.raises(ValueError, match='focal length'):
        ops.undistort_map('OPENCV', p, 67, 45, ((0.0, 50.0, 33.0, 22.0), (67, 45)))
    import torch
    with pytest.raises(TypeError, match='image_u8'):
        ops.undistort_remap(np.zeros((4, 4, 3), np.uint8), torch.zeros((4, 4, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.undistort_remap(torch.zeros((4, 4, 3), dtype=torch.uint8), torch.zeros((4, 4, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match='map'):
        ops.undistort_remap(torch.zeros((4, 4, 3), dtype=torch.uint8), torch.zeros((4, 4, 3), dtype=torch.int32))


def test_library_declares_and_guards_the_new_entry_points():
    names = _lib.declared_symbols()
    assert 'atvs_undistort_map' in names and 'atvs_undistort_remap' in names
    L = _lib.lib()
    assert _lib.header_abi_version() >= 53 and L.atvs_abi_version() == _lib.header_abi_version()
    buf = (ctypes.c_double * 16)()                                       # 16-byte aligned stand-in: refusals come before any launch
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    good = (ctypes.c_double * 12)(50.0, 50.0, 33.0, 22.0, -0.1, 0.01, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    cam = (ctypes.c_double * 4)(50.0, 50.0, 33.0, 22.0)
    assert L.atvs_undistort_map(4, good, 67, 45, cam, 67, 45, None, None) == -1
    for model_id in (0, 1, 7, 11, -1):                                   # the pinholes, FOV, unknown ids
        assert L.atvs_undistort_map(model_id, good, 67, 45, cam, 67, 45, ptr, None) == -3
    bad = (ctypes.c_double * 12)(*good)
    bad[5] = float('inf')
    assert L.atvs_undistort_map(4, bad, 67, 45, cam, 67, 45, ptr, None) == -3
    assert L.atvs_undistort_map(2, bad, 67, 45, cam, 0, 45, ptr, None) == -3
    assert L.atvs_undistort_map(4, good, 65536, 32768, cam, 67, 45, ptr, None) == -3          # W H = 2^31
    assert L.atvs_undistort_map(4, good, 67, 45, cam, 65536, 32768, ptr, None) == -3
    assert L.atvs_undistort_map(4, good, (1 << 21) + 1, 1, cam, 67, 45, ptr, None) == -3
    nan_cam = (ctypes.c_double * 4)(50.0, float('nan'), 33.0, 22.0)
    assert L.atvs_undistort_map(4, good, 67, 45, nan_cam, 67, 45, ptr, None) == -3
    assert L.atvs_undistort_remap(ptr, 67, 45, ptr, 65536, 32768, ptr, None) == -3
    assert L.atvs_undistort_remap(ptr, 65536, 32768, ptr, 67, 45, ptr, None) == -3
    assert L.atvs_undistort_remap(ptr, 67, 45, ctypes.c_void_p(ptr.value + 4), 67, 45, ptr, None) == -3   # misaligned map
    assert L.atvs_undistort_remap(ptr, 67, 45, None, 67, 45, ptr, None) == -1
