"""COLMAP import, host side (no GPU): the model reader in both formats, the rotation, the camera check, distinct
observations, the ranking and fallback rules of pair.txt, the camera text, and the ABI's argument checks."""
import ctypes
import io
import os

import numpy as np
import pytest

import atvsnet_amd  # noqa: F401
from atvsnet_amd import _lib
from atvsnet_amd.atvsnet import colmap as C
from atvsnet_amd.atvsnet import preprocess as P

from colmap_model import write_binary, write_text

ERR_SHAPE = -2


def _model():
    cameras = [(3, 'PINHOLE', 200, 140, (180.0, 181.5, 100.25, 70.5)), (1, 'SIMPLE_PINHOLE', 160, 120, (150.0, 80.0, 60.0))]
    images = [
        (12, (0.9, 0.1, -0.2, 0.05), (0.1, -0.2, 3.0), 3, 'b.jpg', [(1.0, 2.0, 7), (3.5, 4.0, -1), (5.0, 6.0, 7), (7.0, 8.0, 9)]),
        (4, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1, 'a.jpg', [(1.5, 2.5, 9), (2.0, 2.0, 11)]),
        (30, (0.3, 0.4, 0.5, 0.6), (1.0, 2.0, 3.0), 3, 'c d.jpg', []),                       # empty POINTS2D line
        (20, (2.0, 0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 1, 'e.jpg', [(9.0, 9.0, 11), (1.0, 1.0, 7), (4.0, 4.0, -1)]),
    ]
    points = [(11, (0.5, -0.25, 4.0), [(4, 1), (20, 0)]), (7, (1.0, 2.0, 5.0), [(12, 0), (12, 2), (20, 1)]),
              (9, (-1.0, 0.0, 6.0), [(12, 3), (4, 0)])]
    return cameras, images, points


@pytest.fixture
def model_dirs(tmp_path):
    cams, imgs, pts = _model()
    write_text(str(tmp_path / 'txt'), cams, imgs, pts)
    write_binary(str(tmp_path / 'bin'), cams, imgs, pts)
    return str(tmp_path / 'txt'), str(tmp_path / 'bin')


def test_text_and_binary_read_back_identically(model_dirs):
    a, b = (C.read_model(d) for d in model_dirs)
    for name in C.Model.__slots__:
        va, vb = getattr(a, name), getattr(b, name)
        if isinstance(va, np.ndarray):
            assert va.dtype == vb.dtype and va.shape == vb.shape and va.tobytes() == vb.tobytes(), name
        else:
            assert va == vb, name
    assert a.image_ids.tolist() == [4, 12, 20, 30]                       # ascending IMAGE_ID = scene order
    assert a.names == ['a.jpg', 'b.jpg', 'e.jpg', 'c d.jpg']
    assert a.intrinsics.tolist() == [[150.0, 150.0, 80.0, 60.0], [180.0, 181.5, 100.25, 70.5]] * 2   # SIMPLE_PINHOLE: fx = fy
    assert a.size.tolist() == [[160, 120], [200, 140], [160, 120], [200, 140]]
    assert a.xyz.tolist() == [[1.0, 2.0, 5.0], [-1.0, 0.0, 6.0], [0.5, -0.25, 4.0]]   # ascending POINT3D_ID 7, 9, 11
    assert a.t.tolist() == [[0.0, 0.0, 0.0], [0.1, -0.2, 3.0], [0.5, 0.5, 0.5], [1.0, 2.0, 3.0]]


def test_duplicate_observation_counts_once(model_dirs):
    m = C.read_model(model_dirs[0])
    tracks = [m.observers[m.offsets[i]:m.offsets[i + 1]].tolist() for i in range(len(m.offsets) - 1)]
    # point ids 7, 9, 11: image 12 (scene 1) sees 7 twice -> once; -1 entries dropped (PointList, colmap_helpers.py:18-27)
    assert tracks == [[1, 2], [0, 1], [0, 2]]
    assert m.offsets.dtype == np.int32 and m.observers.dtype == np.int32


def _rodrigues(q):
    """An independent rotation formula: axis-angle of the unit quaternion, R = cos a I + sin a [u]x + (1 - cos a) u u^T."""
    q = np.asarray(q, np.float64) / np.linalg.norm(q)
    a = 2.0 * np.arctan2(np.linalg.norm(q[1:]), q[0])
    u = q[1:] / np.linalg.norm(q[1:]) if np.linalg.norm(q[1:]) > 0 else np.array([1.0, 0.0, 0.0])
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.cos(a) * np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * np.outer(u, u)


def test_rotation_matches_an_independent_formula():
    rng = np.random.default_rng(0)
    qs = rng.normal(size=(200, 4))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    R = C.quaternion_to_rotation(qs)
    for q, r in zip(qs, R):
        assert np.abs(r - _rodrigues(q)).max() <= 1e-15
    # a non-unit quaternion normalises; the world-to-camera convention of colmap_helpers.py:53-57 (identity for (1,0,0,0))
    assert np.abs(C.quaternion_to_rotation(3.7 * qs) - R).max() <= 1e-15
    assert C.quaternion_to_rotation([2.0, 0, 0, 0]).tolist() == np.eye(3).tolist()


@pytest.mark.parametrize('model', ['OPENCV', 'RADIAL'])
@pytest.mark.parametrize('fmt', ['txt', 'bin'])
def test_distorted_cameras_name_the_undistorter(tmp_path, model, fmt):
    cams, imgs, pts = _model()
    params = {'OPENCV': (180.0, 180.0, 100.0, 70.0, 0.1, 0.01, 0.0, 0.0), 'RADIAL': (180.0, 100.0, 70.0, 0.1, 0.01)}[model]
    cams = [(3, model, 200, 140, params), cams[1]]
    (write_text if fmt == 'txt' else write_binary)(str(tmp_path), cams, imgs, pts)
    with pytest.raises(ValueError, match='colmap image_undistorter'):
        C.read_model(str(tmp_path))


def test_images_txt_parsed_by_content(tmp_path):
    """Header counts are not trusted (the reference's regexes read them): a wrong count line, blank lines between records."""
    cams, imgs, pts = _model()
    write_text(str(tmp_path), cams, imgs, pts)
    path = tmp_path / 'images.txt'
    text = path.read_text().replace('# Number of images: 4', '# Number of images: 2') + '\n\n'
    path.write_text(text)
    m = C.read_model(str(tmp_path))
    assert m.image_ids.tolist() == [4, 12, 20, 30]


# pair.txt on a 6-image toy, worked by hand.  Image 4 has no point in view (left out: neither reference nor source).
_SHARED = np.array([[0, 5, 5, 0, 9, 0],
                    [5, 0, 2, 2, 0, 0],
                    [5, 2, 0, 0, 0, 0],
                    [0, 2, 0, 0, 0, 0],
                    [9, 0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0, 0]], np.int32)
_KEEP = np.array([1, 1, 1, 1, 0, 1], bool)
_PAIR = ('5\n'
         '0\n3 2 5 1 5 3 0\n'          # tie 5 / 5: the higher index (2) first; 4 is left out; fallback +3 (1, 2 already listed)
         '1\n3 0 5 3 2 2 2\n'          # tie 2 / 2: 3 before 2
         '2\n3 0 5 1 2 3 0\n'          # zero stops the ranking; fallback +1 = 3
         '3\n3 1 2 2 0 5 0\n'          # fallback: +1 = 4 left out, -1 = 2, +2 = 5 (1 already listed)
         '5\n3 3 0 2 0 1 0\n')         # nothing shared: -2, -3, -4 by scene index, never 5 itself


def test_pair_txt_ranking_and_fallback_by_hand():
    assert C.pair_text(C.select_sources(_SHARED, _KEEP, 3)) == _PAIR


def test_pair_txt_matches_the_restated_reference():
    from colmap_model import neighbours_restated
    rng = np.random.default_rng(4)
    n = 23
    sets = [set(rng.choice(60, size=rng.integers(0, 12), replace=False).tolist()) for _ in range(n)]
    keep = rng.uniform(size=n) > 0.15
    shared = np.array([[0 if i == j else len(sets[i] & sets[j]) for j in range(n)] for i in range(n)], np.int32)
    for num in (1, 4, 10):
        assert C.pair_text(C.select_sources(shared, keep, num)) == neighbours_restated(sets, keep, num)


def test_cam_text_round_trips_through_load_cam():
    R = C.quaternion_to_rotation([0.9, 0.1, -0.2, 0.05])
    cam = C.scene_camera(R, np.array([0.1, -0.2, 3.0]), (180.0, 181.5, 100.25, 70.5), 0.125, 0.4375, 128, 1.33333)
    back = P.load_cam(io.StringIO(P.cam_text(cam)))
    assert back.tobytes() == cam.tobytes()
    # preprocess_colmap.load_cam:204-214 with max_disp = d_hi * stretch, min_disp = d_lo / stretch (colmap_helpers.py:329-331)
    depth_min = 1.0 / float(0.4375 * 1.33333)
    depth_max = 1.0 / float(0.125 / 1.33333)
    assert cam[1, 3].tolist() == [depth_min, (depth_max - depth_min) / float(127), 128.0, depth_max]
    assert cam[0, :3, :3].tolist() == R.tolist() and cam[0, :3, 3].tolist() == [0.1, -0.2, 3.0] and cam[0, 3].tolist() == [0, 0, 0, 1]


def test_non_jpeg_source_is_refused(tmp_path):
    cams, imgs, pts = _model()
    write_text(str(tmp_path / 'sparse'), cams, imgs, pts)
    os.makedirs(str(tmp_path / 'images'))
    for name in ('a.jpg', 'b.jpg', 'e.jpg', 'c d.jpg'):
        (tmp_path / 'images' / name).write_bytes(b'\x89PNG\r\n')
    with pytest.raises(ValueError, match='JPEG'):
        C.make_scene(str(tmp_path), str(tmp_path / 'out'))
    assert not os.path.exists(str(tmp_path / 'out'))


def test_abi_argument_checks():
    L = _lib.lib()
    null = ctypes.c_void_p(0)
    # more than 16384 images: the matrix would pass 1 GiB -- refused before any pointer is read
    assert L.atvs_colmap_covisibility(null, null, 0, 0, 16385, null, null) == ERR_SHAPE
    assert L.atvs_colmap_covisibility(null, null, 0, 0, 0, null, null) == ERR_SHAPE
    nbytes = ctypes.c_long(0)
    assert L.atvs_colmap_depth_range_scratch_size(2000, ctypes.byref(nbytes)) == 0
    assert 2000 * 2 * 256 * 4 <= nbytes.value < 2000 * 2 * 256 * 4 + 2000 * 64 + 256
    assert L.atvs_colmap_depth_range_scratch_size(0, ctypes.byref(nbytes)) == ERR_SHAPE
