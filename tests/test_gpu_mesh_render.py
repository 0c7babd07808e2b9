"""-m gpu: triangle meshes rendered into cameras (csrc/mesh_render.hip, ops.mesh_render, ops.depth_occlude,
eval_depth.render_mesh).

Every comparison of maps with the restatement (tests/mesh_render_restated.py: every face against every pixel) is exact:
np.array_equal on the depth AND on the face.  37 x 53 maps, 9 ring cameras: one camera group of 8 and a remainder of 1."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import atvsnet_amd                                   # noqa: F401
from atvsnet_amd import ops
from atvsnet_amd.atvsnet import eval_depth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_register_restated as RR  # noqa: E402
import mesh_render_restated as MR  # noqa: E402
import tsdf_restated as TR  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS = 37, 53                                  # odd, no multiple of the 64-pixel tile
SMALL = ops.MESH_RENDER_SMALL_PIXELS


def _gpu(dev, vertices, faces, cams, rows, cols, centre=0.0):
    v = torch.from_numpy(np.array(vertices, np.float32).reshape(-1, 3)).to(dev)         # copies: the shared inputs are read-only
    f = torch.from_numpy(np.array(faces, np.int32).reshape(-1, 3)).to(dev)
    c = torch.from_numpy(np.array(cams, np.float64).reshape(-1, 16)).to(dev)
    depth, face = ops.mesh_render(v, f, c, rows, cols, pixel_centre=centre)
    assert depth.dtype == torch.float32 and face.dtype == torch.int32 and depth.device == v.device
    assert tuple(depth.shape) == tuple(face.shape) == (len(c), rows, cols)
    return depth.cpu().numpy(), face.cpu().numpy()


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[0] > 0, got[1] >= 0)


@functools.lru_cache(maxsize=None)
def _cams():
    cams = MR.ring_cameras(9, ROWS, COLS, radius=3.0)
    cams.setflags(write=False)
    return cams


@functools.lru_cache(maxsize=None)
def _soup():
    v, f = MR.triangle_soup(3000, _cams(), ROWS, COLS, seed=5)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


SUBSETS = {'all': np.inf, 'medium': 30.0, 'small': 3.0}      # faces whose longest edge is not known to reach this many pixels


def _subset(name):
    v, f = _soup()
    with np.errstate(invalid='ignore'):
        return f[~(MR.soup_sizes(v, f, _cams()) >= SUBSETS[name])]           # the NaN and infinite faces stay in every subset


@functools.lru_cache(maxsize=None)
def _soup_want(centre, subset):
    want = MR.mesh_render(_soup()[0], _subset(subset), _cams(), ROWS, COLS, centre)
    for w in want:
        w.setflags(write=False)
    return want


@pytest.mark.parametrize('subset', sorted(SUBSETS))
@pytest.mark.parametrize('centre', [0.0, 0.5])
def test_triangle_soup_is_the_restatement(cuda, centre, subset):
    """The whole soup, whose image-sized faces near the cameras hide most of the rest, and the soup without its large faces, where
    the small ones show."""
    v, f = _soup()[0], _subset(subset)
    want = _soup_want(centre, subset)
    covered, shown = (want[0] > 0).mean(), len(np.unique(want[1]))
    assert covered > 0.5 and shown > 40 and (subset != 'medium' or shown > 200)
    got = _gpu(cuda, v, f, _cams(), ROWS, COLS, centre)
    _same(got, want)
    again = _gpu(cuda, v, f, _cams(), ROWS, COLS, centre)                            # the same bits whatever the arrival order
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


def _box_triangle(cam, w, h, u0, v0, depth):
    """A triangle in front of `cam` whose projection spans x in [u0 + 0.3, u0 + w - 1.3], y likewise: under the kernel's rule
    (ceil(min) - 1 .. floor(max) + 1) its box is u0..u0 + w - 1 by v0..v0 + h - 1, w h pixels."""
    c = np.asarray(cam, np.float64)
    R, t = c[:9].reshape(3, 3), c[9:12]
    xs = np.array([u0 + 0.3, u0 + w - 1.3, u0 + 0.3])
    ys = np.array([v0 + 0.3, v0 + 0.3, v0 + h - 1.3])
    p = np.stack([(xs - c[14]) / c[12] * depth, (ys - c[15]) / c[13] * depth, np.full(3, depth)], 1)
    return ((p - t) @ R).astype(np.float32)                                           # R^T (p - t)


@functools.lru_cache(maxsize=None)
def _crossover():
    """Boxes of SMALL - 1, SMALL and SMALL + 1 pixels in camera 0 (and whatever they are in the other eight)."""
    cam = _cams()[0]
    shapes = {}
    for target in (SMALL - 1, SMALL, SMALL + 1):
        w = next(w for w in range(int(np.sqrt(target)), 1, -1) if target % w == 0)
        shapes[target] = (w, target // w)
    assert shapes[64] == (8, 8) and shapes[63] == (7, 9) and shapes[65] == (5, 13)
    v = np.concatenate([_box_triangle(cam, w, h, 3 + 14 * k, 5 + k, 2.0 + 0.1 * k) for k, (w, h) in enumerate(shapes.values())])
    f = np.arange(9, dtype=np.int32).reshape(3, 3)
    return v, f


def test_boxes_at_the_path_crossover(cuda):
    v, f = _crossover()
    want = MR.mesh_render(v, f, _cams(), ROWS, COLS, 0.0)
    assert sorted(np.unique(want[1][0]).tolist()) == [-1, 0, 1, 2]
    _same(_gpu(cuda, v, f, _cams(), ROWS, COLS, 0.0), want)
    for k in range(3):                                                                # and each alone, so each path runs alone
        one = MR.mesh_render(v, f[k:k + 1], _cams(), ROWS, COLS, 0.0)
        _same(_gpu(cuda, v, f[k:k + 1], _cams(), ROWS, COLS, 0.0), one)


@functools.lru_cache(maxsize=None)
def _whole_image_and_dust():
    """Whole-image triangles next to 100 000 sub-pixel ones.  The nine cameras look at the origin from all round a ring, and no
    single plane lies in front of cameras that face each other; so the triangles are the four faces of a tetrahedron around the
    ring: every pixel of all nine images is covered by one of them, and each takes the whole-image box in every camera."""
    rng = np.random.default_rng(17)
    cams = _cams()
    n = 100000
    centre = rng.uniform(-1.0, 1.0, (n, 3))
    pixel = 3.0 / cams[0, 12]
    dust = centre[:, None, :] + rng.normal(size=(n, 3, 3)) * (pixel * rng.uniform(0.05, 0.4, (n, 1, 1)))
    # a closed tetrahedron around ring and dust, radius 60: every ray of every camera leaves through one of its faces, so every
    # pixel of all nine images is covered; its faces cross camera planes.  Face 0 of the mesh is one of them.
    tet = 60.0 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    v = np.concatenate([tet, dust.reshape(-1, 3)]).astype(np.float32)
    f = np.concatenate([np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]), 4 + np.arange(3 * n).reshape(n, 3)]).astype(np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def test_a_triangle_over_every_pixel_next_to_100000_sub_pixel_ones(cuda):
    v, f = _whole_image_and_dust()
    want = MR.mesh_render(v, f, _cams(), ROWS, COLS, 0.0)
    assert (want[0] > 0).all()                                                        # every pixel of all nine images
    assert ((want[1] >= 0) & (want[1] < 4)).any(axis=(1, 2)).all() and (want[1] >= 4).sum() > 1000
    _same(_gpu(cuda, v, f, _cams(), ROWS, COLS, 0.0), want)
    # and the face of the tetrahedron that shows most in one image, alone: the large path with nothing beside it
    k = int(np.argmax([(want[1][c] < 4).sum() for c in range(9)]))
    big = int(np.bincount(want[1][k][want[1][k] < 4]).argmax())
    alone = _gpu(cuda, v, f[big:big + 1], _cams(), ROWS, COLS, 0.0)
    _same(alone, MR.mesh_render(v, f[big:big + 1], _cams(), ROWS, COLS, 0.0))


@pytest.mark.parametrize('n_cams', [1, 9])
@pytest.mark.parametrize('n_faces', [0, 1, 257])
def test_face_counts(cuda, n_cams, n_faces):
    v, f = _soup()
    pick = np.flatnonzero(np.isfinite(v[f].reshape(len(f), -1)).all(1))[:n_faces]     # 256 + 1: a second workgroup of one lane
    want = MR.mesh_render(v, f[pick], _cams()[:n_cams], ROWS, COLS, 0.0)
    got = _gpu(cuda, v, f[pick], _cams()[:n_cams], ROWS, COLS, 0.0)
    _same(got, want)
    if n_faces == 0:
        assert not got[0].any() and (got[1] == -1).all()
    elif n_faces > 1:
        assert got[0].any()


def test_the_tie_rule(cuda):
    v, f = MR.lattice_square()
    for faces, winner in ((np.array([[0, 1, 2], [0, 1, 2]]), 0), (np.array([[0, 2, 3], [0, 1, 2], [2, 1, 0], [0, 1, 2]]), 1)):
        depth, face = _gpu(cuda, v, faces, MR.LATTICE_CAM[None], 24, 32, 0.5)
        only = _gpu(cuda, v, np.array([[0, 1, 2]]), MR.LATTICE_CAM[None], 24, 32, 0.5)
        inside = only[0][0] > 0
        assert inside.sum() > 100 and (face[0][inside] <= winner).all() and (face[0][inside] == winner).sum() > 100
        _same((depth, face), MR.mesh_render(v, faces, MR.LATTICE_CAM[None], 24, 32, 0.5))


def test_known_answer_lattice_square(cuda):
    MR.check_lattice(lambda *a: _gpu(cuda, *a))


def test_watertight_sphere(cuda):
    MR.check_watertight_sphere(lambda *a: _gpu(cuda, *a))


def test_the_devices_own_tsdf_sphere(cuda):
    """tests/test_tsdf_host.py's sphere (radius 10.3, voxel 1) meshed by ops.tsdf_mesh and rendered: no empty pixel inside the
    silhouette shrunk by a voxel, and the depth within twice that test's radial bound 3 h^2 / (8 (r - sqrt(3) h)) of the analytic
    depth where the ray meets the sphere at under 60 degrees of incidence (1 / cos 60 = 2)."""
    h, radius, centre = 1.0, 10.3, np.array([15.7, 16.2, 15.1])
    field = TR.sphere_field(32, h, radius, tuple(centre))
    vol = ops.TsdfVolume.from_dense(field, np.ones_like(field), None, (0.0, 0.0, 0.0), h, 4.0 * h, device=cuda)
    vertices, _, faces = ops.tsdf_mesh(vol)
    assert len(faces) == 11888
    cams = MR.ring_cameras(9, ROWS, COLS, radius=40.0, focal=1.4 * COLS, height=4.0)
    cams[:, 9:12] -= np.einsum('nij,j->ni', cams[:, :9].reshape(-1, 3, 3), centre)      # the ring around the sphere's centre
    depth, face = ops.mesh_render(vertices, faces, torch.from_numpy(cams).to(cuda), ROWS, COLS)
    depth, face = depth.cpu().numpy(), face.cpu().numpy()
    bound = 3.0 * h * h / (8.0 * (radius - np.sqrt(3.0) * h))
    for k in range(len(cams)):
        inner, _, _ = MR.sphere_silhouette(cams[k], ROWS, COLS, radius - h, centre)
        hit, t, cos = MR.sphere_silhouette(cams[k], ROWS, COLS, radius, centre)
        assert inner.sum() > 300 and ((depth[k] == 0) & inner).sum() == 0
        steep = hit & (cos > 0.5)
        assert steep.sum() > 300 and (depth[k][steep] > 0).all()
        assert np.abs(depth[k][steep].astype(np.float64) - t[steep]).max() <= 2.0 * bound + 1e-5


def test_a_bad_index_raises(cuda):
    v, f = MR.lattice_square()
    for bad in (len(v), -1):
        faces = np.concatenate([f, [[0, 1, bad]]]).astype(np.int32)
        with pytest.raises(ValueError, match='1 of 3 faces'):
            _gpu(cuda, v, faces, MR.LATTICE_CAM[None], 24, 32)
    _same(_gpu(cuda, v, f, MR.LATTICE_CAM[None], 24, 32), MR.mesh_render(v, f, MR.LATTICE_CAM[None], 24, 32))


def test_depth_occlude_is_the_rule(cuda):
    rng = np.random.default_rng(23)
    shape = (3, ROWS, COLS)
    d = rng.uniform(0.5, 4.0, shape).astype(np.float32)
    o = (d * rng.choice(np.float32([0.5, 0.97, 1.0, 1.03, 2.0]), shape)).astype(np.float32)
    for a in (d, o):
        flat = a.reshape(-1)
        flat[rng.choice(flat.size, 600, replace=False)] = rng.choice(np.float32([0.0, np.nan, np.inf, -1.0]), 600)
    for tol in (0.0, 0.03, 0.05):
        want = MR.depth_occlude(d, o, tol)
        assert 0.1 < ((want == 0) & (d > 0)).mean() < 0.6
        dd, oo = torch.from_numpy(d).to(cuda), torch.from_numpy(o).to(cuda)
        out = ops.depth_occlude(dd, oo, tol=tol)
        assert np.array_equal(out.cpu().numpy(), want, equal_nan=True) and np.array_equal(dd.cpu().numpy(), d, equal_nan=True)
        assert ops.depth_occlude(dd, oo, tol=tol, out=dd) is dd                        # in place
        assert np.array_equal(dd.cpu().numpy(), want, equal_nan=True)


def test_render_mesh_moves_the_vertices_by_the_inverse(cuda):
    v, f = _soup()
    keep = np.flatnonzero(np.isfinite(v[f].reshape(len(f), -1)).all(1))[:600]
    recon, faces = v[f[keep]].reshape(-1, 3), np.arange(3 * len(keep), dtype=np.int32).reshape(-1, 3)
    a = np.deg2rad(30.0)
    T = np.eye(4)
    T[:3, :3] = 2.5 * np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    T[:3, 3] = (4.0, -7.0, 1.5)
    scan = RR.transform(recon, T)
    back = RR.transform(scan, eval_depth.inverse_similarity(T))
    assert not np.array_equal(back, recon)
    got = eval_depth.render_mesh(scan, faces, _cams(), ROWS, COLS, transform=T, pixel_centre=0.5, device=cuda)
    _same((got[0].cpu().numpy(), got[1].cpu().numpy()), MR.mesh_render(back, faces, _cams(), ROWS, COLS, 0.5))
