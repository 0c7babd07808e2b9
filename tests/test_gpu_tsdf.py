"""ops.tsdf_integrate and ops.tsdf_mesh on the GPU against tests/tsdf_restated.py, bit for bit (np.array_equal everywhere): the
dense restatement visits every voxel of the box for every view, so equal `blocks` is the allocation proof -- nothing the dense
form finds is missing from the marked blocks."""
import numpy as np
import pytest
import torch

import tsdf_restated as R
from scan_render_restated import ring_cameras
from tsdf_cases import _mesh_equal, _volume_equal

pytestmark = pytest.mark.gpu

RADIUS, VOXEL, TRUNC = 0.9, 0.05, 0.2
ORIGIN = (-1.237, -1.181, -1.213)
DIMS = (6, 6, 6)


@pytest.fixture(scope='module')
def ops():
    from atvsnet_amd import ops as o
    return o


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


class Case(object):
    def __init__(self, n, rows, cols, origin=ORIGIN, dims=DIMS, voxel=VOXEL, trunc=TRUNC, with_images=True):
        self.cams = ring_cameras(n, rows, cols)
        self.depths, images = R.sphere_depths(self.cams, rows, cols, RADIUS)
        self.images = images if with_images else None
        self.origin, self.dims, self.voxel, self.trunc = origin, dims, voxel, trunc
        self.want = R.integrate(self.depths, self.cams, voxel, trunc, origin, dims, self.images)

    def run(self, ops, **kw):
        d, c, im = _dev(self.depths, self.cams, self.images)
        return ops.tsdf_integrate(d, c, self.voxel, self.trunc, self.origin, self.dims, images=im, **kw)

    def want_mesh(self, min_weight=1.0):
        return R.mesh(self.want['tsdf'], self.want['weight'], self.want['color'], self.origin, self.voxel, min_weight)


@pytest.fixture(scope='module')
def ring():
    case = Case(9, 37, 53)
    assert len(case.want['blocks']) > 8 and case.want['weight'].max() >= 3
    return case


@pytest.fixture(scope='module')
def ring_volume(ops, ring):
    return ring.run(ops)


def test_integrate_equals_the_dense_restatement(ring, ring_volume):
    _volume_equal(ring_volume, ring.want)


def test_integrate_gives_the_same_bits_again(ops, ring, ring_volume):
    again = ring.run(ops)
    for a, b in ((again.blocks, ring_volume.blocks), (again.tsdf, ring_volume.tsdf), (again.weight, ring_volume.weight),
                 (again.color, ring_volume.color)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope='module')
def ring_mesh_want(ring):
    return ring.want_mesh()


def test_mesh_equals_the_restatement(ops, ring_volume, ring_mesh_want):
    assert len(ring_mesh_want[0]) > 1000 and len(ring_mesh_want[2]) > 2000
    _mesh_equal(ops.tsdf_mesh(ring_volume), ring_mesh_want)
    # min_weight selects among the views' overlaps
    _mesh_equal(ops.tsdf_mesh(ring_volume, min_weight=2), R.mesh_of_volume(ring_volume, 2))


def test_the_open_mesh_is_a_consistently_oriented_surface_near_the_sphere(ops, ring_volume):
    v, _, f = ops.tsdf_mesh(ring_volume)
    v, f = v.cpu().numpy().astype(np.float64), f.cpu().numpy()
    directed, undirected = R.edge_stats(f)
    assert max(undirected.values()) <= 2
    assert max(directed.values()) == 1                  # an edge shared by two faces runs once in each direction
    assert min(undirected.values()) == 1                # the ring does not see the poles: the mesh is open
    assert sorted(set(f.reshape(-1).tolist())) == list(range(len(v)))
    assert np.abs(np.linalg.norm(v, axis=1) - RADIUS).max() <= TRUNC + np.sqrt(3.0) * VOXEL
    # normals point into free space: away from the centre
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum('ij,ij->i', n, v[f].mean(axis=1)) >= 0).mean() > 0.99


def test_one_view(ops):
    case = Case(1, 37, 53)
    vol = case.run(ops)
    _volume_equal(vol, case.want)
    _mesh_equal(ops.tsdf_mesh(vol), case.want_mesh())


def test_65_views_need_a_second_mask_word(ops):
    case = Case(65, 5, 7, origin=(-1.237, -1.181, -1.213), dims=(6, 6, 6), voxel=0.05, trunc=0.2)
    assert case.want['weight'].max() > 1
    vol = case.run(ops)
    _volume_equal(vol, case.want)
    # the last view alone lives in the second word
    d, c, im = _dev(case.depths, case.cams, case.images)
    d[:64] = 0
    last = R.integrate(d.cpu().numpy(), case.cams, case.voxel, case.trunc, case.origin, case.dims, case.images)
    assert last['weight'].max() == 1
    _volume_equal(ops.tsdf_integrate(d, c, case.voxel, case.trunc, case.origin, case.dims, images=im), last)


def test_cameras_that_carry_their_intrinsics_in_the_matrix(ops):
    # K [R | t] with fx = fy = 1, cx = cy = 0: the same pinhole, a 3x3 that is no rotation -- marking must invert it, not transpose it
    case = Case(3, 21, 29)
    K = np.zeros((3, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = case.cams[:, 12], case.cams[:, 13], case.cams[:, 14], case.cams[:, 15], 1.0
    baked = case.cams.copy()
    baked[:, :9] = (K @ case.cams[:, :9].reshape(3, 3, 3)).reshape(3, 9)
    baked[:, 9:12] = np.einsum('nij,nj->ni', K, case.cams[:, 9:12])
    baked[:, 12:] = (1.0, 1.0, 0.0, 0.0)
    want = R.integrate(case.depths, baked, case.voxel, case.trunc, case.origin, case.dims, case.images)
    assert np.array_equal(want['blocks'], case.want['blocks']) and want['weight'].sum() > 0.99 * case.want['weight'].sum()
    d, c, im = _dev(case.depths, baked, case.images)
    _volume_equal(ops.tsdf_integrate(d, c, case.voxel, case.trunc, case.origin, case.dims, images=im), want)


def test_without_images_there_is_no_color(ops):
    case = Case(3, 21, 29, with_images=False)
    vol = case.run(ops)
    assert vol.color is None
    _volume_equal(vol, case.want)
    _mesh_equal(ops.tsdf_mesh(vol), case.want_mesh())


def test_all_zero_depths_give_an_empty_volume_and_mesh(ops, ring):
    d, c, im = _dev(np.zeros_like(ring.depths), ring.cams, ring.images)
    vol = ops.tsdf_integrate(d, c, VOXEL, TRUNC, ORIGIN, DIMS, images=im)
    assert vol.num_blocks == 0 and tuple(vol.tsdf.shape) == (0, 8, 8, 8) and tuple(vol.color.shape) == (0, 8, 8, 8, 3)
    v, col, f = ops.tsdf_mesh(vol)
    assert tuple(v.shape) == (0, 3) and tuple(col.shape) == (0, 3) and tuple(f.shape) == (0, 3)


def test_a_volume_of_a_single_block(ops):
    # a box of one block in front of one camera, on the near side of the sphere
    cams = ring_cameras(2, 37, 53)
    centre = -cams[0, :9].reshape(3, 3).T @ cams[0, 9:12]
    surface = centre / np.linalg.norm(centre) * RADIUS
    origin = tuple((surface - 4 * VOXEL).tolist())
    case = Case(2, 37, 53, origin=origin, dims=(1, 1, 1))
    assert case.want['blocks'].tolist() == [[0, 0, 0]]
    vol = case.run(ops)
    _volume_equal(vol, case.want)
    want = case.want_mesh()
    assert len(want[2]) > 0
    _mesh_equal(ops.tsdf_mesh(vol), want)


def test_a_surface_along_a_block_face_with_the_neighbour_absent(ops):
    # the plane x = 8: block (0,0,0) inside up to its last voxel, the outside half in block (1,0,0), which is absent above y = 8
    f = np.ones((16, 16, 16), np.float32)
    f[:, :, :8] = -0.5
    f[:, :, 7] = -0.25
    w = np.ones((16, 16, 16), np.float32)
    w[:, 8:, 8:] = 0                                     # block (1,1,*) has no weight: it is not there
    w[8:, :, :] = 0                                      # nor is any block of the upper z layer
    color = np.zeros((16, 16, 16, 3), np.float32)
    color[..., 0] = np.arange(16, dtype=np.float32)[None, None, :] * 10
    color[..., 2] = 200
    vol = ops.TsdfVolume.from_dense(f, w, color, (0.5, -0.25, 1.0), 0.1, 0.4, device='cuda')
    assert vol.blocks.cpu().tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    want = R.mesh(f, w, color, (0.5, -0.25, 1.0), 0.1)
    assert len(want[2]) > 0
    got = ops.tsdf_mesh(vol)
    _mesh_equal(got, want)
    assert float(got[0][:, 1].max()) < -0.25 + 8 * 0.1   # nothing is meshed towards the absent block


def test_max_blocks_raises_with_the_needed_count(ops, ring):
    marked = None
    with pytest.raises(ValueError, match=r'mark (\d+) blocks') as e:
        ring.run(ops, max_blocks=1)
    marked = int(str(e.value).split('mark ')[1].split()[0])
    assert len(ring.want['blocks']) <= marked <= 6 * 6 * 6
    assert ring.run(ops, max_blocks=marked).num_blocks == len(ring.want['blocks'])


def test_a_voxel_too_small_raises_without_a_fault(ops, ring):
    d, c, im = _dev(ring.depths, ring.cams, ring.images)
    with pytest.raises(ValueError, match='too small'):
        ops.tsdf_integrate(d, c, 1e-4, TRUNC, (-0.03, -0.03, 0.87), (64, 64, 64), images=im)
    # the device is as it was
    _volume_equal(ring.run(ops), ring.want)
