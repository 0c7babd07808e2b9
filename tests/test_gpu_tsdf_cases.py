"""ops.tsdf_integrate and ops.tsdf_mesh on the inputs of tests/tsdf_cases.py against tests/tsdf_restated.py, bit for bit: uneven
boxes, a shifted pixel centre, four channels, rough depth maps with every kind of invalid depth, trunc below a voxel and above a
block, cameras inside the box, the view mask's halves and top bit, a directory beyond one scan tile, the gather path; and from
dense arrays every sign pattern of a cube, both zeros and denormals, NaN and infinite tsdf, colours and weights, neighbours
missing across a face, an edge and a corner.  What makes each input discriminate is asserted in tests/test_tsdf_cases_host.py."""
import numpy as np
import pytest
import torch

import tsdf_cases as TC
import tsdf_restated as R
from tsdf_cases import _mesh_equal, _mesh_equal_but_for_nan_bits, _volume_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops(cuda):
    from atvsnet_amd import ops as o
    return o


def _integrate(ops, case, **kw):
    d, c = torch.from_numpy(case.depths).cuda(), torch.from_numpy(case.cams).cuda()
    im = None if case.images is None else torch.from_numpy(case.images).cuda()
    return ops.tsdf_integrate(d, c, case.voxel, case.trunc, case.origin, case.dims, images=im, pixel_centre=case.pixel_centre, **kw)


def _marked(ops, case):
    """How many blocks marking finds, read from the error that max_blocks = 1 raises."""
    with pytest.raises(ValueError, match=r'mark (\d+) blocks') as e:
        _integrate(ops, case, max_blocks=1)
    return int(str(e.value).split('mark ')[1].split()[0])


# ------------------------------------------------------------------------------------------------------------------ integration
@pytest.mark.parametrize('trunc', TC.UNEVEN_TRUNCS)
def test_uneven_box_random_depths_shifted_centre_four_channels(ops, trunc):
    case = TC.uneven(trunc)
    vol = _integrate(ops, case)
    _volume_equal(vol, case.want)
    _mesh_equal(ops.tsdf_mesh(vol), case.want_mesh())


def test_uneven_box_without_images(ops):
    case = TC.uneven(0.2, with_images=False)
    vol = _integrate(ops, case)
    assert vol.color is None
    _volume_equal(vol, case.want)
    _mesh_equal(ops.tsdf_mesh(vol), case.want_mesh())


def test_lone_coarse_pixels_need_the_centre_in_the_marking_corners(ops):
    case = TC.lone_pixels()
    vol = _integrate(ops, case)
    _volume_equal(vol, case.want)
    _mesh_equal(ops.tsdf_mesh(vol), case.want_mesh())


def test_every_block_occupied(ops):
    case = TC.full_box()
    vol = _integrate(ops, case)
    assert vol.num_blocks == 6
    _volume_equal(vol, case.want)
    _mesh_equal(ops.tsdf_mesh(vol), case.want_mesh())


def test_cameras_inside_the_box(ops):
    case = TC.camera_inside()
    vol = _integrate(ops, case)
    _volume_equal(vol, case.want)
    _mesh_equal(ops.tsdf_mesh(vol), case.want_mesh())


@pytest.mark.parametrize('live', TC.MASK_LIVE)
def test_mask_bits(ops, live):
    case = TC.mask_bits(live)
    vol = _integrate(ops, case)
    _volume_equal(vol, case.want)
    assert float(vol.weight.max()) == float(case.want['weight'].max())
    _mesh_equal(ops.tsdf_mesh(vol), case.want_mesh())


def test_a_directory_beyond_one_scan_tile(ops):
    case = TC.long_directory()
    vol = _integrate(ops, case)
    _volume_equal(vol, case.want)
    _mesh_equal(ops.tsdf_mesh(vol), case.want_mesh())


@pytest.mark.parametrize('name', TC.GATHER)
def test_the_gather_path_runs(ops, name):
    # marking is a strict superset of the occupied blocks: integration leaves slots without a weight, which gather drops
    case = TC.gather_case(name)
    occupied = len(case.want['blocks'])
    with pytest.raises(ValueError, match=r'mark (\d+) blocks') as e:
        _integrate(ops, case, max_blocks=occupied)
    marked = int(str(e.value).split('mark ')[1].split()[0])
    assert occupied < marked <= int(np.prod(case.dims))
    assert marked == _marked(ops, case)
    with pytest.raises(ValueError, match='mark %d blocks' % marked):
        _integrate(ops, case, max_blocks=marked - 1)
    vol = _integrate(ops, case, max_blocks=marked)
    assert vol.num_blocks == occupied
    _volume_equal(vol, case.want)


# ------------------------------------------------------------------------------------------------------------------- extraction
def _surface_rules(v, f):
    directed, undirected = R.edge_stats(f)
    assert max(undirected.values()) <= 2                # no edge in more than two faces
    assert max(directed.values()) == 1                  # and the two run against each other
    assert sorted(set(f.reshape(-1).tolist())) == list(range(len(v)))              # every vertex is referenced
    assert (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all()                 # the smallest index first
    return directed, undirected


@pytest.mark.parametrize('min_weight', TC.RANDOM_MIN_WEIGHTS)
def test_random_signs_on_an_uneven_box(ops, min_weight):
    case = TC.random_signs()
    vol = case.volume(ops)
    assert vol.dims == (3, 5, 2)
    got = ops.tsdf_mesh(vol, min_weight=min_weight)
    _mesh_equal(got, case.want(min_weight))
    _surface_rules(got[0].cpu().numpy(), got[2].cpu().numpy())
    again = ops.tsdf_mesh(vol, min_weight=min_weight)
    for a, b in zip(got, again):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_the_closed_sphere(ops):
    case = TC.sphere()
    got = ops.tsdf_mesh(case.volume(ops))
    _mesh_equal(got, case.want(1.0))
    v, f = got[0].cpu().numpy(), got[2].cpu().numpy()
    directed, undirected = _surface_rules(v, f)
    assert (len(v), len(f)) == (5946, 11888) and len(v) - len(undirected) + len(f) == 2
    assert all(directed.get((b, a), 0) == 1 for a, b in directed)                 # closed: every directed edge has its reverse


@pytest.mark.parametrize('kind', TC.ZEROS)
def test_zeros_and_denormals(ops, kind):
    case = TC.zeros(kind)
    _mesh_equal(ops.tsdf_mesh(case.volume(ops)), case.want(1.0))


@pytest.mark.parametrize('kind', TC.SPECIALS)
def test_special_values(ops, kind):
    case, mw = TC.special(kind), TC.special_min_weight(kind)
    _mesh_equal_but_for_nan_bits(ops.tsdf_mesh(case.volume(ops), min_weight=mw), case.want(mw))


def test_all_blocks_present(ops):
    case = TC.absent(None)
    vol = case.volume(ops)
    assert vol.num_blocks == 8
    _mesh_equal(ops.tsdf_mesh(vol), case.want(1.0))


@pytest.mark.parametrize('variant', TC.ABSENT, ids=lambda v: '-'.join(str(x) for x in v))
def test_absent_blocks(ops, variant):
    case = TC.absent(variant)
    vol = case.volume(ops)
    assert vol.num_blocks == 8 - len(TC._absent_blocks(variant))
    _mesh_equal(ops.tsdf_mesh(vol), case.want(1.0))


@pytest.mark.parametrize('dims', TC.THIN)
def test_thin_boxes(ops, dims):
    case = TC.thin(dims)
    vol = case.volume(ops)
    assert vol.dims == dims and vol.num_blocks == 4
    _mesh_equal(ops.tsdf_mesh(vol), case.want(1.0))
