"""CPU: every builder of tests/tsdf_cases.py and the conditions tests/test_gpu_tsdf_cases.py relies on, asserted on the dense
restatement alone.  A case that has gone trivial -- every block empty, no NaN anywhere, a sign pattern that no longer occurs --
fails here, with no GPU needed."""
import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_restated as R


@pytest.mark.parametrize('trunc', TC.UNEVEN_TRUNCS)
def test_uneven_box_random_depths_shifted_centre_four_channels(trunc):
    case = TC.uneven(trunc)
    assert case.dims == (3, 5, 2) and case.pixel_centre == 0.5 and case.depths.shape == ((3 if trunc == 0.9 else 5), 23, 31)
    print('uneven, trunc %g: %d of 30 blocks, weight up to %g' % (trunc, len(case.want['blocks']), case.want['weight'].max()))
    TC.check_uneven(case)
    assert len(case.want_mesh()[2]) > 0


def test_uneven_box_without_images():
    case = TC.uneven(0.2, with_images=False)
    assert case.images is None and case.want['color'] is None
    TC.check_uneven(case)
    assert np.array_equal(case.want['weight'], TC.uneven(0.2).want['weight'])


def test_trunc_below_a_voxel_and_above_a_block():
    edge = 8 * TC.VOXEL
    assert TC.UNEVEN_TRUNCS[1] < TC.VOXEL < TC.UNEVEN_TRUNCS[0] < edge < TC.UNEVEN_TRUNCS[2]


def test_lone_coarse_pixels_need_the_centre_in_the_marking_corners():
    TC.check_lone_pixels(TC.lone_pixels())
    # the 23 x 31 maps of the uneven box cannot show it: half a pixel is about a voxel there, which the padding covers
    for trunc in TC.UNEVEN_TRUNCS:
        case = TC.uneven(trunc)
        assert set(case.linear_blocks().tolist()) <= set(TC.marked_blocks(case, centre_in_corners=False).tolist())


@pytest.mark.parametrize('name', TC.GATHER)
def test_marking_is_a_strict_superset_where_the_gather_path_is_tested(name):
    case = TC.gather_case(name)
    marked = TC.check_marking_is_a_strict_superset(case)
    print('%s: %d blocks marked, %d occupied' % (name, marked, len(case.want['blocks'])))


def test_marking_restated_covers_every_case():
    cases = [TC.uneven(t) for t in TC.UNEVEN_TRUNCS] + [TC.full_box(), TC.camera_inside(), TC.lone_pixels()]
    for case in cases + [TC.mask_bits(live) for live in TC.MASK_LIVE]:
        assert set(case.linear_blocks().tolist()) <= set(TC.marked_blocks(case).tolist())


def test_every_block_occupied():
    TC.check_full_box(TC.full_box())


def test_cameras_inside_the_box():
    TC.check_camera_inside(TC.camera_inside())


@pytest.mark.parametrize('live', TC.MASK_LIVE)
def test_mask_bits(live):
    TC.check_mask_bits(TC.mask_bits(live), live)


def test_mask_bits_cover_both_halves_and_the_top_bit():
    assert TC.MASK_LIVE == ((31,), (32,), (63,), (31, 32, 63))


def test_a_directory_beyond_one_scan_tile():
    case = TC.long_directory()
    lin = case.linear_blocks()
    print('long directory: %d blocks, %d..%d, %d at or beyond 2048' % (len(lin), lin.min(), lin.max(), (lin >= 2048).sum()))
    TC.check_long_directory(case)
    assert len(case.want_mesh()[2]) > 10000


def test_random_signs_reach_every_pattern_and_both_clamps():
    case = TC.random_signs()
    v, c, f = case.want(1.0)
    print('random signs: %d cubes meshed, V = %d, F = %d, %d channel values at 0, %d at 255'
          % (case.cubes()[0].sum(), len(v), len(f), (c == 0).sum(), (c == 255).sum()))
    TC.check_random_signs(case)
    assert sorted(set(f.reshape(-1).tolist())) == list(range(len(v)))
    assert (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all()


def test_the_sphere():
    TC.check_sphere(TC.sphere())


@pytest.mark.parametrize('kind', TC.ZEROS)
def test_zeros_and_denormals(kind):
    TC.check_zeros(TC.zeros(kind), kind)


def test_both_zeros_are_outside():
    plus, minus = TC.zeros('plus'), TC.zeros('minus')
    assert np.array_equal(plus.tsdf, minus.tsdf) and not np.array_equal(plus.tsdf.view(np.uint32), minus.tsdf.view(np.uint32))
    assert np.array_equal(plus.want(1.0)[2], minus.want(1.0)[2])
    # counted inside, the zeros would give another mesh
    f = plus.tsdf.copy()
    f[plus.notes['at']] = -1e-30
    assert len(R.mesh(f, plus.weight, plus.color, plus.origin, plus.voxel)[2]) != len(plus.want(1.0)[2])


@pytest.mark.parametrize('kind', TC.SPECIALS)
def test_special_values(kind):
    TC.check_special(TC.special(kind), kind)


def test_special_values_together_give_every_class():
    kinds = {k: TC.special(k) for k in TC.SPECIALS}
    assert any(np.isnan(c.want(TC.special_min_weight(k))[0]).any() for k, c in kinds.items())
    x = kinds['colours'].colour_expressions()
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    assert {TC.special_min_weight(k) for k in TC.SPECIALS} == {1.0, 0.0, float('-inf'), float('inf')}


def test_the_restated_colour_rule_on_finite_inputs_is_round_and_clamp():
    case = TC.random_signs()
    x = case.colour_expressions(2.5)
    assert np.isfinite(x).all()
    want = np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)[:, ::-1]
    assert np.array_equal(case.want(2.5)[1], want)


@pytest.mark.parametrize('variant', TC.ABSENT)
def test_absent_blocks(variant):
    TC.check_absent(TC.absent(variant), variant)


def test_absent_variants():
    assert len(TC.ABSENT) == 8 + 1 + 6 and len(set(TC.ABSENT)) == len(TC.ABSENT)
    assert sorted(len(TC._absent_blocks(v)) for v in TC.ABSENT) == [1] * 8 + [2] + [4] * 6
    # one block away: its opposite lacks a corner neighbour, three lack an edge neighbour, three a face neighbour
    for variant in TC.ABSENT[:8]:
        gone = np.array(variant[1:])
        away = sorted(int(np.abs(np.array(b) - gone).sum()) for b in np.ndindex(2, 2, 2) if tuple(b) != tuple(gone))
        assert away == [1, 1, 1, 2, 2, 2, 3]


@pytest.mark.parametrize('dims', TC.THIN)
def test_thin_boxes(dims):
    TC.check_thin(TC.thin(dims), dims)
