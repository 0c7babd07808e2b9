"""The per-element bar of tests/numerics.py is strong enough: a CPU emulation of the split-operand arithmetic (fp16
pieces h0 + h1 / 2048 of both operands, the three products h0*g0 + (h0*g1 + h1*g0) / 2048, float64 accumulation) passes SPLIT,
and each defect a kernel could have on part of its output -- one tap, the last Cin chunk, the last ragged tile, the 2^-11 scale
of one sample -- fails it.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import tf_ops as T

import numerics as N

SHAPES = {
    # name: (input (G, [D,] H, W, Cin), kernel [k.., Cin, Cout])
    '3x3_cin128': ((3, 10, 21, 128), (3, 3, 128, 32)),
    '1x1_cin64': ((3, 12, 20, 64), (1, 1, 64, 32)),
    '3x3x3_cin32': ((3, 6, 8, 21, 32), (3, 3, 3, 32, 16)),
}


def _operands(name, regime='randn'):
    xs, ws = SHAPES[name]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(xs, generator=g)
    if regime == 'loguniform':
        x = x * 10.0 ** (torch.rand(xs[-1], generator=g) * 6 - 4)
    fan = int(np.prod(ws[:-1]))
    w = torch.randn(ws, generator=g) * (2.0 / fan) ** 0.5
    return x, w


def _emulate(x, w, defect=None):
    """The split convolution in float64 with an optional defect -> (B, .., Cout)."""
    h0, h1 = (t.double() for t in N.emulate_split(x))
    g0, g1 = (t.double() for t in N.emulate_split(w))
    nsp = x.dim() - 2
    keep = torch.ones_like(g0)
    if defect == 'one_tap':
        keep.reshape(-1, *g0.shape[nsp:])[keep.reshape(-1, *g0.shape[nsp:]).shape[0] // 2 - 1] = 0    # an off-centre tap
    elif defect == 'last_cin_chunk':
        keep[..., -16:, :] = 0
    main = T.conv(h0, g0, 1, 'SAME')
    cross = T.conv(h0, g1 * keep, 1, 'SAME') + T.conv(h1, g0 * keep, 1, 'SAME')
    y = main + cross / 2048.0
    if defect == 'ragged_tile':
        # the outputs of the last, partial 16-wide x tile of the last row keep only h0 * g0
        y[..., -1, (y.shape[-2] // 16) * 16:, :] = main[..., -1, (y.shape[-2] // 16) * 16:, :]
    elif defect == 'group_scale':
        y[1] = main[1] + cross[1]                 # sample 1 of the group misses the epilogue's 2^-11
    return y


def _ratio(x, w, defect=None, bar=N.SPLIT):
    got = _emulate(x, w, defect)
    want = N.ref64(T.conv, x, w, 1, 'SAME')
    cnd = N.cond(T.conv, x, w, 1, 'SAME')
    return N.assert_elementwise(got, want, cnd, bar.rel, N.floor_of(w, bar), '%s' % defect)


@pytest.mark.parametrize('regime', ['randn', 'loguniform'])
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_correct_split_passes_the_bar_with_room(name, regime):
    x, w = _operands(name, regime)
    r = _ratio(x, w)
    print('%s %s: correct split err/cond %.2e' % (name, regime, r))
    assert r <= N.SPLIT.rel / 8


@pytest.mark.parametrize('defect', ['one_tap', 'last_cin_chunk', 'ragged_tile', 'group_scale'])
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_each_partial_defect_fails_the_bar(name, defect):
    x, w = _operands(name)
    with pytest.raises(AssertionError, match='err/cond'):
        _ratio(x, w, defect)


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_the_smallest_defect_is_8x_above_the_bar(name):
    """SPLIT.rel is at most 1/8 of the err/cond of the mildest defect (one tap's low pieces dropped)."""
    x, w = _operands(name)
    r = _ratio(x, w, 'one_tap', N.Bar(float('inf'), N.SPLIT.floor))
    print('%s: one tap without its low pieces err/cond %.2e' % (name, r))
    assert N.SPLIT.rel * 8 <= r


def _aanet_case(nv):
    g = torch.Generator().manual_seed(20 + nv)
    X = torch.randn((nv, 2, 5, 12, 8), generator=g)
    ws, wu = (torch.randn((3, 3, 3, 8, 8), generator=g) * (2.0 / 216) ** 0.5 for _ in range(2))
    cnd, spread = N.aanet_cond(X, ws, wu)
    return X, ws, wu, N.aanet64(X, ws, wu), cnd, 2.0 * N.floor_of(torch.cat([ws, wu], -1), N.SPLIT) * spread


def test_aanet64_is_the_oracle_module():
    from oracle import nets
    X, ws, wu, want, _, _ = _aanet_case(5)
    Wd = {'a/attention_activation/weight_unique': wu.double(), 'a/attention_activation/weight_shared': ws.double()}
    ref = nets.attention_aggregation(X.double().permute(1, 2, 3, 4, 0).unsqueeze(0), Wd, 'a')[0]
    assert float((ref - want).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize('nv', [2, 5, 8])
def test_aanet_bound_passes_the_split_and_fails_a_dropped_tap(nv):
    """The AANet module's bound (numerics.aanet_cond): the emulated split score convolutions pass SPLIT with 8x room; one
    tap's low pieces dropped, or plain fp16 operands without the split, fail it."""
    X, ws, wu, want, cnd, floor = _aanet_case(nv)
    good = N.aanet64(X, ws, wu, conv=lambda x, w: _emulate(x.float(), w))
    r = N.assert_elementwise(good, want, cnd, N.SPLIT.rel, floor, 'aanet split')
    print('aanet nv %d: correct split err/cond %.2e' % (nv, r))
    assert r <= N.SPLIT.rel / 8
    for name, conv in (('one_tap', lambda x, w: _emulate(x.float(), w, 'one_tap')),
                       ('fp16', lambda x, w: T.conv(x.half().double(), w.half().double(), 1, 'SAME'))):
        with pytest.raises(AssertionError, match='err/cond'):
            N.assert_elementwise(N.aanet64(X, ws, wu, conv=conv), want, cnd, N.SPLIT.rel, floor, 'aanet ' + name)


@pytest.mark.parametrize('nv,shape', [(5, (2, 3, 12)), (8, (2, 3, 14)), (16, (2, 3, 13))])
def test_the_fp32_aanet_rows_near_max_figure_is_the_rounding_of_the_shared_sum(nv, shape):
    """The near-6e4 regime of the fp32_aanet rows (tests/test_gpu_split_precision.py, the same operands): float64 scores with
    the one add U_n = (R_n - S_n) + S_sum rounded to fp32, as csrc/aanet.hip and the reference form it, give the err / cond the
    rows measure on the GPU (2.8e-5, 2.8e-5, 2.3e-5: tests/numerics.py) and stay inside NEAR_MAX * FP32_MFMA.rel; the softmax of
    R_n - S_n alone, rounded the same way, is four orders below -- the figure is that rounding at the ulp of S_sum, not a kernel's."""
    import test_gpu_split_precision as S
    X = S._input((nv,) + shape + (8,), 61, 'near_max').double()
    ws, wu = S._weights((3, 3, 3, 8, 8), 62), S._weights((3, 3, 3, 8, 8), 63)
    want = N.aanet64(X, ws, wu)
    cnd, _ = N.aanet_cond(X, ws, wu)
    s, r = (T.conv(X, w.double(), 1, 'SAME').clamp(min=0) for w in (ws, wu))
    u32 = ((r - s).float() + s.sum(0, keepdim=True).float()).double()
    with_sum = float((((torch.softmax(u32, 0) * X).sum(0) - want).abs() / cnd).max())
    alone = float((((torch.softmax((r - s).float().double(), 0) * X).sum(0) - want).abs() / cnd).max())
    print('aanet nv %d near 6e4: U rounded to fp32 err/cond %.2e, R - S alone %.2e' % (nv, with_sum, alone))
    assert 2.0e-5 <= with_sum <= N.NEAR_MAX * N.FP32_MFMA.rel
    assert alone <= 1e-7


def test_the_bar_names_the_worst_element():
    want = torch.zeros(2, 3, 4, dtype=torch.float64)
    cnd = torch.ones_like(want)
    got = want.clone().float()
    got[1, 2, 3] = 1e-3
    with pytest.raises(AssertionError, match=r'element \(1, 2, 3\)'):
        N.assert_elementwise(got, want, cnd, 1e-6, 0.0)
    got[1, 2, 3] = float('nan')
    with pytest.raises(AssertionError, match=r'element \(1, 2, 3\)'):
        N.assert_elementwise(got, want, cnd, 1e-6, 0.0)
    got[1, 2, 3] = 5e-7
    assert abs(N.assert_elementwise(got, want, cnd, 1e-6, 0.0) - 5e-7) < 1e-12


def test_split_pieces_are_the_design():
    x = torch.tensor([1.0 + 2.0 ** -20, 3.0e-6, 6.0e4 + 1.0, -0.1, 2.0 ** -20])
    h0, h1 = N.emulate_split(x)
    assert torch.equal(h0, x.half().float())
    rel = ((h0.double() + h1.double() / 2048) - x.double()).abs() / x.double().abs()
    assert float(rel[[0, 2, 3]].max()) <= 2.0 ** -22
    assert float(((h0.double() + h1.double() / 2048) - x.double()).abs().max()) <= 2.0 ** -36 + 2.0 ** -22 * 6.1e4


def test_nan_border_surrounds_a_contiguous_copy():
    t = torch.arange(24.0).reshape(2, 3, 4)
    v = N.nan_bordered(t)
    assert torch.equal(v, t) and v.is_contiguous()
    base = v.untyped_storage()
    full = torch.empty(0).set_(base)
    off = v.storage_offset()
    assert off >= 4096 and bool(full[:off].isnan().all()) and bool(full[off + 24:].isnan().all())
    assert full.numel() - off - 24 >= 4096


def test_the_gpu_table_covers_every_split_family_and_the_fp32_forms():
    import test_gpu_split_precision as S
    assert {r.split for r in S.ROWS if r.bar is N.SPLIT} == {'c16b', 'c3b', 's2b', 'upb', 'c2b', 'c1b', 'btl', 'xb', 'aanet_b'}
    assert all(r.split is None for r in S.ROWS if r.bar is N.FP32_MFMA)
    assert {'xp', 'xp_siblings', 'xp_plane_bias', 'xp_into_plane'} <= {r.family for r in S.ROWS if r.split == 'xb'}
    fp32 = {r.family for r in S.ROWS if r.bar is N.FP32_MFMA}
    assert {'c16', 'tiled', 'xpair_tiled', 'gather', 'xp', 'xp_siblings', 'deconv_up', 'conv2d_lds', 'conv1x1', 'stem',
            'refine_stems', '8to1'} <= fp32
    assert {r.name for r in S.ROWS if r.bar is N.FP32_MFMA and r.family in ('xp', 'xp_siblings')} <= \
        {r.name for r in S.ROWS if r.cfg.get('split16') is False}
    assert len({r.name for r in S.ROWS}) == len(S.ROWS)
    # the rows whose input is formed on load, which run the offset regime too
    assert {r.name for r in S.ROWS if r.lazy} == {'c16b_sum', 'c3b_norm', 's2b_norm', 'c2b_on_load', 'c1b_on_load', 'btl_G2',
                                                  'upb_sum', '8to1_sum', 'xb_siblings_norm', 'xb_siblings_sum',
                                                  'fp32_conv1x1_on_load', 'fp32_conv1x1_on_load_G3', 'fp32_xw_siblings_norm',
                                                  'fp32_xw_siblings_sum', 'fp32_unit_G2', 'fp32_unit_dil2'}


# the convolution entry points conv_dispatch.json names beside ops.conv -> the maker of their rows
ENTRY_POINT_MAKERS = {'conv_siblings': 'siblings_row', 'conv3d_transpose_s2': 'deconv_row', 'conv3d_8to1': 'head_row',
                      'aanet_combine': 'aanet_fp32_row', 'refine_stems': 'refine_stems_row'}
PASSES = ('bn_apply', 'bn_add')          # the materialising passes of the table: no convolution (tests/test_gpu_batch_norm.py)
NO_SPLIT_FORM = ('gather', 'tiled', 'stem', '8to1', 'refine_stems')       # one kernel, whatever split16 says


def fp32_rows_of(event, rows):
    """The rows of the GPU table that hold what one event of a split16=0 dispatch case launches: 'conv:<family>[+]' -> the
    ops.conv rows of that family whose input is (+) / is not formed on load, a named entry point -> the rows of its maker; of
    those, the rows that run under cfg=FP32 or whose family has no split-operand form."""
    if event.startswith('conv:'):
        fam, on_load = event[5:].rstrip('+'), event.endswith('+')
        hits = [r for r in rows if r.maker in ('conv_row', 'stem_row') and r.family == fam and r.lazy == on_load]
    else:
        hits = [r for r in rows if r.maker == ENTRY_POINT_MAKERS[event]]
    return [r for r in hits if r.bar is N.FP32_MFMA and (r.cfg.get('split16') is False or r.family in NO_SPLIT_FORM)]


def _fp32_events():
    import json
    import test_conv_dispatch as CD
    table = json.load(open(CD.GOLDEN))
    cases = [k for k in table if k.endswith('/split16=0')]
    assert len(cases) == 4
    return sorted({e for k in cases for e in table[k].split()} - set(PASSES))


def test_the_fp32_rows_cover_what_the_fp32_path_launches():
    """Every convolution event of the four split16=0 cases of tests/golden/conv_dispatch.json (both pipelines, both sizes)
    has a row of the GPU table that runs the fp32 form it names: a family the fp32 dispatch starts to use fails here until
    it has one."""
    import test_gpu_split_precision as S
    events = _fp32_events()
    assert {'conv:conv1x1+', 'conv:conv2d_lds', 'conv:c16', 'conv:tiled', 'conv:gather', 'conv:xp', 'aanet_combine'} <= set(events)
    for e in events:
        assert e.startswith('conv:') or e in ENTRY_POINT_MAKERS, 'conv_dispatch.json names %r: map it to its row maker' % e
        assert fp32_rows_of(e, S.ROWS), 'no fp32 row of tests/test_gpu_split_precision.py holds %r' % e


@pytest.mark.parametrize('event,names', [('conv:conv1x1+', ('fp32_conv1x1_on_load', 'fp32_conv1x1_on_load_G3')),
                                         ('aanet_combine', tuple('fp32_aanet_nv%d' % n for n in (1, 2, 5, 8, 16)))])
def test_the_coverage_check_sees_a_deleted_row(event, names):
    """Without its rows an event has nothing left: the check above would fail."""
    import test_gpu_split_precision as S
    assert {r.name for r in fp32_rows_of(event, S.ROWS)} == set(names)
    assert not fp32_rows_of(event, [r for r in S.ROWS if r.name not in names])
