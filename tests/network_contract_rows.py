"""One row per ops function behind the network (ops/geometry.py, ops/norm.py, the aggregation of ops/aanet.py, ops/convolution.py and
the single-kernel wrappers of ops/launch.py): what tests/test_gpu_network_contract.py runs under tests/guarded_alloc.py and
tests/test_network_contract_host.py checks for completeness against include/atvsnet_hip.h.  The rows are tests/buffer_contract_rows.py's
`Row`, registered in this module's own ROWS.

Beyond what a row holds there:
    sizes       every size names the entry points it must reach ('entries'): the dispatch of ops/launch.py sends a shape it does not
                like to another kernel without complaint, so a size is a case of a kernel only if the recording proxy saw that kernel
    'cfg'       of a size: the switches of ops.cfg the three runs are made under (tests/guarded_alloc.py weights_under)
    slices(p)   the placed buffers the op writes a part of, and the part (a (lo, hi) channel range or a bool mask): the rest is held
    outputs     may be a function of the size's parameters (a form that writes into a given buffer allocates no output)

Every wide buffer an op writes a slice of is made by `noise`: a different value at every position.  All inputs are finite and of
order one, inside the fp16 range of the split-operand kernels.  Arranged weights are placed under the guard by weights_under; a
statistics result is compared as the columns of its partial sums the header specifies and through ops.bn_params of it.
"""
import collections

import numpy as np
import torch

from buffer_contract_rows import F32, Row

ROWS = collections.OrderedDict()

# ---- the constants the sizes cross (from the sources, as `constants` of the rows say) ----
THREADS = 256                        # workgroup of the element-wise passes (norm.hip, pool.hip, geometry.hip, aanet.hip)
UW = 8                               # softargmin.hip UW: pixels of a row per thread of upsample_softargmin
BATCH_MAP = (128, 256)               # the largest map atvs_transform_depth_batch_supported accepts (h * w <= 32,768) ...
OVER_BATCH_MAP = (129, 256)          # ... and the first it refuses
TILE_C16 = ((3, 7, 15), (4, 8, 16), (5, 9, 17))            # C16_* = B16_* = AB_* = 4 / 8 / 16, W >= 12: one below, at, one above
TILE_XP = ((3, 3, 31), (4, 4, 32), (5, 5, 33))             # XB_TZ/TY/TXV = 4 / 4 / 32, W >= 24
TILE_XW = ((3, 7, 31), (4, 8, 32), (5, 9, 33))             # XW_* = 4 / 8 / 32
TILE_S2_IN = ((2, 6, 29), (3, 7, 31), (5, 9, 33))          # S2_* = 2 / 4 / 16 on the output: outputs (1,3,15), (2,4,16), (3,5,17), Wo >= 8
TILE_UP = ((3, 7, 15), (4, 8, 16), (5, 9, 17))             # UP_TZ/TX = 4 / 16, TY = 32 / NT = 8 (8 channels) | 4 (16 channels)
TILE_81 = ((3, 15, 15), (4, 16, 16), (5, 17, 17))          # C81_* = 4 / 16 / 16
TILE_STEM = ((3, 7, 31), (4, 8, 32), (5, 9, 33))           # ST_TZ/TY/TX = 4 / 8 / 32
MAPS_2D = ((8, 16), (9, 17), (7, 15))                      # conv_plan: H >= 8 and W >= 16 for the LDS-tiled 2-D kernel; (7,15) is below


def Net(name, entries, sizes, **kw):
    return Row(name, entries, sizes, table=ROWS, **kw)


def cases():
    return [(row.name, size) for row in ROWS.values() for size in row.sizes]


def noise(shape, seed, lo=-1.0, hi=1.0):
    """Deterministic float32 values, a different one at (almost) every position."""
    return torch.from_numpy(np.random.RandomState(seed).uniform(lo, hi, tuple(shape)).astype(np.float32))


def kernel(shape, seed):
    """A TF-layout kernel [k.., Cin, Cout] (numpy, host) whose outputs stay of order one."""
    fan = int(np.prod(shape[:-1]))
    return (np.random.RandomState(seed).uniform(-1.0, 1.0, tuple(shape)) * (1.7 / np.sqrt(fan))).astype(np.float32)


def params(G, C, seed):
    """(G,3,C) batch-norm parameters (mean, rstd, beta) of order one."""
    r = np.random.RandomState(seed)
    return torch.from_numpy(np.stack([r.uniform(-0.2, 0.2, (G, C)), r.uniform(0.5, 1.5, (G, C)), r.uniform(-0.3, 0.3, (G, C))], 1).astype(np.float32))


def table(*items):
    """((size name, parameters), ...) -> sizes, names unique."""
    out = collections.OrderedDict()
    for name, p in items:
        assert name not in out, name
        out[name] = p
    return out


def dims(s):
    return 'x'.join(str(v) for v in s)


def planar_mask(ops, K, D, h, w, planes=None):
    """The writable part of a chunk-planar (K, planar_stride) buffer: the D*h*w*8 floats of each plane (of `planes`), never the pad."""
    m = torch.zeros((K, ops.planar_stride(D, h, w)), dtype=torch.bool)
    for k in (range(K) if planes is None else planes):
        m[k, :D * h * w * 8] = True
    return m


def stats_of(ops, st, C, ref, beta=None):
    """[the columns 0..C-1 of a Stats' partial sums, ops.bn_params of it]: the second catches a workgroup that skipped its row."""
    if st is None:
        return [None, None]
    return [st.partial[..., :C], ops.bn_params(st, C, ref, beta)]


STATS, PARAMS = '_stats_buffer: return f((groups, blocks, 2, cpad)', 'params = _new(ref'       # the lines of ops/base.py and ops/norm.py that allocate them
PARTIAL_COLUMNS = ('columns C.. of a [2][16] partial row of an 8-channel layer: "columns 0..7 = channels", header line 272 (the x-pair '
                   'kernels), "[2][16] doubles (columns 0..7)", header line 484 (the stem)')


# =========================================================================================================== ops/geometry.py
def scene(n, h, w, D):
    """cams (n,2,4,4) with every entry filled, (depth_start, depth_interval) as 1-element tensors."""
    import geometry_cases as GC
    cams = GC.general_cams(n, h, w, D)[0].contiguous()
    return cams, cams[0, 1, 3, 0:1].clone(), cams[0, 1, 3, 1:2].clone()


def _homographies(ops, d, place, D):
    return place(ops.get_homographies(d['cams'][0], d['cams'][1], d['ds'], d['di'], D))


def _scene_inputs(p, n=2):
    h, w = p['hw']
    cams, ds, di = scene(n, h, w, p['D'])
    return {'cams': cams, 'ds': ds, 'di': di}


def _scene_shapes(p, n=2):
    return {'cams': ((n, 2, 4, 4), F32), 'ds': ((1,), F32), 'di': ((1,), F32)}


Net('get_homographies', ('atvs_get_homographies',),
    table(*[('D=%d,%s' % (D, 'inverse' if inv else 'metric'), {'D': D, 'hw': (24, 40), 'inverse': inv})
            for D, inv in ((1, True), (32, True), (255, False), (256, True), (257, True))]),
    build=lambda p: dict(_scene_inputs(p), D=p['D'], inverse=p['inverse']), shapes=_scene_shapes,
    run=lambda ops, d, place: ops.get_homographies(d['cams'][0], d['cams'][1], d['ds'], d['di'], d['D'], d['inverse']),
    select=lambda r: [r], names=('homographies',), outputs=('out = _new(left_cam',),
    constants='one thread per depth plane: 1, 32, and 255 | 256 | 257 planes around a 256-thread workgroup')


WARP_HW, WARP_D = (17, 23), 5


def _warp_inputs(p):
    h, w = WARP_HW
    d = _scene_inputs({'hw': WARP_HW, 'D': WARP_D})
    C = p['C']
    d['src'] = noise((h, w, C), 101, 0.05, 0.35)
    if p['mode'] == 1:
        d['ref'] = noise((h, w, C), 102)
    if p.get('out') == 'wide':
        d['out'] = noise((WARP_D, h, w, p['ld']), 103)
    if p.get('out') == 'planar':
        from atvsnet_amd import ops
        d['out'] = noise((C // 8, ops.planar_stride(WARP_D, h, w)), 104)
    d['form'] = dict(p)
    return d


def _warp_shapes(p):
    from atvsnet_amd import ops
    h, w = WARP_HW
    s = dict(_scene_shapes(p), src=((h, w, p['C']), F32))
    if p['mode'] == 1:
        s['ref'] = ((h, w, p['C']), F32)
    if p.get('out') == 'wide':
        s['out'] = ((WARP_D, h, w, p['ld']), F32)
    if p.get('out') == 'planar':
        s['out'] = ((p['C'] // 8, ops.planar_stride(WARP_D, h, w)), F32)
    return s


def _warp_run(ops, d, place):
    f = d['form']
    H = _homographies(ops, d, place, WARP_D)
    r = ops.warp_planes(d['src'], H, out=d.get('out'), c_off=f.get('c_off', 0), mode=f['mode'], ref=d.get('ref'),
                        depth_start=d['ds'] if f['mode'] == 2 else None, depth_interval=d['di'] if f['mode'] == 2 else None,
                        rep=f.get('rep', 1), want_mask=f.get('mask', False), planar=f.get('planar', False), pieces=f.get('pieces', False))
    out, mask = r if f.get('mask') else (r, None)
    if f.get('planar'):
        out = out[..., :WARP_D * WARP_HW[0] * WARP_HW[1] * 8]          # the planes; the pad between them is masked or left out (below)
    return [out, mask]


def _warp_slices(p):
    from atvsnet_amd import ops
    if p.get('out') == 'wide':
        return {'out': (p['c_off'], p['c_off'] + (p['rep'] if p['mode'] == 2 else p['C']))}
    if p.get('out') == 'planar':
        return {'out': planar_mask(ops, p['C'] // 8, WARP_D, *WARP_HW)}
    return {}


_W = ('atvs_get_homographies', 'atvs_warp_planes')
Net('warp_planes', _W, table(
    ('mode 0', {'mode': 0, 'C': 8}), ('mode 0, mask', {'mode': 0, 'C': 5, 'mask': True}), ('mode 1', {'mode': 1, 'C': 8}),
    ('mode 2, rep 16', {'mode': 2, 'C': 1, 'rep': 16}), ('mode 3 (nearest), mask', {'mode': 3, 'C': 4, 'mask': True}),
    ('mode 0 into out[..., 4:12] of 24', {'mode': 0, 'C': 8, 'out': 'wide', 'ld': 24, 'c_off': 4}),
    ('mode 2, rep 16 into out[..., 1:17] of 24', {'mode': 2, 'C': 1, 'rep': 16, 'out': 'wide', 'ld': 24, 'c_off': 1}),
    ('planar, C=16', {'mode': 0, 'C': 16, 'planar': True}), ('planar into a given buffer, C=32', {'mode': 0, 'C': 32, 'planar': True, 'out': 'planar'}),
    ('planar pieces, mode 1, C=16', {'mode': 1, 'C': 16, 'planar': True, 'pieces': True}),
    ('planar pieces into a given buffer, C=16', {'mode': 1, 'C': 16, 'planar': True, 'pieces': True, 'out': 'planar'})),
    build=_warp_inputs, shapes=_warp_shapes, run=_warp_run, select=list, names=('out', 'mask'),
    outputs=lambda p: (() if p.get('out') else ('out = _new(src',)) + (('mask = _new(src',) if p.get('mask') else ()),
    slices=_warp_slices,
    excluded=('the PLANAR_PAD floats behind each chunk plane of an output the op allocates itself: "The pad between the planes is never '
              'written", header line 68 (in a given buffer they are masked as not writable)',),
    constants='a 17 x 23 map (391 pixels: no multiple of the 256-thread workgroup), D = 5; every mode; channel counts 1, 4, 5, 8 and '
              'the planar ones 16, 32; PLANAR_PAD floats between the planes')

Net('build_cost_volume', ('atvs_build_cost_volume',), table(*[('C=%d' % C, {'C': C, 'hw': WARP_HW, 'D': WARP_D}) for C in (4, 8, 32)]),
    build=lambda p: dict(_scene_inputs(p), ref=noise(WARP_HW + (p['C'],), 105), view=noise(WARP_HW + (p['C'],), 106)),
    shapes=lambda p: dict(_scene_shapes(p), ref=(WARP_HW + (p['C'],), F32), view=(WARP_HW + (p['C'],), F32)),
    run=lambda ops, d, place: ops.build_cost_volume(d['ref'], d['view'], _homographies(ops, d, place, WARP_D)),
    select=lambda r: [r], names=('cost volume',), outputs=('out = _new(ref_feature',),
    constants='C % 4 == 0: 4, 8, 32 channels; 391 pixels x 5 planes')


def _wide(p, seed, lead):
    return noise(lead + (p['ld'],), seed)


TILE_SIZES = table(*[('C=%d into [%d:%d] of %d' % (C, off, off + C, ld), {'C': C, 'c_off': off, 'ld': ld, 'hw': WARP_HW, 'D': WARP_D})
                     for C, off, ld in ((1, 0, 1), (1, 3, 8), (3, 5, 8), (8, 8, 24), (12, 4, 16))])

Net('tile_planes', ('atvs_tile_planes',), TILE_SIZES,
    build=lambda p: {'src': noise(WARP_HW + (p['C'],), 107), 'out': _wide(p, 108, (WARP_D,) + WARP_HW), 'c_off': p['c_off']},
    shapes=lambda p: {'src': (WARP_HW + (p['C'],), F32), 'out': ((WARP_D,) + WARP_HW + (p['ld'],), F32)},
    run=lambda ops, d, place: ops.tile_planes(d['src'], d['out'], d['c_off']), select=lambda r: [r], names=('out (whole)',), outputs=(),
    slices=lambda p: {'out': (p['c_off'], p['c_off'] + p['C'])},
    constants='channel counts 1, 3, 8, 12 at offsets 0, 3, 5, 8, 4 of rows of 1, 8, 24, 16 floats')

GEO_SIZES = table(*[('[%d] of %d' % (off, ld), {'c_off': off, 'ld': ld, 'hw': WARP_HW, 'D': WARP_D}) for off, ld in ((0, 1), (0, 4), (3, 4), (16, 24))])

Net('geo_ref_planes', ('atvs_geo_ref_planes',), GEO_SIZES,
    build=lambda p: dict(_scene_inputs(p), depth=noise(WARP_HW, 109, 0.05, 0.35), out=_wide(p, 110, (WARP_D,) + WARP_HW), c_off=p['c_off']),
    shapes=lambda p: dict(_scene_shapes(p), depth=(WARP_HW, F32), out=((WARP_D,) + WARP_HW + (p['ld'],), F32)),
    run=lambda ops, d, place: ops.geo_ref_planes(d['depth'], d['ds'], d['di'], d['out'], d['c_off']), select=lambda r: [r],
    names=('out (whole)',), outputs=(), slices=lambda p: {'out': (p['c_off'], p['c_off'] + 1)},
    constants='one channel at offsets 0, 3, 16 of rows of 1, 4, 24 floats')

Net('geo_volume', ('atvs_geo_volume',),
    table(*[('rep %d at [%d] of %d' % (rep, off, ld), {'c_off': off, 'ld': ld, 'rep': rep, 'hw': WARP_HW, 'D': WARP_D})
            for rep, off, ld in ((1, 0, 2), (1, 1, 4), (16, 0, 17), (16, 3, 24))]),
    build=lambda p: dict(_scene_inputs(p), depth=noise(WARP_HW, 111, 0.05, 0.35), view=noise(WARP_HW, 112, 0.05, 0.35),
                         out=_wide(p, 113, (WARP_D,) + WARP_HW), c_off=p['c_off'], rep=p['rep']),
    shapes=lambda p: dict(_scene_shapes(p), depth=(WARP_HW, F32), view=(WARP_HW, F32), out=((WARP_D,) + WARP_HW + (p['ld'],), F32)),
    run=lambda ops, d, place: ops.geo_volume(d['depth'], d['view'], _homographies(ops, d, place, WARP_D), d['ds'], d['di'], d['out'],
                                             d['c_off'], d['rep']),
    select=lambda r: [r], names=('out (whole)',), outputs=(), slices=lambda p: {'out': (p['c_off'], p['c_off'] + 1 + p['rep'])},
    constants='1 + rep channels, rep 1 and 16 (the reference\'s replicated channel), dense and inside a wider row')

Net('visual_hull', ('atvs_visual_hull',),
    table(('allocated', {'given': False, 'hw': WARP_HW, 'D': WARP_D, 'inverse': True}), ('into out', {'given': True, 'hw': WARP_HW, 'D': WARP_D, 'inverse': True}),
          ('metric', {'given': False, 'hw': WARP_HW, 'D': WARP_D, 'inverse': False})),
    build=lambda p: dict(_scene_inputs(p), ref=noise(WARP_HW, 114, 0.05, 0.35), view=noise(WARP_HW, 115, 0.05, 0.35), inverse=p['inverse'],
                         **({'out': noise((WARP_D,) + WARP_HW, 116)} if p['given'] else {})),
    shapes=lambda p: dict(_scene_shapes(p), ref=(WARP_HW, F32), view=(WARP_HW, F32), **({'out': ((WARP_D,) + WARP_HW, F32)} if p['given'] else {})),
    run=lambda ops, d, place: ops.visual_hull(d['ref'], d['view'], _homographies(ops, d, place, WARP_D), d['ds'], d['di'], d['inverse'], out=d.get('out')),
    select=lambda r: [r], names=('hull',), outputs=lambda p: () if p['given'] else ('out = _new(ref_depth',),
    slices=lambda p: {'out': (0, WARP_HW[1])} if p['given'] else {}, constants='391 pixels x 5 planes; both depth conventions')


def _by_depth_inputs(p):
    h, w = p['hw']
    d = _scene_inputs(dict(p, D=WARP_D))
    d.update(src=noise((h, w, p['C']), 117), depth=noise((h, w), 118, 0.05, 0.35), method=p['method'])
    return d


BY_DEPTH = table(*[('%s, C=%d, %s' % (m, C, dims(hw)), {'method': m, 'C': C, 'hw': hw}) for m, C, hw in
                   (('bilinear', 8, WARP_HW), ('nearest', 1, WARP_HW), ('bilinear', 3, (1, 257)), ('bilinear', 12, (16, 16)))])

Net('warp_by_depth', ('atvs_warp_by_depth',), BY_DEPTH, build=_by_depth_inputs,
    shapes=lambda p: dict(_scene_shapes(p), src=(p['hw'] + (p['C'],), F32), depth=(p['hw'], F32)),
    run=lambda ops, d, place: ops.warp_by_depth(d['src'], d['cams'][0], d['cams'][1], d['depth'], method=d['method']), select=list,
    names=('warped', 'mask'), outputs=('out = _new(src', 'mask = _new(src'), scratch=('ws = _new(src, (12,))',),
    constants='maps of 391, 257 and 256 pixels; channel counts 1, 3, 8, 12; both methods; the 12-float pose workspace is scratch')


def _err_inputs(p):
    d = _by_depth_inputs(p)
    d.update(ref=noise(p['hw'] + (p['C'],), 119), out=noise(p['hw'] + (p['ld'],), 120), c_off=p['c_off'], copy_ref=p['copy_ref'])
    return d


Net('warp_by_depth_err', ('atvs_warp_by_depth_err',),
    table(*[('%s, C=%d at [%d] of %d%s' % (m, C, off, ld, ', copy_ref' if cr else ''),
             {'method': m, 'C': C, 'hw': WARP_HW, 'c_off': off, 'ld': ld, 'copy_ref': cr})
            for m, C, off, ld, cr in (('bilinear', 8, 0, 8, False), ('bilinear', 8, 4, 24, True), ('nearest', 1, 1, 4, True), ('bilinear', 3, 2, 8, False))]),
    build=_err_inputs,
    shapes=lambda p: dict(_scene_shapes(p), src=(p['hw'] + (p['C'],), F32), depth=(p['hw'], F32), ref=(p['hw'] + (p['C'],), F32),
                          out=(p['hw'] + (p['ld'],), F32)),
    run=lambda ops, d, place: ops.warp_by_depth_err(d['src'], d['ref'], d['cams'][0], d['cams'][1], d['depth'], d['out'], d['c_off'],
                                                    d['method'], True, copy_ref=d['copy_ref']),
    select=lambda r: [r], names=('out (whole)',), outputs=(),
    slices=lambda p: {'out': (p['c_off'], p['c_off'] + p['C'] * (2 if p['copy_ref'] else 1))},
    constants='C channels (2 C with copy_ref: "the C channels behind the error map", header line 110) inside rows of 4, 8, 24 floats')

Net('interpolate', ('atvs_interpolate',),
    table(*[('n=%d, C=%d, %s%s' % (n, C, m, ', mask' if k else ''), {'n': n, 'C': C, 'method': m, 'mask': k})
            for n, C, m, k in ((255, 8, 'bilinear', False), (256, 3, 'bilinear', True), (257, 1, 'nearest', True), (1, 12, 'nearest', False))]),
    build=lambda p: {'src': noise(WARP_HW + (p['C'],), 121), 'x': noise((p['n'],), 122, -2.0, WARP_HW[1] + 2.0),
                     'y': noise((p['n'],), 123, -2.0, WARP_HW[0] + 2.0), 'method': p['method'], 'mask': p['mask']},
    shapes=lambda p: {'src': (WARP_HW + (p['C'],), F32), 'x': ((p['n'],), F32), 'y': ((p['n'],), F32)},
    run=lambda ops, d, place: ops.interpolate(d['src'], d['x'], d['y'], d['method'], d['mask']),
    select=lambda r: list(r) if isinstance(r, tuple) else [r, None], names=('out', 'mask'),
    outputs=lambda p: ('out = _new(src',) + (('mask = _new(src',) if p['mask'] else ()),
    constants='255 | 256 | 257 points around a workgroup, and 1; points inside and outside the map')

Net('pixel_grids', ('atvs_pixel_grids',), table(*[(dims(hw), {'hw': hw}) for hw in ((1, 1), (15, 17), (16, 16), (1, 257), WARP_HW)]),
    build=lambda p: {'ref': noise((1,), 124), 'hw': p['hw']}, shapes=lambda p: {'ref': ((1,), F32)},
    run=lambda ops, d, place: ops.pixel_grids(d['ref'], *d['hw']), select=lambda r: [r], names=('grids',), outputs=('out = _new(ref',),
    constants='maps of 1, 255, 256, 257 and 391 pixels')


def _maps_inputs(p):
    h, w = p['hw']
    n = p.get('jobs', 1)
    cams, _, _ = scene(3, h, w, 8)
    maps = noise((n, h, w), 125, 0.05, 0.35)
    maps[:, :min(h, 2), :min(w, 3)] = 0.0                               # invalid depths
    return {'maps': maps, 'cams': cams, 'inverse': p.get('inverse', True)}


Net('transform_depth', ('atvs_transform_depth',),
    table(*[('%s%s' % (dims(hw), '' if inv else ', metric'), {'hw': hw, 'inverse': inv})
            for hw, inv in (((1, 1), True), ((15, 17), True), ((16, 16), True), ((1, 257), True), (WARP_HW, False), (OVER_BATCH_MAP, True))]),
    build=_maps_inputs, shapes=lambda p: {'maps': ((1,) + p['hw'], F32), 'cams': ((3, 2, 4, 4), F32)},
    run=lambda ops, d, place: ops.transform_depth(d['maps'][0], d['cams'][0], d['cams'][1], d['inverse']), select=lambda r: [r],
    names=('out',), outputs=('out = _new(depth',), scratch=('ws = _new(depth, (14,))',),
    constants='the general path of four launches over its 14-float workspace: maps of 1, 255, 256, 257, 391 pixels and the first map '
              'the one-workgroup path refuses (129 x 256)')


def _batch_run(ops, d, place):
    n = d['maps'].shape[0]
    return ops.transform_depth_batch([(d['maps'][i], d['cams'][i % 3], d['cams'][(i + 1) % 3]) for i in range(n)], d['inverse'])


Net('transform_depth_batch', ('atvs_transform_depth_batch', 'atvs_transform_depth'),
    table(*[('%d jobs of %s' % (n, dims(hw)),
             {'hw': hw, 'jobs': n, 'entries': ('atvs_transform_depth_batch',) if (hw != OVER_BATCH_MAP and n > 1) else ('atvs_transform_depth',)})
            for hw in (BATCH_MAP, OVER_BATCH_MAP, (1, 1), WARP_HW) for n in (1, 2, 16)]),
    build=_maps_inputs, shapes=lambda p: {'maps': ((p['jobs'],) + p['hw'], F32), 'cams': ((3, 2, 4, 4), F32)},
    run=_batch_run, select=list, names=tuple('out[%d]' % i for i in range(16)),
    outputs=lambda p: ('outs = [_new(d',) if 'atvs_transform_depth_batch' in p['entries'] else ('out = _new(depth',),
    constants='atvs_transform_depth_batch_supported(h, w) says h * w <= 32,768: 128 x 256 is the largest map it accepts, 129 x 256 the '
              'first it refuses (the single-map launches then); 1, 2 and 16 jobs (one job always takes the single-map path)')

Net('absdiff_mask', ('atvs_absdiff_mask',),
    table(*[('%d pixels, C=%d' % (n, C), {'n': n, 'C': C}) for n, C in ((255, 8), (256, 1), (257, 3), (391, 12), (1, 128))]),
    build=lambda p: {'a': noise((p['n'], p['C']), 126), 'b': noise((p['n'], p['C']), 127), 'mask': (noise((p['n'],), 128) > 0).float()},
    shapes=lambda p: {'a': ((p['n'], p['C']), F32), 'b': ((p['n'], p['C']), F32), 'mask': ((p['n'],), F32)},
    run=lambda ops, d, place: ops.absdiff_mask(d['a'], d['b'], d['mask']), select=lambda r: [r], names=('out',), outputs=('out = _new(a',),
    constants='255 | 256 | 257 pixels; channel counts 1, 3, 8, 12, 128')


def _cost_inputs(p):
    h, w = p['hw']
    _, ds, di = scene(2, h, w, p['D'])
    lead = (p['G'],) if p.get('G') else ()
    return {'cost': noise(lead + (p['D'], h, w), 129, -3.0, 3.0), 'ds': ds, 'di': di, 'G': p.get('G')}


def _cost_shapes(p):
    return {'cost': (((p['G'],) if p.get('G') else ()) + (p['D'],) + p['hw'], F32), 'ds': ((1,), F32), 'di': ((1,), F32)}


Net('softargmin', ('atvs_softargmin',),
    table(*[('%s%s, D=%d' % (dims(hw), ', G=%d' % G if G else '', D), {'hw': hw, 'G': G, 'D': D})
            for hw, G, D in (((15, 17), None, 8), ((16, 16), 3, 8), ((1, 257), 1, 32), (WARP_HW, 3, 5), ((1, 1), None, 1))]),
    build=_cost_inputs, shapes=_cost_shapes, run=lambda ops, d, place: ops.softargmin(d['cost'], d['ds'], d['di'], groups=d['G']),
    select=lambda r: [r], names=('depth',), outputs=('out = _new(cost',), constants='maps of 255, 256, 257, 391 and 1 pixels; G = 1 and 3')

Net('upsample_softargmin', ('atvs_upsample_softargmin',),
    table(*[('%s x%d, D=%d' % (dims(hw), up, D), {'hw': hw, 'up': up, 'D': D})
            for hw, up, D in (((5, 7), 4, 8), ((5, 8), 4, 8), ((5, 9), 4, 5), ((3, 2), 4, 32), ((6, 5), 2, 4))]),
    build=lambda p: dict(_cost_inputs(p), up=p['up']), shapes=_cost_shapes,
    run=lambda ops, d, place: ops.upsample_softargmin(d['cost'], d['ds'], d['di'], d['up']), select=lambda r: [r], names=('depth',),
    outputs=('out = _new(cost',), constants='UW = 8 output pixels of a row per thread (softargmin.hip): output rows of 28, 32, 36, 8 and 10 pixels')


def _prob_inputs(p):
    d = _cost_inputs(p)
    h, w = p['hw']
    lo, step = float(d['ds']), float(d['di'])
    d['depth'] = noise((h * p['up'], w * p['up']), 130, lo - step, lo + (p['D'] + 1) * step)
    d.update(up=p['up'], softmax=p['softmax'])
    return d


Net('probability_map', ('atvs_probability_map',),
    table(*[('%s x%d, softmax %s' % (dims(hw), up, sm), {'hw': hw, 'up': up, 'softmax': sm, 'D': 8})
            for hw, up, sm in (((15, 17), 1, True), ((16, 16), 1, False), ((5, 7), 4, True), ((5, 9), 4, False), ((1, 257), 1, True))]),
    build=_prob_inputs, shapes=lambda p: dict(_cost_shapes(p), depth=((p['hw'][0] * p['up'], p['hw'][1] * p['up']), F32)),
    run=lambda ops, d, place: ops.probability_map(d['cost'], d['depth'], d['ds'], d['di'], d['up'], d['softmax']), select=lambda r: [r],
    names=('probability',), outputs=('out = _new(vol',),
    constants='up_scale 1 and 4, softmax on and off; maps of 255, 256, 257 pixels; depths below, inside and above the sweep')


# =============================================================================================================== ops/norm.py
ROWS_C = ((255, 8), (256, 1), (257, 3), (391, 12), (130, 128))


def _rows_name(G, rows, C):
    return '%s%d rows, C=%d' % ('G=%d, ' % G if G else '', rows, C)


Net('channel_stats', ('atvs_channel_stats',),
    table(*[(_rows_name(G, r, C), {'G': G, 'rows': r, 'C': C}) for G, (r, C) in zip((None, 3, 1, 3, None), ROWS_C)] + [
        ('4099 rows, C=8', {'G': None, 'rows': 4099, 'C': 8})]),
    build=lambda p: {'x': noise(((p['G'],) if p['G'] else ()) + (p['rows'], p['C']), 201), 'G': p['G']},
    shapes=lambda p: {'x': (((p['G'],) if p['G'] else ()) + (p['rows'], p['C']), F32)},
    run=lambda ops, d, place: stats_of(ops, ops.channel_stats(d['x'], d['G']), d['x'].shape[-1], d['x']), select=list,
    names=('partial', 'bn_params of it'), outputs=(STATS,),
    constants='255 | 256 | 257 rows, 4099 rows (several blocks of atvs_channel_stats_num_blocks); C = 1, 3, 8, 12, 128; G = 1 and 3')


def _finalize_inputs(p):
    G, B, cpad = p['G'], p['blocks'], p['C'] * p['fold']
    return {'partial': torch.from_numpy(np.random.RandomState(202).uniform(0.5, 2.0, (G, B, 2, cpad))),
            'beta': noise((p['C'],), 203) if p['beta'] else None, 'form': dict(p)}


def _finalize_run(ops, d, place):
    f = d['form']
    st = ops.Stats()
    st.partial, st.blocks, st.cpad, st.count, st.groups, st.fold = d['partial'], f['blocks'], f['C'] * f['fold'], 1000 * f['fold'], f['G'], f['fold']
    ref = d['partial'].new_empty((1,), dtype=torch.float32)
    return ops.bn_params(st, f['C'], ref, d['beta'])


Net('bn_params', ('atvs_bn_finalize',),
    table(*[('G=%d, %d blocks, C=%d, fold %d, beta %s' % (G, B, C, fold, beta), {'G': G, 'blocks': B, 'C': C, 'fold': fold, 'beta': beta})
            for G, B, C, fold, beta in ((1, 1, 8, 1, False), (1, 255, 8, 1, True), (3, 256, 16, 1, True), (1, 257, 8, 8, False),
                                        (3, 7, 12, 2, True), (1, 40, 128, 1, False), (1, 5, 1, 1, True), (3, 1, 3, 1, False))]),
    build=_finalize_inputs,
    shapes=lambda p: dict({'partial': ((p['G'], p['blocks'], 2, p['C'] * p['fold']), torch.float64)}, **({'beta': ((p['C'],), F32)} if p['beta'] else {})),
    run=_finalize_run, select=lambda r: [r], names=('params',), outputs=(PARAMS,),
    constants='1, 255 | 256 | 257 rows of partial sums; fold 1, 2 and 8 (the fused transposed convolution\'s classes); beta given or NULL; '
              'G = 1 and 3; the flag word is ops.nonfinite_flag\'s pooled buffer, made before the guarded blocks (warm)')


def _apply_inputs(p):
    G = p['G']
    lead = (G,) if G else ()
    d = {'x': noise(lead + (p['rows'], p['ld']), 204), 'params': params(G or 1, p['C'], 205), 'form': dict(p)}
    if not G:
        d['params'] = d['params'][0].contiguous()
    if p['dest'] == 'out':
        d['out'] = noise(lead + (p['rows'], p['ld']), 206)
    return d


def _apply_run(ops, d, place):
    f = d['form']
    if f['dest'] == 'slice':
        return ops.bn_apply(d['x'], d['params'], f['relu'], C=f['C'], c_off=f['c_off'])
    return ops.bn_apply(d['x'], d['params'], f['relu'], out=d.get('out'))


Net('bn_apply', ('atvs_bn_apply',),
    table(*[('%s, %s%s' % (_rows_name(G, r, C), dest if dest != 'slice' else 'in place on [%d:%d] of %d' % (off, off + C, ld), ', relu' if relu else ''),
             {'G': G, 'rows': r, 'C': C, 'ld': ld, 'c_off': off, 'dest': dest, 'relu': relu})
            for G, r, C, ld, off, dest, relu in ((None, 255, 8, 8, 0, 'out', True), (3, 256, 1, 1, 0, 'in place', False), (None, 257, 3, 8, 2, 'slice', True),
                                                 (3, 391, 12, 32, 20, 'slice', False), (None, 130, 128, 128, 0, 'out', True), (1, 257, 8, 24, 0, 'slice', True))]),
    build=_apply_inputs,
    shapes=lambda p: dict({'x': ((((p['G'],) if p['G'] else ()) + (p['rows'], p['ld'])), F32), 'params': (((p['G'], 3, p['C']) if p['G'] else (3, p['C'])), F32)},
                          **({'out': ((((p['G'],) if p['G'] else ()) + (p['rows'], p['ld'])), F32)} if p['dest'] == 'out' else {})),
    run=_apply_run, select=lambda r: [r], names=('y (whole)',), outputs=(),
    slices=lambda p: {'out': (0, p['ld'])} if p['dest'] == 'out' else {'x': (p['c_off'], p['c_off'] + p['C'])},
    constants='255 | 256 | 257 rows; C = 1, 3, 8, 12, 128; into out, in place, and a channel slice in place inside rows of 8, 24, 32 floats')

Net('batch_norm', ('atvs_channel_stats', 'atvs_bn_finalize', 'atvs_bn_apply'),
    table(*[(_rows_name(G, r, C) + (', in place' if ip else ''), {'G': G, 'rows': r, 'C': C, 'inplace': ip})
            for (G, ip), (r, C) in zip(((None, False), (3, True), (1, False), (3, False), (None, True)), ROWS_C)]),
    build=lambda p: {'x': noise(((p['G'],) if p['G'] else ()) + (p['rows'], p['C']), 207), 'beta': noise((p['C'],), 208), 'G': p['G'], 'inplace': p['inplace']},
    shapes=lambda p: {'x': (((p['G'],) if p['G'] else ()) + (p['rows'], p['C']), F32), 'beta': ((p['C'],), F32)},
    run=lambda ops, d, place: ops.batch_norm(d['x'], beta=d['beta'], relu=True, inplace=d['inplace'], groups=d['G']), select=lambda r: [r],
    names=('y',), outputs=lambda p: (STATS, PARAMS) + (() if p['inplace'] else ('out=(x if inplace else _new',)),
    slices=lambda p: {'x': (0, p['C'])} if p['inplace'] else {},
    constants='as channel_stats; the statistics partials are written by one launch and read by the next')


def _bn_add_inputs(p):
    G, C, n = p['G'], p['C'], p['items']
    shape = (G, p['rows'], C)
    d = {'x%d' % i: noise(shape, 210 + i) for i in range(n)}
    for i in range(n):
        if p['pending'][i]:
            d['p%d' % i] = params(G, C, 220 + i)
    if p['plus']:
        d['plus'] = noise(shape[1:], 230)
    d['form'] = dict(p)
    return d


def _bn_add_shapes(p):
    shape = (p['G'], p['rows'], p['C'])
    s = {'x%d' % i: (shape, F32) for i in range(p['items'])}
    s.update({'p%d' % i: ((p['G'], 3, p['C']), F32) for i in range(p['items']) if p['pending'][i]})
    if p['plus']:
        s['plus'] = (shape[1:], F32)
    return s


def _bn_add_run(ops, d, place):
    f = d['form']
    items = [ops.PendingBN(d['x%d' % i], d['p%d' % i], relu=bool(i % 2 == 0)) if f['pending'][i] else d['x%d' % i] for i in range(f['items'])]
    if f['plus']:
        return list(ops.bn_add(items, plus=d['plus'], keep_sum=f['keep']))
    return [ops.bn_add(items), None]


Net('bn_add', ('atvs_bn_add', 'atvs_bn_add_plus'),
    table(*[('%d items (%s pending), %s%s' % (n, ''.join('01'[v] for v in pend), _rows_name(G, r, C), (', plus' + ('' if keep else ', the sum not kept')) if plus else ''),
             {'items': n, 'pending': pend, 'G': G, 'rows': r, 'C': C, 'plus': plus, 'keep': keep, 'entries': ('atvs_bn_add_plus' if plus else 'atvs_bn_add',)})
            for n, pend, G, r, C, plus, keep in ((2, (1, 1), 1, 255, 8, False, True), (3, (1, 0, 1), 3, 256, 12, False, True), (2, (1, 0), 3, 257, 128, False, True),
                                                 (2, (1, 1), 1, 257, 8, True, True), (3, (1, 1, 1), 3, 255, 16, True, True), (2, (1, 1), 3, 391, 8, True, False))]),
    build=_bn_add_inputs, shapes=_bn_add_shapes, run=_bn_add_run, select=list, names=('sum', 'plus + sum'),
    outputs=lambda p: ('out = _new(xs[0]',) + (('out2 = out if not keep_sum',) if (p['plus'] and p['keep']) else ()),
    constants='two and three items, pending and final mixed; C % 4 == 0: 8, 12, 16, 128; 255 | 256 | 257 rows; plus, and plus without '
              'the sum ("y may be NULL", header line 554)')

Net('add_n', ('atvs_add_n',),
    table(*[('%d tensors of %d%s' % (n, e, ', into out' if given else ''), {'n': n, 'elems': e, 'given': given})
            for n, e, given in ((2, 1020, False), (3, 1024, False), (4, 1028, True), (2, 4, True), (5, 1023, False))]),
    build=lambda p: dict({'t%d' % i: noise((p['elems'],), 240 + i) for i in range(p['n'])}, n=p['n'], **({'out': noise((p['elems'],), 250)} if p['given'] else {})),
    shapes=lambda p: dict({'t%d' % i: ((p['elems'],), F32) for i in range(p['n'])}, **({'out': ((p['elems'],), F32)} if p['given'] else {})),
    run=lambda ops, d, place: ops.add_n([d['t%d' % i] for i in range(d['n'])], out=d.get('out')), select=lambda r: [r], names=('sum',),
    outputs=lambda p: () if (p['given'] and p['n'] <= 3) else ('dst = out if',), slices=lambda p: {'out': (0, p['elems'])} if p['given'] else {},
    constants='two to five tensors (three per launch at most, then one more per launch); 1020 | 1024 | 1028 elements around 256 float4s, 4, 1023')

Net('avg_pool_same', ('atvs_avg_pool_same',),
    table(*[('%s%s, C=%d, pool %d stride %d' % ('G=%d, ' % G if G else '', dims(hw), C, k, s), {'G': G, 'hw': hw, 'C': C, 'pool': k, 'stride': s})
            for G, hw, C, k, s in ((None, (15, 17), 8, 4, 4), (3, (16, 16), 12, 8, 8), (1, (31, 40), 128, 16, 16), (None, (9, 13), 3, 2, 2), (3, (5, 7), 1, 8, 8))]),
    build=lambda p: {'x': noise(((p['G'],) if p['G'] else ()) + p['hw'] + (p['C'],), 251), 'form': dict(p)},
    shapes=lambda p: {'x': (((p['G'],) if p['G'] else ()) + p['hw'] + (p['C'],), F32)},
    run=lambda ops, d, place: ops.avg_pool_same(d['x'], d['form']['pool'], d['form']['stride'], d['form']['G']), select=lambda r: [r], names=('y',),
    outputs=('y = _new(x',), scratch=('ws = _new(x',),
    constants='windows of 2, 4, 8, 16 over maps that are and are not multiples of them (a partial last window); C = 1, 3, 8, 12, 128; its workspace is scratch')

Net('resize_bilinear', ('atvs_resize_bilinear',),
    table(*[('%s%s -> %s, C=%d%s' % ('G=%d, ' % G if G else '', dims(hw), dims(to), C, ' at [%d] of %d' % (off, ld) if ld else ''),
             {'G': G, 'hw': hw, 'to': to, 'C': C, 'ld': ld, 'c_off': off})
            for G, hw, to, C, ld, off in ((None, (4, 5), (15, 17), 8, None, 0), (3, (2, 3), (16, 16), 12, 32, 8), (1, (1, 1), (9, 13), 3, 8, 5),
                                          (None, (8, 10), (31, 40), 32, 128, 96), (3, (5, 7), (5, 7), 1, None, 0))]),
    build=lambda p: dict({'x': noise(((p['G'],) if p['G'] else ()) + p['hw'] + (p['C'],), 252), 'form': dict(p)},
                         **({'out': noise(((p['G'],) if p['G'] else ()) + p['to'] + (p['ld'],), 253)} if p['ld'] else {})),
    shapes=lambda p: dict({'x': (((p['G'],) if p['G'] else ()) + p['hw'] + (p['C'],), F32)},
                          **({'out': (((p['G'],) if p['G'] else ()) + p['to'] + (p['ld'],), F32)} if p['ld'] else {})),
    run=lambda ops, d, place: ops.resize_bilinear(d['x'], d['form']['to'], out=d.get('out'), c_off=d['form']['c_off'], groups=d['form']['G']),
    select=lambda r: [r], names=('y (whole)',), outputs=lambda p: () if p['ld'] else ('y = _new(x',),
    slices=lambda p: {'out': (p['c_off'], p['c_off'] + p['C'])} if p['ld'] else {},
    constants='maps of 255, 256, 117, 1240 and 35 pixels from smaller ones and from 1 x 1; a channel slice of rows of 8, 32, 128 floats')

Net('copy_channels', ('atvs_copy_channels',),
    table(*[('%d rows, %d of %d at %d -> %d at %d' % (r, C, ls, so, ld, do), {'rows': r, 'C': C, 'ls': ls, 'so': so, 'ld': ld, 'do': do})
            for r, C, ls, so, ld, do in ((255, 8, 8, 0, 24, 8), (256, 1, 4, 3, 1, 0), (257, 3, 8, 2, 8, 5), (391, 12, 16, 4, 32, 20), (130, 128, 128, 0, 128, 0))]),
    build=lambda p: {'src': noise((p['rows'], p['ls']), 254), 'dst': noise((p['rows'], p['ld']), 255), 'form': dict(p)},
    shapes=lambda p: {'src': ((p['rows'], p['ls']), F32), 'dst': ((p['rows'], p['ld']), F32)},
    run=lambda ops, d, place: ops.copy_channels(d['src'], d['dst'], d['form']['C'], d['form']['so'], d['form']['do']), select=lambda r: [r],
    names=('dst (whole)',), outputs=(), slices=lambda p: {'dst': (p['do'], p['do'] + p['C'])},
    constants='255 | 256 | 257 rows; C = 1, 3, 8, 12, 128 from and into wider rows at aligned and unaligned offsets')

Net('stack', ('atvs_stack', 'atvs_copy_channels'),
    table(*[('%d tensors of %d' % (n, e), {'n': n, 'elems': e, 'entries': ('atvs_stack',) if (n <= 16 and e % 4 == 0) else ('atvs_copy_channels',)})
            for n, e in ((1, 4), (2, 1020), (16, 1024), (17, 1028), (3, 1023))]),
    build=lambda p: {'t': noise((p['n'], 1, p['elems']), 256)}, shapes=lambda p: {'t': ((p['n'], 1, p['elems']), F32)},
    run=lambda ops, d, place: ops.stack([d['t'][i] for i in range(d['t'].shape[0])], dim=1), select=lambda r: [r], names=('stacked',),
    outputs=('out = _new(tensors[0]',),
    constants='1, 2, 16 tensors in one launch; 17 tensors and 1023 elements (no multiple of 4) take atvs_copy_channels')

Net('concat_channels', ('atvs_copy_channels',),
    table(*[('%d rows of %s' % (r, '+'.join(str(c) for c in cs)), {'rows': r, 'cs': cs}) for r, cs in ((255, (8, 8)), (257, (1, 3, 12)), (256, (128, 8, 1)))]),
    build=lambda p: {'t%d' % i: noise((p['rows'], c), 257 + i) for i, c in enumerate(p['cs'])},
    shapes=lambda p: {'t%d' % i: ((p['rows'], c), F32) for i, c in enumerate(p['cs'])},
    run=lambda ops, d, place: ops.concat_channels([d[k] for k in sorted(d)]), select=lambda r: [r], names=('concat',), outputs=('out = _new(tensors[0]',),
    constants='255 | 256 | 257 rows; parts of 1, 3, 8, 12, 128 channels at the offsets they add up to')


# ============================================================================================== the aggregation of ops/aanet.py
def _views_inputs(p):
    nv, V = p['nv'], p['V']
    return {'srs': noise((nv, V, 16), 301, 0.0, 2.0), 'xs': noise((nv, V, 8), 302), **({'out': noise((V, 8), 303)} if p.get('given') else {})}


def _views_shapes(p):
    return dict({'srs': ((p['nv'], p['V'], 16), F32), 'xs': ((p['nv'], p['V'], 8), F32)}, **({'out': ((p['V'], 8), F32)} if p.get('given') else {}))


def _each(t):
    return [t[i] for i in range(t.shape[0])]


VIEW_SIZES = [(1, 255, False), (2, 256, False), (3, 257, True), (5, 391, False), (16, 64, True)]

Net('aanet_combine', ('atvs_aanet_combine',),
    table(*[('%d views, V=%d%s' % (nv, V, ', into out' if g else ''), {'nv': nv, 'V': V, 'given': g}) for nv, V, g in VIEW_SIZES]),
    build=_views_inputs, shapes=_views_shapes, run=lambda ops, d, place: ops.aanet_combine(_each(d['srs']), _each(d['xs']), out=d.get('out')),
    select=lambda r: [r], names=('out',), outputs=lambda p: () if p['given'] else ('out = _new(xs[0]',),
    slices=lambda p: {'out': (0, 8)} if p['given'] else {}, constants='1, 2, 3, 5 and 16 (the most) views; 255 | 256 | 257 voxels')


def _partial_run(ops, d, place):
    srs, xs = _each(d['srs']), _each(d['xs'])
    ssum = place(ops.aanet_partial(srs, xs, 0))
    umax = place(ops.aanet_partial(srs, xs, 1, ssum=ssum))
    return [ssum, umax, ops.aanet_partial(srs, xs, 2, ssum=ssum, umax=umax)]


Net('aanet_partial', ('atvs_aanet_partial',), table(*[('%d views, V=%d' % (nv, V), {'nv': nv, 'V': V}) for nv, V, _ in VIEW_SIZES]),
    build=_views_inputs, shapes=_views_shapes, run=_partial_run, select=list, names=('stage 0: sum S', 'stage 1: max U', 'stage 2: [sum e; sum e X]'),
    outputs=('out = _new(xs[0]',), constants='the three stages, ssum and umax passed on; views and voxels as aanet_combine')

Net('divide', ('atvs_divide',), table(*[('n=%d' % n, {'n': n}) for n in (4, 1020, 1024, 1028, 3128)]),
    build=lambda p: {'num': noise((p['n'],), 304), 'den': noise((p['n'],), 305, 0.5, 2.0)},
    shapes=lambda p: {'num': ((p['n'],), F32), 'den': ((p['n'],), F32)}, run=lambda ops, d, place: ops.divide(d['num'], d['den']),
    select=lambda r: [r], names=('out',), outputs=('out = _new(num',), constants='n % 4 == 0: 1020 | 1024 | 1028 around 256 float4s, 4, 3128')


def _fused_run(ops, d, place):
    xs = _each(d['xs'])
    assert ops.aanet_fused_ok(xs), 'the one-launch AANet module refuses this size'
    return ops.aanet_fused(xs, 'aanet', d['w_shared'], d['w_unique'])


Net('aanet_fused', ('atvs_aanet_b_f32',),
    table(*[('%d views of %s' % (nv, dims(s)), {'nv': nv, 'shape': s}) for nv, s in zip((1, 2, 4, 5, 8), TILE_C16 + ((4, 9, 12), (1, 1, 13)))]),
    build=lambda p: {'xs': noise((p['nv'],) + p['shape'] + (8,), 306), 'w_shared': kernel((3, 3, 3, 8, 8), 307), 'w_unique': kernel((3, 3, 3, 8, 8), 308)},
    shapes=lambda p: {'xs': ((p['nv'],) + p['shape'] + (8,), F32)}, run=_fused_run, select=lambda r: [r], names=('out',), outputs=('out = _new(xs[0]',),
    constants='AB_* = 4 / 8 / 16 tiles with W >= 12 (aanet_fused_ok): one below, at and one above per axis, W = 12 and 13, D = H = 1; '
              'nv = 1, 2, 4, 5, 8: five views and more take the running-softmax path; the arranged weights lie under the guard')


# ============================================================================================================ convolutions
FAMILY_ENTRY = {
    'conv2d_lds': 'atvs_conv2d_lds_f32', 'conv2d_b': 'atvs_conv2d_b_f32', 'conv2d_b_s2': 'atvs_conv2d_b_s2_f32', 'conv1x1': 'atvs_conv1x1_f32',
    'conv1x1_b': 'atvs_conv1x1_b_f32', 'stem': 'atvs_conv_stem_f32', 'c3b': 'atvs_conv3d_b_f32', 'c3b_norm': 'atvs_conv3d_b_norm_f32',
    'c16b': 'atvs_conv_c16b_f32', 'c16b_sum': 'atvs_conv_c16b_sum_f32', 'c16': 'atvs_conv_c16_f32', 's2b': 'atvs_conv3d_s2b_f32',
    's2b_norm': 'atvs_conv3d_s2b_norm_f32', 'xp/xb': 'atvs_conv_xb_f32', 'xp/xw': 'atvs_conv_xw_f32', 'xpair_tiled': 'atvs_conv_tiled_f32',
    'tiled': 'atvs_conv_tiled_f32', 'gather': 'atvs_conv_mfma_f32'}
PLAN_FAMILY = {'conv2d_b': 'conv2d_lds', 'conv1x1_b': 'conv1x1', 'xp/xb': 'xp', 'xp/xw': 'xp'}
FP32 = {'split16': False}


def conv_case(family, shape, cin, cout, G=1, k=3, stride=1, dilation=1, pad=None, bias=False, relu=False, residual=False, plane_bias=False,
              stats=True, out=None, lazy=None, cfg=None, tile_y=None):
    """One size of the `conv` row.  out = (row length, channel offset) of a given wider output; lazy: None | 'bn' | 'sum' | 'bn+sum'."""
    p = dict(family=family, shape=tuple(shape), cin=cin, cout=cout, G=G, k=k, stride=stride, dilation=dilation, pad=pad, bias=bias, relu=relu,
             residual=residual, plane_bias=plane_bias, stats=stats, out=out, lazy=lazy, cfg=dict(cfg or {}), tile_y=tile_y)
    # (with fused_finalize the last workgroup of the launch writes the parameters itself: no finalize launch follows)
    p['entries'] = (FAMILY_ENTRY[family],) + (('atvs_bn_finalize',) if (stats and not p['cfg'].get('fused_finalize')) else ())
    forms = [n for n in ('bias', 'relu', 'residual', 'plane_bias') if p[n]] + (['no stats'] if not stats else []) + \
        (['into [%d] of %d' % (out[1], out[0])] if out else []) + (['on load: %s' % lazy] if lazy else []) + \
        (['stride %d' % stride] if stride != 1 else []) + (['dilation %d' % dilation] if dilation != 1 else []) + \
        (['k=%d' % k] if k != 3 else []) + (['%s=%s' % kv for kv in sorted(p['cfg'].items()) if kv[0] != 'split_off'] if cfg else [])
    name = '%s: G=%d, %s, %d->%d%s' % (family, G, dims(shape), cin, cout, ''.join(', ' + f for f in forms))
    return name, p


def conv_outs(p):
    from atvsnet_amd import ops
    nsp = len(p['shape'])
    ks = (1,) * (3 - nsp) + (p['k'],) * nsp
    ins = (1,) * (3 - nsp) + p['shape']
    return ops.conv_geometry(ins, ks, p['stride'], p['dilation'], p['pad'] if p['pad'] else 'SAME', nsp)[1][3 - nsp:]


def _conv_inputs(p):
    G, cin, cout, nsp = p['G'], p['cin'], p['cout'], len(p['shape'])
    outs = conv_outs(p)
    d = {'x': noise((G,) + p['shape'] + (cin,), 401), 'w': kernel((p['k'],) * nsp + (cin, cout), 402), 'form': dict(p)}
    if p['bias']:
        d['bias'] = noise((cout,), 403)
    if p['residual']:
        d['residual'] = noise((G,) + outs + (cout,), 404)
    if p['plane_bias']:
        d['plane_bias'] = noise((G,) + outs[1:] + (3 * cout,), 405)
    if p['out']:
        d['out'] = noise((G,) + outs + (p['out'][0],), 406)
    if p['lazy'] and 'bn' in p['lazy']:
        d['in_params'] = params(G, cin, 407)
    if p['lazy'] and 'sum' in p['lazy']:
        d['x1'], d['params1'] = noise((G,) + p['shape'] + (cin,), 408), params(G, cin, 409)
    return d


def _conv_shapes(p):
    d = _conv_inputs(p)
    return {k: (tuple(v.shape), v.dtype) for k, v in d.items() if isinstance(v, torch.Tensor)}


def _conv_run(ops, d, place):
    f = d['form']
    nsp = len(f['shape'])
    plan = ops.conv_plan(f['shape'], f['k'], f['cin'], f['cout'], f['stride'], f['dilation'], f['pad'] if f['pad'] else 'SAME', f['bias'], f['residual'],
                         f['plane_bias'], f['out'], 'sum' if (f['lazy'] and 'sum' in f['lazy']) else f['lazy'])
    assert plan.family == PLAN_FAMILY.get(f['family'], f['family']), 'conv_plan sends this size to %r' % (plan.family,)
    assert not f['lazy'] or plan.on_load, 'conv_plan does not form this lazy input on load'
    if f['tile_y']:
        assert ops.tiled_tile_y(f['shape'][1], f['shape'][2], f['cout']) == f['tile_y']
    r = ops.conv(d['x'], 'layer', d['w'], stride=f['stride'], dilation=f['dilation'], explicit_pad=f['pad'], bias=d.get('bias'),
                 residual=d.get('residual'), relu=f['relu'], want_stats=f['stats'], out=d.get('out'), y_coff=f['out'][1] if f['out'] else 0,
                 plane_bias=d.get('plane_bias'), groups=f['G'], in_params=d.get('in_params'), in_relu=bool(f['lazy']),
                 in_sum=(d['x1'], d['params1'], True) if 'x1' in d else None)
    y, st = r if f['stats'] else (r, None)
    assert nsp in (2, 3)
    tickets = None
    if f['cfg'].get('fused_finalize') and not y.is_meta:
        # the arrival ticket "must be zero before the layer's first launch and is left at zero" (header line 238): the whole pooled
        # buffer the word was taken from, which lives outside the guarded blocks
        assert st.params is not None
        tickets = ops._fin_pool[str(y.device)][0]
    return [y] + stats_of(ops, st, f['cout'], y) + [tickets]


_S = {'split_off': ('c2b',)}
_2D = [
    conv_case('conv2d_lds', MAPS_2D[0], 16, 32, bias=True, relu=True, cfg=_S), conv_case('conv2d_lds', MAPS_2D[1], 32, 64, G=3, residual=True, cfg=_S),
    conv_case('conv2d_lds', (17, 33), 48, 32, out=(64, 16), stats=False, cfg=_S), conv_case('conv2d_lds', (13, 19), 16, 128, dilation=2, bias=True, cfg=_S),
    conv_case('conv2d_lds', (16, 24), 64, 128, G=3, dilation=4, relu=True, cfg=_S),
    conv_case('conv2d_b', MAPS_2D[0], 32, 32, bias=True, relu=True), conv_case('conv2d_b', MAPS_2D[1], 64, 64, G=3, residual=True, lazy='bn'),
    conv_case('conv2d_b', (17, 33), 32, 128, out=(192, 32), dilation=2, lazy='bn'), conv_case('conv2d_b', (2, 2), 32, 32, G=3, bias=True),
    conv_case('conv2d_b', (3, 5), 128, 32, relu=True, lazy='bn'), conv_case('conv2d_b', MAPS_2D[2], 64, 32, stats=False), conv_case('conv2d_b', (16, 24), 128, 128, dilation=4),
    conv_case('conv2d_b_s2', (16, 32), 32, 64, pad=((1, 1), (1, 1)), stride=2, bias=True, relu=True),
    conv_case('conv2d_b_s2', (18, 34), 64, 64, G=3, pad=((1, 1), (1, 1)), stride=2), conv_case('conv2d_b_s2', (34, 66), 128, 64, pad=((1, 1), (1, 1)), stride=2, stats=False),
    conv_case('conv1x1', (15, 17), 16, 32, k=1, bias=True, relu=True), conv_case('conv1x1', (16, 16), 48, 64, G=3, k=1, residual=True, lazy='bn'),
    conv_case('conv1x1', (1, 257), 16, 128, k=1, out=(160, 32), stats=False), conv_case('conv1x1', (1, 1), 48, 32, k=1, G=3),
    conv_case('conv1x1_b', (15, 17), 32, 32, k=1, bias=True, relu=True), conv_case('conv1x1_b', (16, 16), 64, 64, G=3, k=1, residual=True, lazy='bn'),
    conv_case('conv1x1_b', (1, 257), 128, 128, k=1, out=(160, 32), stats=False), conv_case('conv1x1_b', (1, 1), 32, 64, k=1, G=3),
    conv_case('conv1x1_b', (9, 14), 32, 32, k=1), conv_case('conv1x1_b', (8, 16), 128, 32, k=1, lazy='bn'), conv_case('conv1x1_b', (3, 43), 64, 128, k=1, bias=True)]
_OFF = lambda *names: {'split_off': tuple(names)}          # noqa: E731
_3D = [
    conv_case('stem', TILE_STEM[0], 1, 8, plane_bias=True), conv_case('stem', TILE_STEM[1], 2, 8, G=3, relu=True, out=(32, 8)),
    conv_case('stem', TILE_STEM[2], 2, 8, plane_bias=True, stats=False, out=(32, 24)), conv_case('stem', (1, 1, 1), 1, 8),
    conv_case('c3b', TILE_C16[0], 16, 32, bias=True, relu=True), conv_case('c3b', TILE_C16[1], 32, 64, G=3), conv_case('c3b', TILE_C16[2], 48, 32, out=(64, 32), stats=False),
    conv_case('c3b', (1, 1, 12), 64, 64, bias=True), conv_case('c3b_norm', TILE_C16[0], 16, 32, lazy='bn', bias=True), conv_case('c3b_norm', TILE_C16[2], 32, 64, G=3, lazy='bn', relu=True),
    conv_case('c3b_norm', TILE_C16[1], 64, 32, lazy='bn', out=(64, 0), stats=False),
    conv_case('c16b', TILE_C16[0], 8, 16, bias=True, relu=True), conv_case('c16b', TILE_C16[1], 16, 16, G=3), conv_case('c16b', TILE_C16[2], 8, 16, out=(32, 16), stats=False),
    conv_case('c16b', (1, 1, 12), 16, 16), conv_case('c16b_sum', TILE_C16[0], 16, 16, lazy='bn', bias=True), conv_case('c16b_sum', TILE_C16[1], 16, 16, G=3, lazy='sum', relu=True),
    conv_case('c16b_sum', TILE_C16[2], 16, 16, lazy='bn+sum', out=(32, 8), stats=False),
    conv_case('c16', TILE_C16[0], 8, 16, bias=True, relu=True, cfg=_OFF('c16b')), conv_case('c16', TILE_C16[1], 16, 16, G=3, cfg=_OFF('c16b')),
    conv_case('c16', TILE_C16[2], 32, 16, out=(32, 16), stats=False), conv_case('c16', TILE_C16[1], 16, 32, bias=True, cfg=_OFF('c3b')),
    conv_case('c16', TILE_C16[2], 64, 32, G=3, relu=True, cfg=_OFF('c3b')), conv_case('c16', (1, 1, 12), 48, 32, cfg=_OFF('c3b')),
    conv_case('s2b', TILE_S2_IN[0], 16, 32, stride=2, bias=True, relu=True), conv_case('s2b', TILE_S2_IN[1], 32, 64, G=3, stride=2),
    conv_case('s2b', TILE_S2_IN[2], 16, 64, stride=2, out=(96, 32), stats=False), conv_case('s2b_norm', TILE_S2_IN[1], 16, 32, stride=2, lazy='bn'),
    conv_case('s2b_norm', TILE_S2_IN[2], 32, 32, G=3, stride=2, lazy='bn', bias=True, relu=True),
    conv_case('xp/xb', TILE_XP[0], 8, 8, bias=True, relu=True), conv_case('xp/xb', TILE_XP[1], 16, 8, G=3, plane_bias=True), conv_case('xp/xb', TILE_XP[2], 32, 8, out=(32, 8), stats=False),
    conv_case('xp/xb', (1, 1, 24), 8, 8), conv_case('xp/xb', (3, 17, 25), 64, 8, plane_bias=True, bias=True),
    conv_case('xp/xw', TILE_XW[0], 8, 8, bias=True, relu=True, cfg=FP32), conv_case('xp/xw', TILE_XW[1], 16, 8, G=3, plane_bias=True, cfg=FP32),
    conv_case('xp/xw', TILE_XW[2], 32, 8, out=(32, 8), stats=False, cfg=FP32), conv_case('xp/xw', (1, 1, 24), 8, 8, cfg=FP32),
    conv_case('xpair_tiled', (4, 8, 24), 8, 8, residual=True, bias=True), conv_case('xpair_tiled', (5, 17, 25), 16, 8, G=3, residual=True, relu=True),
    conv_case('xpair_tiled', (3, 7, 31), 4, 8, plane_bias=True, out=(16, 8)),
    conv_case('tiled', (3, 7, 15), 16, 16, residual=True, bias=True, tile_y=4), conv_case('tiled', (5, 9, 17), 16, 32, G=3, residual=True, relu=True, tile_y=4),
    conv_case('tiled', (4, 16, 16), 8, 16, residual=True, plane_bias=True, tile_y=8), conv_case('tiled', (5, 17, 13), 16, 16, G=3, plane_bias=True, out=(32, 16), stats=False, tile_y=8),
    conv_case('tiled', (4, 15, 12), 32, 64, residual=True, tile_y=4), conv_case('tiled', (3, 16, 15), 16, 16, residual=True, cfg={'fused_finalize': True}, tile_y=8),
    conv_case('gather', (3, 5, 7), 16, 16, G=3, bias=True, relu=True), conv_case('gather', (4, 9, 11), 8, 16, residual=True, plane_bias=True),
    conv_case('gather', (5, 9, 13), 8, 16, stride=2, out=(32, 16)), conv_case('gather', (65, 1, 1), 16, 8, stats=False), conv_case('gather', (1, 1, 1), 3, 5),
    conv_case('gather', (9, 13), 3, 8, k=5, G=3, bias=True), conv_case('gather', (7, 15), 16, 32, dilation=2, relu=True)]
CONV_EXCLUDED = (PARTIAL_COLUMNS,
                 'columns C.. of a partial row of the gather kernel whose 16 * ntiles columns exceed its C channels: "per-workgroup (sum, sum of '
                 'squares) of the values written, per channel", header line 202')

Net('conv', tuple(sorted(set(FAMILY_ENTRY.values()))) + ('atvs_bn_finalize',), table(*(_2D + _3D)), build=_conv_inputs, shapes=_conv_shapes,
    run=_conv_run, select=list, names=('y (whole)', 'stats partial[..., :C]', 'bn_params of the stats', 'the pool of arrival tickets (fused_finalize)'),
    outputs=lambda p: (() if (p['out'] or p['family'] in ('conv2d_lds', 'conv2d_b', 'conv1x1', 'conv1x1_b')) else ('y5 = _new(x',)) +
    ((STATS, 'fin.counter, fin.params, fin.stats = ' if p['cfg'].get('fused_finalize') else PARAMS) if p['stats'] else ()),
    slices=lambda p: {'out': (p['out'][1], p['out'][1] + p['cout'])} if p['out'] else {}, excluded=CONV_EXCLUDED,
    constants='once per family conv_plan can return, each asserted against conv_plan and by the entry point reached.  XB_TZ/TY/TXV = 4/4/32 and '
              'XW_* = 4/8/32 with W >= 24; C16_* = B16_* = 4/8/16 with W >= 12; S2_* = 2/4/16 on the output with Wo >= 8; ST_* = 4/8/32; '
              'the tiled kernel\'s 4 x tile_y x 16 block with tile_y 4 (H < 16 or more than 32 channels) and 8; the gather kernel\'s 64 * tile_m '
              'voxels per workgroup (105, 396, 65 and 1 voxels); 2-D: H >= 8 and W >= 16, tiny maps from 2 x 2 on the split-operand kernel, '
              'stride 2 from 16 x 32 (even); 128 pixels per workgroup of conv1x1_b (C1B_PX): 126 | 128 | 129 and 255 | 256 | 257 pixels')


def _direct2d_inputs(p):
    G, (H, W), cin, cout = p['G'], p['hw'], p['cin'], p['cout']
    d = {'x': noise((G, H, W, cin), 411), 'w': kernel(((3, 3) if p['op'] == 'conv2d_lds' else (1, 1)) + (cin, cout), 412), 'bias': noise((cout,), 413),
         'in_params': params(G, cin, 415), 'form': dict(p)}
    if p['out']:
        d['out'] = noise((G, H, W, p['out'][0]), 416)
    else:
        d['residual'] = noise((G, H, W, cout), 414)           # "residual (same addressing as y, y_coff must be 0)", header line 194
    return d


def _direct2d_run(ops, d, place):
    f = d['form']
    fn = ops.conv2d_lds if f['op'] == 'conv2d_lds' else ops.conv1x1
    kw = dict(bias=d['bias'], residual=d.get('residual'), relu=True, want_stats=True, out=d.get('out'), y_coff=f['out'][1] if f['out'] else 0,
              in_params=d['in_params'] if f['norm'] else None, in_relu=f['norm'])
    y, st = fn(d['x'], 'layer', d['w'], **kw)
    return [y] + stats_of(ops, st, f['cout'], y)


def _direct2d(op, entry, hw, cin, cout, G=1, out=None, norm=False, cfg=None):
    p = dict(op=op, hw=hw, cin=cin, cout=cout, G=G, out=out, norm=norm, cfg=dict(cfg or {}), entries=(entry, 'atvs_bn_finalize'))
    return '%s: G=%d, %s, %d->%d%s%s' % (entry[5:-4], G, dims(hw), cin, cout, ', into [%d] of %d' % (out[1], out[0]) if out else '', ', norm on load' if norm else ''), p


for _op, _fp32, _b in (('conv2d_lds', 'atvs_conv2d_lds_f32', 'atvs_conv2d_b_f32'), ('conv1x1', 'atvs_conv1x1_f32', 'atvs_conv1x1_b_f32')):
    Net(_op, (_fp32, _b, 'atvs_bn_finalize'),
        table(_direct2d(_op, _fp32, (8, 16), 16, 32), _direct2d(_op, _fp32, (9, 17), 48, 64, G=3, out=(96, 32)),
              _direct2d(_op, _b, (8, 16), 32, 32, norm=True), _direct2d(_op, _b, (9, 17), 64, 64, G=3, out=(96, 32)), _direct2d(_op, _b, (7, 15), 32, 128, norm=True)),
        build=_direct2d_inputs, shapes=lambda p: {k: (tuple(v.shape), v.dtype) for k, v in _direct2d_inputs(p).items() if isinstance(v, torch.Tensor)},
        run=_direct2d_run, select=list, names=('y (whole)', 'stats partial', 'bn_params of the stats'),
        outputs=lambda p: (() if p['out'] else ('y = _new(x',)) + (STATS, PARAMS),
        slices=lambda p: {'out': (p['out'][1], p['out'][1] + p['cout'])} if p['out'] else {},
        constants='the wrapper reached directly, with bias, residual (dense outputs), ReLU and statistics at once: H >= 8, W >= 16 at the threshold, one above '
                  'and one below; the fp32 and the split-operand kernel; a channel slice of rows of 96 floats')


def _unit_inputs(p):
    G, (H, W), C = p['G'], p['hw'], p['C']
    return {'x': noise((G, H, W, C), 421), 'in_params': params(G, C, 422), 'w1': kernel((1, 1, C, C), 423), 'w2': kernel((3, 3, C, C), 424),
            'w3': kernel((1, 1, C, C), 425), 'b1': noise((C,), 426), 'b2': noise((C,), 427), 'b3': noise((C,), 428), 'residual': noise((G, H, W, C), 429), 'form': dict(p)}


def _unit_shapes(p):
    return {k: (tuple(v.shape), v.dtype) for k, v in _unit_inputs(p).items() if isinstance(v, torch.Tensor)}


def _bottleneck_run(ops, d, place):
    f = d['form']
    assert ops.bottleneck_ok(f['C'], f['dilation'], *f['hw'])
    y, st = ops.bottleneck(d['x'], d['in_params'], ('k1', 'k2', 'k3'), d['w1'], d['b1'], d['w2'], d['b2'], d['w3'], d['b3'], f['dilation'])
    return [y] + stats_of(ops, st, f['C'], y)


def _tail_run(ops, d, place):
    f = d['form']
    assert ops.conv2d_tail_ok(f['C'], f['dilation'], *f['hw'])
    y, st = ops.conv2d_tail(d['x'], ('k2', 'k3'), d['w2'], d['b2'], d['w3'], d['b3'], residual=d['residual'] if f['residual'] else None, dilation=f['dilation'])
    return [y] + stats_of(ops, st, f['C'], y)


Net('bottleneck', ('atvs_bottleneck_b_f32', 'atvs_bn_finalize'),
    table(*[('G=%d, %s, C=%d' % (G, dims(hw), C), {'G': G, 'hw': hw, 'C': C, 'dilation': 1}) for G, hw, C in ((1, (8, 16), 32), (3, (9, 17), 64), (1, (17, 33), 32))]),
    build=_unit_inputs, shapes=_unit_shapes, run=_bottleneck_run, select=list, names=('y', 'stats partial', 'bn_params of the stats'),
    outputs=('y = _new(x', STATS, PARAMS),
    constants='bottleneck_ok: H >= 8 and W >= 16 at the threshold and above, both channel counts atvs_bottleneck_b_supported admits (32, 64); three arranged kernels under the guard')

Net('conv2d_tail', ('atvs_conv2d_b_tail_f32', 'atvs_bn_finalize'),
    table(*[('G=%d, %s, dilation %d%s' % (G, dims(hw), dil, ', residual' if res else ''), {'G': G, 'hw': hw, 'C': 128, 'dilation': dil, 'residual': res})
            for G, hw, dil, res in ((1, (8, 16), 2, True), (3, (9, 17), 4, False), (1, (17, 33), 4, True))]),
    build=_unit_inputs, shapes=_unit_shapes, run=_tail_run, select=list, names=('y', 'stats partial', 'bn_params of the stats'),
    outputs=('y = _new(x', STATS, PARAMS),
    constants='conv2d_tail_ok: H >= 8 and W >= 16, C = 128 with dilation 2 and 4 (atvs_conv2d_b_tail_supported), with and without the shortcut')

for _row in ('bottleneck', 'conv2d_tail'):
    for _p in ROWS[_row].sizes.values():
        _p['entries'] = ROWS[_row].entries


def _head_inputs(p):
    G, s = p['G'], p['shape']
    lead = (G,) if G else ()
    d = {'w': noise((3, 3, 3, 8, 1), 431, -0.2, 0.2), 'form': dict(p)}
    if p['bn2']:
        d.update(x0=noise(lead + s + (8,), 432), x1=noise(lead + s + (8,), 433), p0=params(G, 8, 434), p1=params(G, 8, 435))
    else:
        d['x'] = noise(lead + s + (8,), 436)
    return d


def _head_run(ops, d, place):
    f = d['form']
    if f['bn2']:
        x = ops.PendingSum([ops.PendingBN(d['x0'], d['p0'], True), ops.PendingBN(d['x1'], d['p1'], False)])
        assert x.two_pending() is not None
        return ops.conv3d_8to1(x, d['w'], groups=f['G'])
    return ops.conv3d_8to1(d['x'], d['w'], groups=f['G'])


Net('conv3d_8to1', ('atvs_conv3d_8to1', 'atvs_conv3d_8to1_bn2'),
    table(*[('%s%s%s' % ('G=%d, ' % G if G else '', dims(s), ', over a pending two-term sum' if bn2 else ''),
             {'G': G, 'shape': s, 'bn2': bn2, 'entries': ('atvs_conv3d_8to1_bn2' if bn2 else 'atvs_conv3d_8to1',)})
            for G, s, bn2 in ((None, TILE_81[0], False), (3, TILE_81[1], False), (1, TILE_81[2], False), (None, (1, 1, 1), False),
                              (1, TILE_81[0], True), (3, TILE_81[1], True), (2, TILE_81[2], True), (1, (1, 1, 1), True))]),
    build=_head_inputs, shapes=lambda p: {k: (tuple(v.shape), v.dtype) for k, v in _head_inputs(p).items() if isinstance(v, torch.Tensor)},
    run=_head_run, select=lambda r: [r], names=('y',), outputs=lambda p: ('y = _new(a.raw',) if p['bn2'] else ('y = _new(x',),
    constants='C81_TZ/TY/TX = 4 / 16 / 16: one below, at and one above per axis, and one voxel; plain and the bn2 form (the sum is never written)')


def _up_inputs(p):
    G, s, cin, cout = p['G'], p['shape'], p['cin'], p['cout']
    d = {'w': kernel((3, 3, 3, cout, cin), 441) * np.float32(np.sqrt(cout / float(cin))), 'form': dict(p)}
    for i in range(p['terms'] or 1):
        d['x%d' % i] = noise((G,) + s + (cin,), 442 + i)
        if p['terms'] and p['pending'][i]:
            d['p%d' % i] = params(G, cin, 446 + i)
    return d


def _up_run(ops, d, place):
    f = d['form']
    x = d['x0']
    if f['terms']:
        x = ops.PendingSum([ops.PendingBN(d['x%d' % i], d['p%d' % i], bool(i != 1)) if f['pending'][i] else d['x%d' % i] for i in range(f['terms'])])
        assert ops.deconv_sum_ok(x, f['cout'], f['G'])
    y, st = ops.conv3d_transpose_s2(x, 'up', d['w'], relu=f['relu'], want_stats=True, groups=f['G'])
    return [y] + stats_of(ops, st, f['cout'], y)


def _up(entry, shape, cin, cout, G=1, relu=False, terms=0, pending=(), cfg=None):
    p = dict(shape=shape, cin=cin, cout=cout, G=G, relu=relu, terms=terms, pending=pending, cfg=dict(cfg or {}), entries=(entry, 'atvs_bn_finalize'))
    return '%s: G=%d, %s, %d->%d%s%s' % (entry[5:], G, dims(shape), cin, cout, ', relu' if relu else '',
                                         ', %d terms (%s pending)' % (terms, ''.join('01'[v] for v in pending)) if terms else ''), p


_UPF = 'atvs_deconv_up_f32'
Net('conv3d_transpose_s2', ('atvs_deconv_up_f32', 'atvs_deconv_up_b_f32', 'atvs_deconv_up_b_sum_f32', 'atvs_conv_tiled_f32', 'atvs_conv_mfma_f32', 'atvs_bn_finalize'),
    table(_up(_UPF, TILE_UP[0], 16, 8, cfg=_OFF('upb')), _up(_UPF, TILE_UP[1], 32, 16, G=3, relu=True, cfg=_OFF('upb')), _up(_UPF, TILE_UP[2], 64, 8, cfg=_OFF('upb')),
          _up(_UPF, (5, 5, 17), 16, 16, cfg=_OFF('upb')),
          _up('atvs_deconv_up_b_f32', TILE_UP[0], 16, 8), _up('atvs_deconv_up_b_f32', TILE_UP[1], 32, 16, G=3, relu=True), _up('atvs_deconv_up_b_f32', TILE_UP[2], 48, 8),
          _up('atvs_deconv_up_b_f32', (5, 5, 17), 64, 16), _up('atvs_deconv_up_b_f32', (2, 4, 8), 64, 32, G=3), _up('atvs_deconv_up_b_f32', (1, 1, 1), 16, 8),
          _up('atvs_deconv_up_b_sum_f32', TILE_UP[0], 16, 8, terms=2, pending=(1, 1)), _up('atvs_deconv_up_b_sum_f32', TILE_UP[1], 16, 8, G=3, terms=3, pending=(1, 1, 1), relu=True),
          _up('atvs_deconv_up_b_sum_f32', TILE_UP[2], 16, 8, terms=3, pending=(1, 0, 1)), _up('atvs_deconv_up_b_sum_f32', (1, 9, 17), 16, 8, G=3, terms=2, pending=(0, 1)),
          _up('atvs_conv_tiled_f32', (3, 7, 15), 16, 8, cfg={'deconv_up': False}), _up('atvs_conv_tiled_f32', (5, 17, 17), 16, 8, G=3, relu=True, cfg={'deconv_up': False}),
          _up('atvs_conv_tiled_f32', (4, 8, 12), 32, 16, cfg={'deconv_up': False}), _up('atvs_conv_mfma_f32', (3, 5, 7), 16, 8, G=3, cfg={'deconv_up': False})),
    build=_up_inputs, shapes=lambda p: {k: (tuple(v.shape), v.dtype) for k, v in _up_inputs(p).items() if isinstance(v, torch.Tensor)},
    run=_up_run, select=list, names=('y', 'stats partial[..., :C]', 'bn_params of the stats'), outputs=('y = _new(x', PARAMS),
    excluded=('columns 8.. of a [2][16] partial row of an 8-channel layer: "rows of [2][16] doubles (sum / sum of squares per channel)", header line 708',
              'the columns of the class-tap form beyond C are compared through bn_params(fold), which sums "columns c + C, c + 2C, ..." (header line 528)'),
    constants='UP_TZ/TX = 4 / 16, TY = 32 / NT = 8 input rows (8 channels) and 4 (16 channels): one below, at and one above per axis; deconv_up, '
              'deconv_up_b (and the 64 -> 32 layer as two launches into halves of y), deconv_up_b_sum over two and three terms, the class-tap form '
              'on the tiled kernel (W >= 12) and on the gather kernel (W < 12)')


def _sib_inputs(p):
    G, s, cin = p['G'], p['shape'], p['cin']
    d = {'w': kernel((3, 3, 3, cin, 8), 451), 'w2': kernel((3, 3, 3, cin, 16), 452), 'x': noise((G,) + s + (cin,), 453, 0.05, 0.35 if p['form'].startswith('planar') else 1.0),
         'case': dict(p)}
    if p['form'] in ('bn', 'sum'):
        d['p0'] = params(G, cin, 454)
    if p['form'] == 'sum':
        d['x1'], d['p1'] = noise((G,) + s + (cin,), 455), params(G, cin, 456)
    if p['bias']:
        D, H, W = s
        d['pb'], d['pb2'] = noise((G, H, W, 24), 457), noise((G, (H + 1) // 2, (W + 1) // 2, 48), 458)
    return d


def _to_planar(ops, x, place, pieces):
    """(G,D,H,W,C) channel-last -> the chunk-planar buffer (G, C/8, planar_stride) [of fp16 pieces], its pad holding noise."""
    G, D, H, W, C = x.shape
    n = D * H * W * 8
    buf = noise((G, C // 8, ops.planar_stride(D, H, W)), 459).to(x.device)
    planes = x.reshape(G, D, H, W, C // 8, 8).permute(0, 4, 1, 2, 3, 5).reshape(G, C // 8, n)
    if pieces:
        h0 = planes.half()
        h1 = ((planes - h0.float()) * 2048.0).half()
        planes = torch.stack([h0.reshape(G, C // 8, n), h1.reshape(G, C // 8, n)], 2).reshape(G, C // 8, 2 * n).view(torch.float32)
    buf[..., :n] = planes
    return place(buf)


def _sib_run(ops, d, place):
    f = d['case']
    G = f['G']
    x, kw = d['x'], {}
    if f['form'] == 'bn':
        x = ops.PendingBN(d['x'], d['p0'], True)
    elif f['form'] == 'sum':
        x = ops.PendingSum([ops.PendingBN(d['x'], d['p0'], True), ops.PendingBN(d['x1'], d['p1'], False)])
    elif f['form'].startswith('planar'):
        x = _to_planar(ops, d['x'], place, f['form'] == 'planar pieces')
        kw = dict(planar=f['shape'], pieces=f['form'] == 'planar pieces')
    (y, st), (y2, st2) = ops.conv_siblings(x, 'a', d['w'], 'b', d['w2'], plane_bias=d.get('pb'), plane_bias2=d.get('pb2'), groups=G, **kw)
    return [y] + stats_of(ops, st, 8, y) + [y2] + stats_of(ops, st2, 16, y2)


def _sib(kind, shape, cin, G=1, form='plain', bias=False):
    p = dict(shape=shape, cin=cin, G=G, form=form, bias=bias, cfg=FP32 if kind == 'xw' else {}, entries=('atvs_conv_%s_f32' % kind, 'atvs_bn_finalize'))
    return '%s: G=%d, %s, Cin=%d, %s%s' % (kind, G, dims(shape), cin, form, ', plane biases' if bias else ''), p


Net('conv_siblings', ('atvs_conv_xb_f32', 'atvs_conv_xw_f32', 'atvs_bn_finalize'),
    table(_sib('xb', TILE_XP[0], 8, bias=True), _sib('xb', TILE_XP[1], 16, G=3), _sib('xb', TILE_XP[2], 16, form='bn'), _sib('xb', TILE_XP[2], 8, G=3, form='sum'),
          _sib('xb', TILE_XP[0], 16, G=3, form='planar', bias=True), _sib('xb', TILE_XP[2], 32, form='planar pieces'), _sib('xb', (1, 1, 24), 8),
          _sib('xw', TILE_XW[0], 8, bias=True), _sib('xw', TILE_XW[1], 16, G=3), _sib('xw', TILE_XW[2], 16, form='bn'), _sib('xw', TILE_XW[2], 8, G=3, form='sum'),
          _sib('xw', TILE_XW[0], 16, G=3, form='planar', bias=True)),
    build=_sib_inputs, shapes=lambda p: {k: (tuple(v.shape), v.dtype) for k, v in _sib_inputs(p).items() if isinstance(v, torch.Tensor)},
    run=_sib_run, select=list, names=('y', 'stats partial[..., :8]', 'bn_params', 'y2', 'stats2 partial', 'bn_params of stats2'),
    outputs=('y, y2 = _new(x', STATS, PARAMS), excluded=(PARTIAL_COLUMNS,),
    constants='both outputs and both statistics buffers; XB_* = 4/4/32 and XW_* = 4/8/32 with W >= 24, odd extents (the stride-2 sibling rounds up); '
              'a chunk-planar input, fp16 pieces, a pending batch norm (Cin 16) and a two-term sum (Cin 8) formed on load')


def _split_inputs(p):
    G, (D, H, W), cv, cc = p['G'], p['shape'], p['cv'], p['cc']
    d = {'var': noise((G, D, H, W, cv), 461, 0.05, 0.35), 'const': noise((G, H, W, cc), 462), 'w': kernel((3, 3, 3, cv + cc + p['dup'], p['cout']), 463), 'case': dict(p)}
    if p['op'] == 'conv_split_siblings':
        d['w2'] = kernel((3, 3, 3, cv + cc + p['dup'], 16), 464)
    if p['op'] == 'conv_split' and p.get('out'):
        d['out'] = noise((G, D, H, W, p['out'][0]), 465)
    if p['op'] == 'conv_split_into_plane':
        from atvsnet_amd import ops
        d['buf'] = noise((G, 4, ops.planar_stride(D, H, W)), 466)
    return d


def chan_map(cv, cc, dup):
    """The reference's concat: the D-constant channels, the D-varying ones, then `dup` more copies of varying channel 0 (quirk C7)."""
    return [('c', i) for i in range(cc)] + [('v', i) for i in range(cv)] + [('v', 0)] * dup


def _split_run(ops, d, place):
    f = d['case']
    G, (D, H, W) = f['G'], f['shape']
    cm = chan_map(f['cv'], f['cc'], f['dup'])
    if f.get('planar'):
        sv = ops.SplitVolume(_to_planar(ops, d['var'], place, f['planar'] == 'pieces'), d['const'], cm, planar=(D, H, W), pieces=f['planar'] == 'pieces')
    else:
        sv = ops.SplitVolume(d['var'], d['const'], cm)
    if f['op'] == 'conv_split':
        y, st = ops.conv_split(sv, 'a', d['w'], stride=f.get('stride', 1), want_stats=True, out=d.get('out'), y_coff=f['out'][1] if f.get('out') else 0)
        return [y] + stats_of(ops, st, f['cout'], y)
    if f['op'] == 'conv_split_siblings':
        (y, st), (y2, st2) = ops.conv_split_siblings(sv, 'a', d['w'], 'b', d['w2'])
        return [y] + stats_of(ops, st, 8, y) + [y2] + stats_of(ops, st2, 16, y2)
    st = ops.conv_split_into_plane(sv, 'a', d['w'], d['buf'], 0, (D, H, W))
    return [d['buf']] + stats_of(ops, st, 8, d['var'])


def _split(op, entry, shape, cv, cc, cout=8, G=1, dup=0, out=None, planar=None, stride=1, cfg=None):
    p = dict(op=op, shape=shape, cv=cv, cc=cc, cout=cout, G=G, dup=dup, out=out, planar=planar, stride=stride, cfg=dict(cfg or {}),
             entries=(entry, 'atvs_bn_finalize'))
    return '%s: G=%d, %s, %d varying + %d constant%s -> %d%s%s' % (entry[5:-4], G, dims(shape), cv, cc, ' + %d copies' % dup if dup else '', cout,
                                                                   ', into [%d] of %d' % (out[1], out[0]) if out else '', ', planar %s' % planar if planar else ''), p


Net('conv_split', ('atvs_conv_xb_f32', 'atvs_conv_tiled_f32', 'atvs_conv_mfma_f32', 'atvs_bn_finalize'),
    table(_split('conv_split', 'atvs_conv_xb_f32', TILE_XP[0], 16, 16), _split('conv_split', 'atvs_conv_xb_f32', TILE_XP[2], 8, 32, G=3, dup=15, out=(32, 8)),
          _split('conv_split', 'atvs_conv_tiled_f32', TILE_C16[2], 8, 16, cout=16, G=3), _split('conv_split', 'atvs_conv_mfma_f32', (5, 9, 13), 8, 16, cout=16, stride=2)),
    build=_split_inputs, shapes=lambda p: {k: (tuple(v.shape), v.dtype) for k, v in _split_inputs(p).items() if isinstance(v, torch.Tensor)},
    run=_split_run, select=list, names=('y (whole)', 'stats partial[..., :C]', 'bn_params of the stats'), outputs=(STATS, PARAMS),
    slices=lambda p: {'out': (p['out'][1], p['out'][1] + p['cout'])} if p['out'] else {}, excluded=CONV_EXCLUDED,
    constants='the D-constant channels as a plane bias of the x-pair, the tiled (a plane bias keeps conv_plan off the dedicated 16-channel kernels) '
              'and the gather kernel (stride 2); 15 more copies of a varying channel folded into one (quirk C7); sizes as `conv`')

Net('conv_split_siblings', ('atvs_conv_xb_f32', 'atvs_conv_xw_f32', 'atvs_bn_finalize'),
    table(_split('conv_split_siblings', 'atvs_conv_xb_f32', TILE_XP[0], 16, 16), _split('conv_split_siblings', 'atvs_conv_xb_f32', TILE_XP[2], 16, 16, G=3, planar='plain'),
          _split('conv_split_siblings', 'atvs_conv_xb_f32', TILE_XP[1], 32, 32, planar='pieces'), _split('conv_split_siblings', 'atvs_conv_xw_f32', TILE_XW[2], 16, 16, G=3, planar='plain', cfg=FP32)),
    build=_split_inputs, shapes=lambda p: {k: (tuple(v.shape), v.dtype) for k, v in _split_inputs(p).items() if isinstance(v, torch.Tensor)},
    run=_split_run, select=list, names=('y', 'stats partial[..., :8]', 'bn_params', 'y2', 'stats2 partial', 'bn_params of stats2'),
    outputs=('y, y2 = _new(x', STATS, PARAMS), excluded=(PARTIAL_COLUMNS,),
    constants='the cost volume\'s two consumers in one launch: channel-last, chunk-planar and fp16 pieces; sizes as conv_siblings')


def _plane_slices(p):
    from atvsnet_amd import ops
    D, H, W = p['shape']
    m = planar_mask(ops, 4, D, H, W, planes=(0,))
    return {'buf': m.unsqueeze(0).expand(p['G'], -1, -1).contiguous()}


Net('conv_split_into_plane', ('atvs_conv_xb_f32', 'atvs_bn_finalize'),
    table(_split('conv_split_into_plane', 'atvs_conv_xb_f32', TILE_XP[0], 16, 16), _split('conv_split_into_plane', 'atvs_conv_xb_f32', TILE_XP[2], 16, 16, G=3, planar='pieces'),
          _split('conv_split_into_plane', 'atvs_conv_xb_f32', TILE_XP[1], 8, 32, G=2)),
    build=_split_inputs, shapes=lambda p: {k: (tuple(v.shape), v.dtype) for k, v in _split_inputs(p).items() if isinstance(v, torch.Tensor)},
    run=_split_run, select=list, names=('buf (whole)', 'stats partial[..., :8]', 'bn_params of the stats'), outputs=(STATS, PARAMS),
    slices=_plane_slices, excluded=(PARTIAL_COLUMNS,),
    constants='the photo stem as the producer of plane 0 of the (B, 4, planar_stride) concat: planes 1..3 and every pad are masked as not writable '
              '("ldy = 8 the output lands in one 8-channel plane", header line 312)')


def _stems_inputs(p):
    G, (D, H, W) = p['G'], p['shape']
    d = {'geo': noise((G, D, H, W, 2), 471), 'gpb': noise((G, H, W, 24), 472), 'prob': noise((G, D, H, W, 1), 473), 'hull': noise((G, D, H, W, 1), 474),
         'w_geo': kernel((3, 3, 3, 2, 8), 475), 'w_prob': kernel((3, 3, 3, 1, 8), 476), 'w_hull': kernel((3, 3, 3, 1, 8), 477), 'planar': p['planar']}
    if p['planar']:
        from atvsnet_amd import ops
        d['buf'] = noise((G, 4, ops.planar_stride(D, H, W)), 478)
    else:
        d['photo'] = noise((G, D, H, W, 8), 479)
    return d


def _stems_run(ops, d, place):
    buf, st = ops.refine_stems(d.get('photo'), d['geo'], d['gpb'], d['prob'], d['hull'], 'stems', d['w_geo'], d['w_prob'], d['w_hull'], planar_out=d.get('buf'))
    return [buf] + stats_of(ops, st, 24, d['geo'])


def _stems_slices(p):
    from atvsnet_amd import ops
    if not p['planar']:
        return {}
    D, H, W = p['shape']
    return {'buf': planar_mask(ops, 4, D, H, W, planes=(1, 2, 3)).unsqueeze(0).expand(p['G'], -1, -1).contiguous()}


Net('refine_stems', ('atvs_refine_stems_f32', 'atvs_bn_finalize'),
    table(*[('G=%d, %s%s' % (G, dims(s), ', planar_out' if pl else ''), {'G': G, 'shape': s, 'planar': pl, 'entries': ('atvs_refine_stems_f32', 'atvs_bn_finalize')})
            for G, s, pl in ((1, TILE_STEM[0], False), (3, TILE_STEM[1], False), (1, TILE_STEM[2], True), (3, TILE_STEM[0], True), (2, (2, 1, 1), True))]),
    build=_stems_inputs, shapes=lambda p: {k: (tuple(v.shape), v.dtype) for k, v in _stems_inputs(p).items() if isinstance(v, torch.Tensor)},
    run=_stems_run, select=list, names=('buffer (whole)', 'stats partial', 'bn_params of the stats'),
    outputs=lambda p: (STATS, PARAMS) + (() if p['planar'] else ('buf = _new(photo_raw',)),
    slices=_stems_slices,
    constants='ST_TZ/TY/TX = 4 / 8 / 32: one below, at and one above per axis, and two voxels (a geo plane bias needs D >= 2); with planar_out "planes 1..3 = geo | prob | hull are '
              'written, plane 0 is the photo stem\'s own" (header line 496): plane 0 and every pad are masked as not writable')


for _row in ROWS.values():
    for _p in _row.sizes.values():
        _p.setdefault('entries', _row.entries)
        _p.setdefault('cfg', {})
