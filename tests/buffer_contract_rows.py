"""One row per ops function that takes caller-owned buffers after the network (fusion, depth normals, view preparation, COLMAP
import, undistortion, the point-cloud family, scan and mesh rendering, TSDF fusion and meshing, mesh cleaning and simplification):
what tests/test_gpu_buffer_contract.py runs under tests/guarded_alloc.py and tests/test_buffer_contract_host.py checks for
completeness against include/atvsnet_hip.h.

A row holds
    name        the ops function
    entries     the C entry points (size queries included) the call must reach; a size may name its own with 'entries'
    sizes       {size name: parameters of `build`}, the smallest at which each kernel constant named in `constants` is crossed
    build(p)    -> {input name: CPU tensor or host value}, deterministic
    shapes(p)   -> {input name: (shape, dtype)} of every tensor `build` makes: what tests/test_buffer_contract_host.py holds it to
    run(ops, d, place) -> the result; d = the inputs on the device (placed under the guard), place = the guard's place for
                intermediates an op only reads (a CloudGrid's buffer, a clustering), the identity in the plain run
    select(r)   -> the specified part of the result as a list of tensors (host numbers become tensors); opaque handles (CloudGrid.buf)
                are compared through the ops that consume them, inside `run`
    outputs, scratch   pieces of the source lines that allocate them: at least one guarded allocation must match each (scratch:
                only where the call launches, `launches(p)`)
    writable    the inputs the op rewrites in place
    slices(p)   -> {input name: what of it the op may write, a bool mask or (lo, hi) of the last axis}: every other element is held
    excluded    what the selection leaves out, each with the line of include/atvsnet_hip.h that allows it

Where the header specifies a whole buffer of which the wrapper returns a slice (the 16 tolerance counters, the component counts),
the selection takes the whole buffer from the slice's first element on.
"""
import collections

import numpy as np
import torch

KTHREADS = 256                       # csrc/cloud_common.h kThreads (also colmap.hip, undistort.hip, fusion_grid.h kRun)
SCAN_TILE = 2048                     # csrc/cloud_scan.h kScanTile = kThreads * kScanItems
MOMENT_TILE = 4096                   # csrc/cloud_tree.h kMomentTile = kThreads * ATVS_CLOUD_MOMENT_RUN
TABLE_MIN_POINTS = 512               # 2 n <= 1024 = kMinSlots (cloud_register.hip), kClusterMinSlots, ATVS_MESH_SIMPLIFY_MIN_SLOTS;
#                                      8 n <= 4096 = kMinCells (cloud_grid.h): 513 is the first larger table and grid
CENSUS_MIN_FACES = 170               # 6 n_faces <= 1024 = ATVS_MESH_CENSUS_MIN_SLOTS: 171 is the first larger table
FEATURE_TILE = 128                   # ATVS_CLOUD_FEATURE_TILE
MAX_K, MAX_TOLERANCES, MAX_SPLAT = 32, 16, 4          # ATVS_CLOUD_MAX_K, ATVS_CLOUD_MAX_TOLERANCES, ATVS_SCAN_RENDER_MAX_SPLAT
CAMERA_GROUP = 8                     # kGroup of scan_render.hip, mesh_render.hip, colmap.hip: cameras per workgroup
RADIUS = 0.3

AROUND_WORKGROUP = (KTHREADS - 1, KTHREADS, KTHREADS + 1)
AROUND_TABLE = (TABLE_MIN_POINTS, TABLE_MIN_POINTS + 1)
AROUND_SCAN = (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1)
POINT_COUNTS = (0, 1) + AROUND_WORKGROUP + AROUND_TABLE + AROUND_SCAN
MAP = (23, 31)                       # 713 pixels: no multiple of 256

ROWS = collections.OrderedDict()


class Row(object):
    def __init__(self, name, entries, sizes, build, shapes, run, select, names, outputs, scratch=(), launches=None, writable=(),
                 excluded=(), constants='', slices=None, table=None):
        self.name, self.entries, self.sizes, self.build, self.shapes, self.run, self.select = name, tuple(entries), sizes, build, shapes, run, select
        self.names, self.scratch, self.writable, self.excluded = tuple(names), tuple(scratch), tuple(writable), tuple(excluded)
        self.outputs = outputs if callable(outputs) else tuple(outputs)      # (a function of the size's parameters in the network table)
        self.launches = launches or (lambda p: True)
        self.constants = constants
        self.slices = slices or (lambda p: {})      # slices(p) -> {input name: bool mask | (lo, hi) of the last axis}: what the op may write
        table = ROWS if table is None else table    # (tests/network_contract_rows.py registers in a table of its own)
        assert name not in table
        table[name] = self

    def required(self, size):
        """The entry points this size must reach."""
        p = self.sizes[size]
        if 'entries' in p:
            return tuple(p['entries'])
        return self.entries if self.launches(p) else ()


def sizes(key, values, **fixed):
    return collections.OrderedDict(('%s=%d' % (key, v), dict(fixed, **{key: v})) for v in values)


def merged(*parts):
    out = collections.OrderedDict()
    for part in parts:
        for k, v in part.items():
            assert k not in out, k
            out[k] = v
    return out


def cases():
    """[(row name, size name)] for pytest's parametrize."""
    return [(row.name, size) for row in ROWS.values() for size in row.sizes]


def _t(x, dtype=None):
    """A host result as a tensor: a number, a numpy array or None."""
    if x is None:
        return None
    return torch.as_tensor(np.asarray(x, dtype))


def _whole(t, n):
    """The n elements of the buffer whose first elements the wrapper returned as the slice t."""
    return t.as_strided((n,), (1,))


# ------------------------------------------------------------------------------------------------------------------ inputs
def cloud(n, seed, lo=-1.0, hi=1.0, bad=True):
    """n points in a box; from 8 points on a NaN row, an infinite row and a duplicate."""
    p = np.random.RandomState(seed).uniform(lo, hi, (n, 3)).astype(np.float32)
    if bad and n >= 8:
        p[3, 0], p[n // 2, 1] = np.nan, np.inf
        p[n - 1] = p[0]
    return torch.from_numpy(p)


def normals(n, seed):
    v = np.random.RandomState(seed).normal(size=(n, 3)).astype(np.float32)
    if n >= 8:
        v[1], v[5, 2] = 0.0, np.nan
    return torch.from_numpy(v)


def neighbours(m, k, n, seed):
    """(m,k) int32 in -1..n-1 as cloud_knn pads them: a row's valid entries first."""
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, max(n, 1), (m, k)).astype(np.int32)
    valid = rng.randint(0, k + 1, (m, 1)) if n else np.zeros((m, 1), np.int64)
    idx[np.arange(k)[None, :] >= valid] = -1
    return torch.from_numpy(idx)


def matches(m, n, seed):
    """(idx (m,) int32 in -1..n-1, d2 (m,) float32 with +inf where idx is -1 and a NaN) as cloud_nearest returns them."""
    rng = np.random.RandomState(seed)
    idx = rng.randint(-1, max(n, 1), m).astype(np.int32) if n else np.full(m, -1, np.int32)
    d2 = rng.uniform(0.0, 0.2, m).astype(np.float32)
    d2[idx < 0] = np.inf
    if m >= 8:
        d2[6] = np.nan
    return torch.from_numpy(idx), torch.from_numpy(d2)


MATRIX = np.array([[0.96, -0.28, 0.0, 0.1], [0.28, 0.96, 0.0, -0.2], [0.0, 0.0, 1.0, 0.05], [0, 0, 0, 1]], np.float64)
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


def ring(n_cams, rows, cols):
    from scan_render_restated import ring_cameras
    return torch.from_numpy(ring_cameras(n_cams, rows, cols))


# ============================================================================================================== ops/cloud.py
def _grid_run(ops, d, place):
    grid = ops.cloud_grid(d['points'], RADIUS)
    return (grid,) + ops.cloud_nearest(grid, d['queries']) + ops.cloud_knn(grid, d['queries'], 4)


Row('cloud_grid', ('atvs_cloud_grid_scratch_size', 'atvs_cloud_grid_build'), sizes('n', POINT_COUNTS),
    build=lambda p: {'points': cloud(p['n'], 1), 'queries': cloud(300, 2)},
    shapes=lambda p: {'points': ((p['n'], 3), F32), 'queries': ((300, 3), F32)},
    run=_grid_run, select=lambda r: list(r[1:]), names=('nearest d2', 'nearest idx', 'knn d2', 'knn idx'),
    outputs=(), scratch=('buf = torch.empty',),                # the grid IS its scratch: atvs_cloud_grid_scratch_size sizes it
    excluded=('CloudGrid.buf is opaque ("it IS the grid afterwards", header line 828): compared through cloud_nearest and cloud_knn',),
    constants='kThreads 256 points per workgroup; kMinCells 4096 = 8 x 512 points; the scan tile of 2048 counters')


def _searched(ops, d, place):
    grid = ops.cloud_grid(d['points'], RADIUS)
    grid.buf = place(grid.buf)
    return grid


SEARCH_SIZES = merged(collections.OrderedDict(('n=m=%d' % v, {'n': v, 'm': v}) for v in POINT_COUNTS[1:]),
                      {'n=0,m=5': {'n': 0, 'm': 5}, 'n=5,m=0': {'n': 5, 'm': 0}})

Row('cloud_nearest', ('atvs_cloud_nearest_scratch_size', 'atvs_cloud_nearest'), SEARCH_SIZES,
    build=lambda p: {'points': cloud(p['n'], 3), 'queries': cloud(p['m'], 4)},
    shapes=lambda p: {'points': ((p['n'], 3), F32), 'queries': ((p['m'], 3), F32)},
    run=lambda ops, d, place: ops.cloud_nearest(_searched(ops, d, place), d['queries']), select=list, names=('d2', 'idx'),
    outputs=('d2 = torch.empty', 'idx = torch.empty'), scratch=('scratch = torch.empty',), launches=lambda p: p['m'] > 0,
    constants='kThreads 256 queries per workgroup; the queries\' counting sort over the grid\'s cells (scan tile 2048)')

Row('cloud_counts', ('atvs_cloud_counts',), merged(sizes('m', (0, 1) + AROUND_WORKGROUP, k=3), sizes('k', (1, MAX_TOLERANCES), m=300)),
    build=lambda p: {'d2': matches(p['m'], 50, 5)[1], 'tolerances': np.linspace(0.05, 0.29, p['k']).tolist()},
    shapes=lambda p: {'d2': ((p['m'],), F32)},
    run=lambda ops, d, place: ops.cloud_counts(d['d2'], d['tolerances'], RADIUS), select=lambda r: [_whole(r, MAX_TOLERANCES)], names=('counts[16]',),
    outputs=('counts = torch.empty',),
    constants='kThreads 256; 1 and ATVS_CLOUD_MAX_TOLERANCES tolerances (all 16 words are "zeroed on the stream", header line 831)')


def _transform_run(ops, d, place):
    if d['in_place']:
        return ops.cloud_transform(d['points'], MATRIX, out=d['points'])
    return ops.cloud_transform(d['points'], MATRIX)


Row('cloud_transform', ('atvs_cloud_transform',), sizes('n', (0, 1) + AROUND_WORKGROUP, in_place=False),
    build=lambda p: {'points': cloud(p['n'], 6), 'in_place': p['in_place']}, shapes=lambda p: {'points': ((p['n'], 3), F32)},
    run=_transform_run, select=lambda r: [r], names=('out',), outputs=('out = torch.empty_like',), constants='kThreads 256')

Row('cloud_transform_in_place', ('atvs_cloud_transform',), sizes('n', (KTHREADS + 1,), in_place=True),
    build=lambda p: {'points': cloud(p['n'], 6), 'in_place': p['in_place']}, shapes=lambda p: {'points': ((p['n'], 3), F32)},
    run=_transform_run, select=lambda r: [r], names=('out',), outputs=(), writable=('points',),
    constants='"out may be points" (header line 853)')

MOMENT_SIZES = merged(sizes('m', (0, 1) + AROUND_WORKGROUP + (MOMENT_TILE - 1, MOMENT_TILE, MOMENT_TILE + 1), n=300))


def _moment_inputs(p):
    idx, d2 = matches(p['m'], p['n'], 7)
    return {'src': cloud(p['m'], 8), 'dst': cloud(p['n'], 9), 'idx': idx, 'd2': d2, 'normals': normals(p['m'], 10),
            'dst_normals': normals(p['n'], 11)}


def _moment_shapes(p):
    return {'src': ((p['m'], 3), F32), 'dst': ((p['n'], 3), F32), 'idx': ((p['m'],), I32), 'd2': ((p['m'],), F32),
            'normals': ((p['m'], 3), F32), 'dst_normals': ((p['n'], 3), F32)}


def _moments(r):
    return [_t(r[0], np.int64), _t(r[1])]


Row('cloud_pair_moments', ('atvs_cloud_pair_moments_scratch_size', 'atvs_cloud_pair_moments'), MOMENT_SIZES, _moment_inputs, _moment_shapes,
    run=lambda ops, d, place: ops.cloud_pair_moments(d['src'], d['dst'], d['idx'], d['d2'], trim=0.4, pivot_src=(0.1, 0.2, 0.3)),
    select=_moments, names=('count', 'moments[18]'), outputs=('out = torch.empty',), scratch=('scratch = torch.empty',),
    constants='kThreads 256; kMomentTile 4096 = 256 lanes x ATVS_CLOUD_MOMENT_RUN 16: a second partial row')

Row('cloud_plane_moments', ('atvs_cloud_plane_moments_scratch_size', 'atvs_cloud_plane_moments'), MOMENT_SIZES, _moment_inputs,
    _moment_shapes,
    run=lambda ops, d, place: ops.cloud_plane_moments(d['src'], d['normals'], MATRIX, d['dst'], d['idx'], d['d2'], trim=0.4, pivot=(0.1, 0, 0)),
    select=_moments, names=('count', 'moments[37]'), outputs=('out = torch.empty',), scratch=('scratch = torch.empty',),
    constants='as cloud_pair_moments')

Row('cloud_plane_moments_target', ('atvs_cloud_plane_moments_target_scratch_size', 'atvs_cloud_plane_moments_target'), MOMENT_SIZES,
    _moment_inputs, _moment_shapes,
    run=lambda ops, d, place: ops.cloud_plane_moments_target(d['src'], MATRIX, d['dst'], d['dst_normals'], d['idx'], d['d2'], trim=0.4),
    select=_moments, names=('count', 'moments[37]'), outputs=('out = torch.empty',), scratch=('scratch = torch.empty',),
    constants='as cloud_pair_moments')

_DOWNSAMPLE = ('atvs_cloud_voxel_downsample_scratch_size', 'atvs_cloud_voxel_downsample')

Row('cloud_voxel_downsample', _DOWNSAMPLE,
    merged(sizes('n', POINT_COUNTS, origin=(-2.0, -2.0, -2.0)),
           {'the default origin': {'n': 300, 'origin': None, 'entries': _DOWNSAMPLE + ('atvs_cloud_bounds',)}}),
    build=lambda p: {'points': cloud(p['n'], 12), 'origin': p['origin']}, shapes=lambda p: {'points': ((p['n'], 3), F32)},
    run=lambda ops, d, place: ops.cloud_voxel_downsample(d['points'], 0.25, origin=d['origin']), select=list,
    names=('means[:k]', 'first[:k]'), outputs=('means = torch.empty', 'first = torch.empty', 'count = torch.empty'),
    scratch=('scratch = torch.empty',),
    excluded=('rows k.. of means and first: "out_first (k) int32 ..., out_points (k,3) the means (both with room for n rows)", header '
              'line 910',),
    constants='kThreads 256; the table of max(2 n, 1024) slots: 512 | 513 points; the compaction\'s scan tile 2048')

Row('cloud_bounds', ('atvs_cloud_bounds',), sizes('n', (0, 1) + AROUND_WORKGROUP), build=lambda p: {'points': cloud(p['n'], 13)},
    shapes=lambda p: {'points': ((p['n'], 3), F32)}, run=lambda ops, d, place: ops.cloud_bounds(d['points']),
    select=lambda r: [_t(r[0]), _t(r[1])], names=('min', 'max'), outputs=('out = torch.empty',), constants='kThreads 256')

KNN_SIZES = merged(collections.OrderedDict(('n=m=%d,k=5' % v, {'n': v, 'm': v, 'k': 5, 'self': True}) for v in POINT_COUNTS[1:]),
                   {'k=1': {'n': 300, 'm': 257, 'k': 1, 'self': False}, 'k=32': {'n': 300, 'm': 257, 'k': MAX_K, 'self': False},
                    'n=0,m=5': {'n': 0, 'm': 5, 'k': 3, 'self': False}, 'n=5,m=0': {'n': 5, 'm': 0, 'k': 3, 'self': False}})


def _knn_inputs(p):
    pts = cloud(p['n'], 14, bad=not p['self'])
    return {'points': pts, 'queries': pts.clone() if p['self'] else cloud(p['m'], 15), 'k': p['k'], 'self': p['self']}


Row('cloud_knn', ('atvs_cloud_knn_scratch_size', 'atvs_cloud_knn'), KNN_SIZES, _knn_inputs,
    shapes=lambda p: {'points': ((p['n'], 3), F32), 'queries': ((p['m'], 3), F32)},
    run=lambda ops, d, place: ops.cloud_knn(_searched(ops, d, place), d['queries'], d['k'], exclude_same_index=d['self']),
    select=list, names=('d2', 'idx'), outputs=('d2 = torch.empty', 'idx = torch.empty'), scratch=('scratch = torch.empty',),
    launches=lambda p: p['m'] > 0, constants='kThreads 256; k = 1 and ATVS_CLOUD_MAX_K; the queries\' counting sort (scan tile 2048)')

Row('cloud_radius_count', ('atvs_cloud_knn_scratch_size', 'atvs_cloud_radius_count'), KNN_SIZES, _knn_inputs,
    shapes=lambda p: {'points': ((p['n'], 3), F32), 'queries': ((p['m'], 3), F32)},
    run=lambda ops, d, place: ops.cloud_radius_count(_searched(ops, d, place), d['queries'], exclude_same_index=d['self']),
    select=lambda r: [r], names=('count',), outputs=('count = torch.empty',), scratch=('scratch = torch.empty',),
    launches=lambda p: p['m'] > 0, constants='as cloud_knn')


def _knn_d2(m, k, seed):
    d2 = np.sort(np.random.RandomState(seed).uniform(0, 0.09, (m, k)).astype(np.float32), axis=1)
    d2[::3, k - 1:] = np.inf
    return torch.from_numpy(d2)


Row('cloud_knn_mean', ('atvs_cloud_knn_mean',), merged(sizes('m', (0, 1) + AROUND_WORKGROUP, k=5), sizes('k', (1, MAX_K), m=257)),
    build=lambda p: {'d2': _knn_d2(p['m'], p['k'], 16)}, shapes=lambda p: {'d2': ((p['m'], p['k']), F32)},
    run=lambda ops, d, place: ops.cloud_knn_mean(d['d2']), select=lambda r: [r], names=('s',), outputs=('s = torch.empty',),
    launches=lambda p: p['m'] > 0, constants='kThreads 256; k = 1 and ATVS_CLOUD_MAX_K')


def _sor_s(m, seed):
    s = np.random.RandomState(seed).uniform(0.01, 0.3, m)
    s[::7] = np.inf
    return torch.from_numpy(s)


Row('cloud_sor_stats', ('atvs_cloud_sor_stats_scratch_size', 'atvs_cloud_sor_stats'),
    sizes('m', (0, 1, 2) + AROUND_WORKGROUP + (MOMENT_TILE - 1, MOMENT_TILE, MOMENT_TILE + 1)),
    build=lambda p: {'s': _sor_s(p['m'], 17)}, shapes=lambda p: {'s': ((p['m'],), F64)},
    run=lambda ops, d, place: ops.cloud_sor_stats(d['s']), select=lambda r: [_t(r[0], np.int64), _t(r[1:], np.float64)],
    names=('count', 'mean, std'), outputs=('out = torch.empty',), scratch=('scratch = torch.empty',),
    constants='kThreads 256; kMomentTile 4096')


def _normals_inputs(p):
    return {'points': cloud(p['n'], 18), 'queries': cloud(p['m'], 19), 'idx': neighbours(p['m'], p['k'], p['n'], 20),
            'view_of': torch.from_numpy((np.arange(p['m']) % 3 - 1).astype(np.int32))}


Row('cloud_normals', ('atvs_cloud_normals',),
    merged(sizes('m', (0, 1) + AROUND_WORKGROUP, n=300, k=8), sizes('k', (1, MAX_K), n=300, m=257)), _normals_inputs,
    shapes=lambda p: {'points': ((p['n'], 3), F32), 'queries': ((p['m'], 3), F32), 'idx': ((p['m'], p['k']), I32), 'view_of': ((p['m'],), I32)},
    run=lambda ops, d, place: ops.cloud_normals(d['points'], d['queries'], d['idx'], viewpoints=[(0, 0, 3.0), (3.0, 0, 0)],
                                                view_of=d['view_of'], variation=True),
    select=list, names=('normals', 'variation'), outputs=('normals = torch.empty', 'var = torch.empty'), launches=lambda p: p['m'] > 0,
    constants='kThreads 256 queries per workgroup; k = 1 and ATVS_CLOUD_MAX_K')

Row('cloud_fpfh', ('atvs_cloud_fpfh_scratch_size', 'atvs_cloud_fpfh'),
    merged(sizes('n', (0, 1, 7, 63, 64, 65) + AROUND_WORKGROUP + AROUND_TABLE, k=8), sizes('k', (1, MAX_K), n=257)),
    build=lambda p: {'points': cloud(p['n'], 21), 'idx': neighbours(p['n'], p['k'], p['n'], 22), 'normals': normals(p['n'], 23)},
    shapes=lambda p: {'points': ((p['n'], 3), F32), 'idx': ((p['n'], p['k']), I32), 'normals': ((p['n'], 3), F32)},
    run=lambda ops, d, place: ops.cloud_fpfh(d['points'], d['idx'], d['normals']), select=lambda r: [r], names=('fpfh',),
    outputs=('out = torch.empty',), scratch=('scratch = torch.empty',), launches=lambda p: p['n'] > 0,
    constants='kThreads 256; the scratch of align256(n * 36 + 256) bytes: n = 64 makes n * 36 a multiple of 256, 7 and 63 | 65 '
              'sit one row under | over a boundary; k = 1 and ATVS_CLOUD_MAX_K')


def _features(n, seed):
    f = np.random.RandomState(seed).uniform(0, 1, (n, 33)).astype(np.float32)
    f[::5] = 0.0
    return torch.from_numpy(f)


Row('cloud_feature_nearest', ('atvs_cloud_feature_nearest',),
    merged(sizes('n', (0, 1, FEATURE_TILE - 1, FEATURE_TILE, FEATURE_TILE + 1, 2 * FEATURE_TILE + 1), m=130),
           sizes('m', (0, 1) + AROUND_WORKGROUP, n=130)),
    build=lambda p: {'ref': _features(p['n'], 24), 'query': _features(p['m'], 25)},
    shapes=lambda p: {'ref': ((p['n'], 33), F32), 'query': ((p['m'], 33), F32)},
    run=lambda ops, d, place: ops.cloud_feature_nearest(d['ref'], d['query']), select=list, names=('d2', 'idx'),
    outputs=('d2 = torch.empty', 'idx = torch.empty'), launches=lambda p: p['m'] > 0,
    constants='ATVS_CLOUD_FEATURE_TILE 128 reference rows per LDS tile; kThreads 256 queries per workgroup')


def _ransac_inputs(p):
    rng = np.random.RandomState(26)
    src = cloud(p['c'], 27, bad=False)
    dst = torch.from_numpy((src.numpy().astype(np.float64) @ MATRIX[:3, :3].T + MATRIX[:3, 3]).astype(np.float32)
                           + rng.normal(scale=0.01, size=(p['c'], 3)).astype(np.float32))
    triples = rng.randint(0, p['c'], (p['h'], 3)).astype(np.int32)
    if p['h'] >= 8:
        triples[2] = (0, 0, 1)                      # a repeated index
        triples[5, 1] = p['c']                      # outside 0..c-1
    return {'src': src, 'dst': dst, 'triples': torch.from_numpy(triples), 'best': p['best']}


def _ransac_select(r):
    found, valid = r
    return [_t(np.stack([f['matrix'] for f in found])), _t([f['count'] for f in found], np.int64), _t([f['sum'] for f in found], np.float64),
            _t([f['index'] for f in found], np.int64), _t(valid, np.int64)]


Row('cloud_ransac', ('atvs_cloud_ransac_scratch_size', 'atvs_cloud_ransac_score'),
    merged(sizes('h', (1, 63, 64, 65) + AROUND_WORKGROUP + AROUND_SCAN, c=300, best=4), sizes('best', (1, 8), c=257, h=300),
           sizes('c', (3,) + AROUND_WORKGROUP, h=100, best=2)),
    _ransac_inputs, shapes=lambda p: {'src': ((p['c'], 3), F32), 'dst': ((p['c'], 3), F32), 'triples': ((p['h'], 3), I32)},
    run=lambda ops, d, place: ops.cloud_ransac(d['src'], d['dst'], d['triples'], 0.05, True, best=d['best'], return_valid=True),
    select=_ransac_select, names=('matrices', 'counts', 'sums', 'indices', 'valid (read from the scratch\'s h counts)'),
    outputs=('out = torch.empty',), scratch=('scratch = torch.empty',),
    constants='kThreads 256 hypotheses per workgroup and 256 pairs per LDS tile; the sums begin at the next multiple of 256 bytes '
              'behind 4 h bytes of counts: h = 64 is on it, 63 | 65 beside it; best 1 and ATVS_CLOUD_RANSAC_MAX_BEST')

Row('scan_render', ('atvs_scan_render_scratch_size', 'atvs_scan_render'),
    merged(sizes('n', (0, 1) + AROUND_WORKGROUP, cams=2, splat=1), sizes('splat', (0, MAX_SPLAT), n=300, cams=2),
           sizes('cams', (1, CAMERA_GROUP, CAMERA_GROUP + 1), n=300, splat=2)),
    build=lambda p: {'points': cloud(p['n'], 28), 'cams': ring(p['cams'], *MAP), 'splat': p['splat']},
    shapes=lambda p: {'points': ((p['n'], 3), F32), 'cams': ((p['cams'], 16), F64)},
    run=lambda ops, d, place: ops.scan_render(d['points'], d['cams'], MAP[0], MAP[1], pixel_centre=0.5, splat=d['splat'], occlusion_tol=0.01),
    select=lambda r: [r], names=('depth',), outputs=('depth = torch.empty',), scratch=('scratch = torch.empty',),
    constants='kThreads 256 points and kGroup 8 cameras per workgroup; splat 0 and ATVS_SCAN_RENDER_MAX_SPLAT; maps of 713 pixels')


def _cube_inputs(p):
    from atvsnet_amd.atvsnet.eval_eth3d import cube_cameras
    rng = np.random.RandomState(29)
    cams = np.concatenate([cube_cameras((0.3 * s, -0.2 * s, 0.1), p['size']) for s in range(p['scanners'])])
    maps = rng.uniform(0.4, 1.6, (6 * p['scanners'], p['size'], p['size'])).astype(np.float32)
    maps[rng.uniform(size=maps.shape) < 0.3] = 0.0
    return {'points': cloud(p['m'], 30), 'cams': torch.from_numpy(cams), 'maps': torch.from_numpy(maps), 'window': p['window']}


Row('cloud_scan_excess', ('atvs_cloud_scan_excess',),
    merged(sizes('m', (0, 1) + AROUND_WORKGROUP, scanners=2, size=13, window=1), sizes('window', (0, 2), m=300, scanners=1, size=13)),
    _cube_inputs,
    shapes=lambda p: {'points': ((p['m'], 3), F32), 'cams': ((6 * p['scanners'], 16), F64), 'maps': ((6 * p['scanners'], p['size'], p['size']), F32)},
    run=lambda ops, d, place: ops.cloud_scan_excess(d['points'], d['cams'], d['maps'], window=d['window']), select=list,
    names=('excess', 'scanner'), outputs=('excess = torch.empty', 'scanner = torch.empty'), launches=lambda p: p['m'] > 0,
    constants='kThreads 256 points per workgroup; window 0 and ATVS_CLOUD_SCAN_MAX_WINDOW; faces of 13 x 13')


def _share_inputs(p):
    rng = np.random.RandomState(31)
    d2 = matches(p['n'], 50, 32)[1]
    excess = rng.normal(scale=0.05, size=p['n']).astype(np.float32)
    excess[::6] = np.inf
    return {'points': cloud(p['n'], 33), 'd2': d2, 'excess': torch.from_numpy(excess) if p['excess'] else None,
            'tolerances': np.linspace(0.02, 0.4, p['t']).tolist()}


Row('cloud_voxel_shares', ('atvs_cloud_voxel_shares_scratch_size', 'atvs_cloud_voxel_shares'),
    merged(sizes('n', (0, 1) + AROUND_WORKGROUP + AROUND_TABLE, t=2, excess=True), sizes('t', (1, 4, 5, MAX_TOLERANCES), n=300, excess=True),
           {'no excess': {'n': 300, 't': 3, 'excess': False}}),
    _share_inputs,
    shapes=lambda p: dict({'points': ((p['n'], 3), F32), 'd2': ((p['n'],), F32)}, **({'excess': ((p['n'],), F32)} if p['excess'] else {})),
    run=lambda ops, d, place: ops.cloud_voxel_shares(d['points'], d['d2'], d['excess'], 0.25, (-2.0, -2.0, -2.0), d['tolerances'], margin=0.01),
    select=lambda r: [r], names=('shares (T,4)',), outputs=('out = torch.empty',), scratch=('scratch = torch.empty',),
    constants='kThreads 256; the table of max(2 n, 1024) slots: 512 | 513; kSharePass 4 tolerances per pass: 4 | 5; 1 and '
              'ATVS_CLOUD_MAX_TOLERANCES')


# =============================================================================================================== ops/mesh.py
def _soup_inputs(p):
    from mesh_render_restated import triangle_soup
    cams = ring(p['cams'], *MAP)
    v, f = triangle_soup(p['faces'], cams.numpy(), MAP[0], MAP[1], seed=34)
    return {'vertices': torch.from_numpy(v), 'faces': torch.from_numpy(f), 'cams': cams}


Row('mesh_render', ('atvs_mesh_render_scratch_size', 'atvs_mesh_render'),
    merged(sizes('faces', (0, 1) + AROUND_WORKGROUP, cams=2), sizes('cams', (1, CAMERA_GROUP, CAMERA_GROUP + 1), faces=300)), _soup_inputs,
    shapes=lambda p: {'vertices': ((3 * p['faces'], 3), F32), 'faces': ((p['faces'], 3), I32), 'cams': ((p['cams'], 16), F64)},
    run=lambda ops, d, place: ops.mesh_render(d['vertices'], d['faces'], d['cams'], MAP[0], MAP[1], pixel_centre=0.5), select=list,
    names=('depth', 'face'), outputs=('depth = torch.empty', 'face = torch.empty', 'err = torch.empty'), scratch=('scratch = torch.empty',),
    constants='kThreads 256 faces and kGroup 8 cameras per workgroup; the soup\'s faces lie on both sides of '
              'ATVS_MESH_RENDER_SMALL_PIXELS 64 (the pair list and the 64-pixel tiles); maps of 713 pixels')


def _occlude_inputs(p):
    rng = np.random.RandomState(35)
    depth = rng.uniform(0.5, 2.0, p['pixels']).astype(np.float32)
    occ = (depth * rng.uniform(0.8, 1.2, p['pixels'])).astype(np.float32)
    depth[::5], occ[::7] = 0.0, 0.0
    if p['pixels'] >= 8:
        depth[2], occ[4] = np.nan, np.nan
    return {'depth': torch.from_numpy(depth), 'occluder': torch.from_numpy(occ)}


Row('depth_occlude', ('atvs_depth_occlude',), sizes('pixels', (0, 1) + AROUND_WORKGROUP + (MAP[0] * MAP[1],)), _occlude_inputs,
    shapes=lambda p: {'depth': ((p['pixels'],), F32), 'occluder': ((p['pixels'],), F32)},
    run=lambda ops, d, place: ops.depth_occlude(d['depth'], d['occluder'], tol=0.05), select=lambda r: [r], names=('out',),
    outputs=('out = torch.empty_like',), constants='kThreads 256 pixels per workgroup; a map of 713 pixels')


# ====================================================================================================== ops/mesh_topology.py
def _mesh(p, seed=36):
    """V vertices, F faces that stay inside blocks of 16 vertices (many components), a repeated-index face and a doubled face."""
    rng = np.random.RandomState(seed)
    V, F = p['V'], p['F']
    base = (rng.randint(0, max(V, 1), (F, 1)) // 16) * 16
    faces = np.minimum(base + rng.randint(0, 16, (F, 3)), max(V - 1, 0)).astype(np.int32)
    if F >= 8:
        faces[3, 2] = faces[3, 0]
        faces[6] = faces[5, ::-1]
    vertices = cloud(V, seed + 1)
    colors = torch.from_numpy(rng.randint(0, 256, (V, 3)).astype(np.uint8))
    keep = torch.from_numpy((rng.uniform(size=F) < 0.6).astype(np.uint8))
    return {'vertices': vertices, 'colors': colors, 'faces': torch.from_numpy(faces), 'keep': keep, 'V': V}


def _mesh_shapes(p):
    return {'vertices': ((p['V'], 3), F32), 'colors': ((p['V'], 3), U8), 'faces': ((p['F'], 3), I32), 'keep': ((p['F'],), U8)}


MESH_COUNTS = (1,) + AROUND_WORKGROUP + AROUND_TABLE + AROUND_SCAN
MESH_SIZES = merged({'V=0,F=0': {'V': 0, 'F': 0}, 'V=5,F=0': {'V': 5, 'F': 0}},
                    collections.OrderedDict(('V=F=%d' % v, {'V': v, 'F': v}) for v in MESH_COUNTS))

Row('mesh_components', ('atvs_mesh_components_scratch_size', 'atvs_mesh_components'), MESH_SIZES, _mesh, _mesh_shapes,
    run=lambda ops, d, place: ops.mesh_components(d['faces'], d['V']), select=lambda r: [r[0], r[1]] + [_whole(t, max(1, min(len(r[0]), len(r[1])))) for t in r[2:]],
    names=('vertex_component', 'face_component', 'face_count (whole: "the rest 0", header line 1366)', 'vertex_count (whole)'),
    outputs=('vertex_component = torch.empty', 'face_component = torch.empty', 'face_count = torch.empty', 'vertex_count = torch.empty',
             'info = torch.empty'),
    scratch=('scratch = torch.empty',), constants='kThreads 256 faces / vertices per workgroup; the scan tile of 2048 vertices')

Row('mesh_select', ('atvs_mesh_select_scratch_size', 'atvs_mesh_select'), MESH_SIZES, _mesh, _mesh_shapes,
    run=lambda ops, d, place: ops.mesh_select(d['vertices'], d['colors'], d['faces'], d['keep']), select=list,
    names=('vertices[:V\']', 'colors[:V\']', 'faces[:F\']', 'vertex_map'),
    outputs=('vertices_out = torch.empty_like', 'colors_out = ', 'faces_out = torch.empty_like', 'vertex_map = torch.empty', 'info = torch.empty'),
    scratch=('scratch = torch.empty',),
    excluded=('rows V\'.. of vertices_out and colors_out, rows F\'.. of faces_out: "the first V\' and F\' rows are written", header line 1373',),
    constants='kThreads 256; the scan tile of 2048 vertices and faces')

Row('mesh_edge_census', ('atvs_mesh_edge_census_scratch_size', 'atvs_mesh_edge_census'),
    merged(MESH_SIZES, collections.OrderedDict(('V=F=%d' % v, {'V': v, 'F': v}) for v in (CENSUS_MIN_FACES, CENSUS_MIN_FACES + 1))),
    _mesh, _mesh_shapes, run=lambda ops, d, place: ops.mesh_edge_census(d['faces'], d['V']),
    select=lambda r: [_t([r[k] for k in sorted(r)], np.int64)], names=('census[8]',), outputs=('words = torch.empty',),
    scratch=('scratch = torch.empty',),
    constants='kThreads 256; the table of max(6 n_faces, ATVS_MESH_CENSUS_MIN_SLOTS 1024) slots: 170 | 171 faces')


# ====================================================================================================== ops/mesh_simplify.py
CELL, CELL_ORIGIN = 0.2, (-2.0, -2.0, -2.0)


def _clustered(ops, d, place):
    c = ops.mesh_cluster(d['vertices'], d['colors'], CELL, CELL_ORIGIN)
    return type(c)(*[None if t is None else place(t) for t in c])


Row('mesh_cluster', ('atvs_mesh_cluster_scratch_size', 'atvs_mesh_cluster'), MESH_SIZES, _mesh, _mesh_shapes,
    run=lambda ops, d, place: ops.mesh_cluster(d['vertices'], d['colors'], CELL, CELL_ORIGIN), select=list,
    names=('vertex_cluster', 'cells[:C]', 'counts[:C]', 'position_sums[:C]', 'color_sums[:C]'),
    outputs=('vertex_cluster = torch.empty', 'cells = torch.empty', 'counts = torch.empty', 'position_sums = torch.empty', 'color_sums = ',
             'count = torch.empty'),
    scratch=('scratch = torch.empty',), launches=lambda p: p['V'] > 0,
    excluded=('rows C.. of cells, counts, position_sums, color_sums: "rows of buffers of n_vertices rows of which the first C are written", '
              'header line 1419',),
    constants='kThreads 256; the table of max(2 n_vertices, 1024) slots: 512 | 513; the compaction\'s scan tile 2048')


def _quadrics_run(ops, d, place):
    c = _clustered(ops, d, place)
    return ops.mesh_cluster_quadrics(d['vertices'], d['faces'], c.vertex_cluster, int(c.cells.shape[0]), CELL, CELL_ORIGIN)


Row('mesh_cluster_quadrics', ('atvs_mesh_cluster_quadrics',), MESH_SIZES, _mesh, _mesh_shapes, run=_quadrics_run, select=list,
    names=('quadrics', 'incidences'), outputs=('quadrics = torch.empty', 'incidences = torch.empty', 'info = torch.empty'),
    constants='kThreads 256 faces per workgroup; both outputs are "zeroed here" (header line 1426)')


def _place_run(ops, d, place):
    c = _clustered(ops, d, place)
    q, _ = ops.mesh_cluster_quadrics(d['vertices'], d['faces'], c.vertex_cluster, int(c.cells.shape[0]), CELL, CELL_ORIGIN)
    q = place(q)
    return ops.mesh_cluster_place(c.cells, c.counts, c.position_sums, c.color_sums, q, CELL, CELL_ORIGIN, 'quadric') + \
        ops.mesh_cluster_place(c.cells, c.counts, c.position_sums, None, None, CELL, CELL_ORIGIN, 'mean')


Row('mesh_cluster_place', ('atvs_mesh_cluster_place',), MESH_SIZES, _mesh, _mesh_shapes, run=_place_run, select=list,
    names=('positions', 'colors', 'placed', 'mean positions', 'mean colors (None)', 'mean placed'),
    outputs=('positions = torch.empty', 'colors = ', 'placed = torch.empty'), launches=lambda p: p['V'] > 0,
    constants='kThreads 256 clusters per workgroup; both placements')


def _move_run(ops, d, place):
    c = _clustered(ops, d, place)
    positions = place(ops.mesh_cluster_place(c.cells, c.counts, c.position_sums, None, None, CELL, CELL_ORIGIN, 'mean')[0])
    return ops.mesh_cluster_max_move(d['vertices'], c.vertex_cluster, positions)


Row('mesh_cluster_max_move', ('atvs_mesh_cluster_max_move',), MESH_SIZES, _mesh, _mesh_shapes, run=_move_run,
    select=lambda r: [_t(r, np.float64)], names=('max move',), outputs=('out = torch.empty',), launches=lambda p: p['V'] > 0,
    constants='kThreads 256; out is "zeroed here" (header line 1456)')

Row('mesh_cluster_faces', ('atvs_mesh_cluster_faces_scratch_size', 'atvs_mesh_cluster_faces'), MESH_SIZES, _mesh, _mesh_shapes,
    run=lambda ops, d, place: ops.mesh_cluster_faces(d['faces'], _clustered(ops, d, place).vertex_cluster),
    select=lambda r: [r[0], r[1], _t([r[2][k] for k in sorted(r[2])], np.int64)], names=('faces_out', 'keep', 'counts'),
    outputs=('faces_out = torch.empty_like', 'keep = torch.empty', 'info = torch.empty'), scratch=('scratch = torch.empty',),
    launches=lambda p: p['F'] > 0, constants='kThreads 256; the table of max(2 n_faces, ATVS_MESH_SIMPLIFY_MIN_SLOTS 1024) slots: 512 | 513 faces')


# =============================================================================================================== ops/tsdf.py
def _all_blocks(dims, count, seed):
    bx, by, bz = dims
    lin = np.sort(np.random.RandomState(seed).choice(bx * by * bz, count, replace=False))
    return torch.from_numpy(np.stack([lin % bx, (lin // bx) % by, lin // (bx * by)], 1).astype(np.int32))


FREE_DIMS = (6, 6, 9)

Row('tsdf_free_views', ('atvs_tsdf_free_views',),
    merged(sizes('count', (0, 1, 3, 4, 5) + AROUND_WORKGROUP, views=3), sizes('views', (1, 64, 65), count=37)),
    build=lambda p: {'blocks': _all_blocks(FREE_DIMS, p['count'], 37), 'cams': ring(p['views'], 5, 7)},
    shapes=lambda p: {'blocks': ((p['count'], 3), I32), 'cams': ((p['views'], 16), F64)},
    run=lambda ops, d, place: ops.tsdf_free_views(d['blocks'], d['cams'], 5, 7, 0.05, (-1.2, -1.2, -1.8), FREE_DIMS, pixel_centre=0.5),
    select=lambda r: [r], names=('masks',), outputs=('masks = torch.empty',), launches=lambda p: p['count'] > 0,
    constants='kFreeWaves 4 (block, word) items per workgroup: 3 | 4 | 5 blocks; 64 and 65 views: the second mask word of '
              '(n + 63) // 64')


def _one_block():
    import tsdf_restated as R
    from scan_render_restated import ring_cameras
    cams = ring_cameras(3, *MAP)
    depths, images = R.sphere_depths(cams, MAP[0], MAP[1], 0.15)
    return dict(depths=depths, cams=cams, images=images, voxel=0.05, trunc=0.1, origin=(-0.2, -0.2, -0.2), dims=(1, 1, 1), pixel_centre=0.0)


def _of(case):
    return dict(depths=case.depths, cams=case.cams, images=case.images, voxel=case.voxel, trunc=case.trunc, origin=case.origin,
                dims=case.dims, pixel_centre=case.pixel_centre)


def _tsdf_scene(name):
    import tsdf_cases as TC
    import tsdf_carve_restated as CR
    return {'one_block': _one_block, 'uneven': lambda: _of(TC.uneven(0.2)), 'long_directory': lambda: _of(TC.long_directory()),
            'views64': lambda: _of(TC.mask_bits((31, 32, 63))), 'views65': lambda: _of(CR.views65())}[name]()


def _integrate_inputs(p):
    s = _tsdf_scene(p['scene'])
    w = np.random.RandomState(38).uniform(0.2, 2.0, s['depths'].shape).astype(np.float32)
    for start, value in enumerate((0.0, -1.0, np.nan, np.inf)):               # the four kinds of a weight that is no sample
        w.reshape(-1)[start::29] = value
    d = {'depths': torch.from_numpy(s['depths']), 'cams': torch.from_numpy(s['cams']), 'images': torch.from_numpy(s['images']),
         'weights': torch.from_numpy(w) if 'weighted' in p['form'] else None, 'carve': 0.5 if 'carve' in p['form'] else None}
    d.update({k: s[k] for k in ('voxel', 'trunc', 'origin', 'dims', 'pixel_centre')})
    return d


def _integrate_shapes(p):
    s = _tsdf_scene(p['scene'])
    out = {'depths': (s['depths'].shape, F32), 'cams': ((len(s['cams']), 16), F64), 'images': (s['depths'].shape + (s['images'].shape[-1],), F32)}
    if 'weighted' in p['form']:
        out['weights'] = (s['depths'].shape, F32)
    return out


def _integrate_run(ops, d, place):
    return ops.tsdf_integrate(d['depths'], d['cams'], d['voxel'], d['trunc'], d['origin'], d['dims'], images=d['images'],
                              pixel_centre=d['pixel_centre'], carve_weight=d['carve'], weights=d['weights'])


_MARK = ('atvs_tsdf_mark', 'atvs_tsdf_scan_scratch_size', 'atvs_tsdf_scan', 'atvs_tsdf_assign')
_FORM = {'plain': ('atvs_tsdf_integrate',), 'carve': ('atvs_tsdf_free_views', 'atvs_tsdf_integrate_carve'),
         'weighted': ('atvs_tsdf_integrate_weighted',), 'weighted+carve': ('atvs_tsdf_free_views', 'atvs_tsdf_integrate_weighted')}
_GATHERS = ('uneven', 'long_directory')          # marking is a strict superset of the occupied blocks (tests/tsdf_cases.py GATHER)


def _integrate_sizes():
    out = collections.OrderedDict()
    for scene, forms in (('one_block', ('plain', 'carve', 'weighted')), ('uneven', ('plain', 'carve', 'weighted', 'weighted+carve')),
                         ('long_directory', ('plain', 'carve')), ('views64', ('carve',)), ('views65', ('plain', 'carve', 'weighted+carve'))):
        for form in forms:
            out['%s,%s' % (scene, form)] = {'scene': scene, 'form': form,
                                            'entries': _MARK + _FORM[form] + (('atvs_tsdf_gather',) if scene in _GATHERS else ())}
    return out


Row('tsdf_integrate', _MARK + ('atvs_tsdf_integrate', 'atvs_tsdf_integrate_carve', 'atvs_tsdf_integrate_weighted', 'atvs_tsdf_free_views',
                               'atvs_tsdf_gather'),
    _integrate_sizes(), _integrate_inputs, _integrate_shapes, run=_integrate_run,
    select=lambda v: [v.blocks, v.tsdf, v.weight, v.color, v.free], names=('blocks', 'tsdf', 'weight', 'color', 'free'),
    outputs=('directory = torch.empty', 'err = torch.empty', 'total = torch.empty', 'coords = torch.empty', 'masks = torch.empty',
             'tsdf = torch.empty', 'weight = torch.empty', 'color = torch.empty', 'keep = torch.empty'),
    scratch=('scratch = torch.empty',),
    excluded=('the directory, the slot coordinates, the view masks and keep are intermediates between the launches (no header line '
              'gives them to the caller): they are held through the volume the launches that read them produce',),
    constants='a box of one block; (3,5,2) with a shifted pixel centre and the gather; a directory of 2431 words: a second scan '
              'tile of 2048; 64 and 65 views: the second mask word')


def _dense_inputs(p):
    from atvsnet_amd.ops import TsdfVolume
    rng = np.random.RandomState(39)
    nz, ny, nx = 8, 8, 8 * p['blocks']
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    tsdf = (np.sin(0.7 * x) + np.cos(0.9 * y) + 0.3 * (z - 3.5) + rng.normal(scale=0.05, size=x.shape)).astype(np.float32) * 0.4
    weight = rng.randint(0, 4, x.shape).astype(np.float32)
    weight[:, :, ::8] = np.maximum(weight[:, :, ::8], 1.0)                # every block keeps a voxel of weight > 0
    color = rng.uniform(0, 255, x.shape + (3,)).astype(np.float32)
    vol = TsdfVolume.from_dense(tsdf, weight, color, (0.5, -0.25, 1.0), 0.1, 0.3)
    assert vol.num_blocks == p['blocks']
    return {'blocks': vol.blocks, 'tsdf': vol.tsdf, 'weight': vol.weight, 'color': vol.color, 'dims': vol.dims}


def _mesh_run(ops, d, place):
    vol = ops.TsdfVolume((0.5, -0.25, 1.0), 0.1, 0.3, d['dims'], d['blocks'], d['tsdf'], d['weight'], d['color'])
    return ops.tsdf_mesh(vol, min_weight=1.0)


Row('tsdf_mesh', ('atvs_tsdf_mesh_count', 'atvs_tsdf_scan_scratch_size', 'atvs_tsdf_scan', 'atvs_tsdf_mesh_emit'), sizes('blocks', (1, 3, 4, 5, 9)),
    _dense_inputs,
    shapes=lambda p: {'blocks': ((p['blocks'], 3), I32), 'tsdf': ((p['blocks'], 8, 8, 8), F32), 'weight': ((p['blocks'], 8, 8, 8), F32),
                      'color': ((p['blocks'], 8, 8, 8, 3), F32)},
    run=_mesh_run, select=list, names=('vertices', 'colors', 'faces'),
    outputs=('cube_ok = torch.empty', 'emask = torch.empty', 'counts = torch.empty', 'totals = torch.empty', 'vertices = torch.empty',
             'faces = torch.empty'),
    scratch=('scratch = torch.empty',),
    constants='512 counters per block against the scan tile of 2048: 1 block, 3 | 4 | 5 blocks (one under, at, one over), 9 blocks '
              '(a third tile)')


# ============================================================================================================= ops/colmap.py
def _colmap_inputs(p):
    rng = np.random.RandomState(40)
    from scan_render_restated import ring_cameras
    c16 = ring_cameras(p['images'], 48, 64)
    cams = np.concatenate([c16, np.tile([64.0, 48.0], (p['images'], 1))], 1)
    return {'points': torch.from_numpy(rng.uniform(-1.0, 1.0, (p['points'], 3))), 'cams': torch.from_numpy(cams)}


Row('colmap_depth_range', ('atvs_colmap_depth_range_scratch_size', 'atvs_colmap_depth_range'),
    merged(sizes('points', (0, 1) + AROUND_WORKGROUP + (4095, 4096, 4097), images=3),
           sizes('images', (1, CAMERA_GROUP, CAMERA_GROUP + 1), points=300)),
    _colmap_inputs, shapes=lambda p: {'points': ((p['points'], 3), F64), 'cams': ((p['images'], 18), F64)},
    run=lambda ops, d, place: ops.colmap_depth_range(d['points'], d['cams'], 0.95), select=list, names=('n', 'd_lo', 'd_hi'),
    outputs=('n = torch.empty', 'd_lo = torch.empty', 'd_hi = torch.empty'), scratch=('scratch = torch.empty',),
    constants='kThreads 256; kRun 4096 points and kGroup 8 images per workgroup of the histogram pass')


def _tracks(p):
    rng = np.random.RandomState(41)
    lengths = rng.randint(2, min(p['images'], 6) + 1, p['tracks']) if p['images'] > 1 else np.ones(p['tracks'], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    observers = np.concatenate([rng.choice(p['images'], n, replace=False) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    return {'offsets': torch.from_numpy(offsets), 'observers': torch.from_numpy(observers), 'images': p['images']}


Row('colmap_covisibility', ('atvs_colmap_covisibility',),
    merged(sizes('tracks', (0, 1, 63, 64, 65) + AROUND_WORKGROUP, images=9), sizes('images', (1, 17), tracks=40)), _tracks,
    shapes=lambda p: {'offsets': ((p['tracks'] + 1,), I32), 'observers': (None, I32)},
    run=lambda ops, d, place: ops.colmap_covisibility(d['offsets'], d['observers'], d['images']), select=lambda r: [r], names=('covis',),
    outputs=('covis = torch.empty',), constants='kThreads 256 (four waves of tracks); the matrix is "zeroed" by the call (header line 780)')

_DISTORTION = ('OPENCV', (60.0, 58.0, 20.3, 14.6, 0.08, -0.02, 0.001, -0.002))


def _undistort_camera(wo, ho):
    return ((55.0, 54.0, wo / 2.0 + 0.3, ho / 2.0 - 0.2), (wo, ho))


UNDISTORT_SHAPES = collections.OrderedDict(('%dx%d' % s, {'wo': s[0], 'ho': s[1]}) for s in
                                           ((1, 1), (3, 1), (51, 5), (64, 4), (257, 1), (31, 23), (1023, 1), (32, 32), (41, 25)))

Row('undistort_map', ('atvs_undistort_map',), UNDISTORT_SHAPES, build=lambda p: dict(p), shapes=lambda p: {},
    run=lambda ops, d, place: ops.undistort_map(_DISTORTION[0], _DISTORTION[1], 40, 30, _undistort_camera(d['wo'], d['ho'])),
    select=lambda r: [r], names=('map',), outputs=('out = torch.empty',),
    constants='kThreads 256 output pixels per workgroup: 255 | 256 | 257 pixels, 713, 1023 | 1024 | 1025')


def _remap_inputs(p):
    rng = np.random.RandomState(42)
    q = np.stack([rng.randint(0, 39 * 1024 + 1, (p['ho'], p['wo'])), rng.randint(0, 29 * 1024 + 1, (p['ho'], p['wo']))], -1).astype(np.int32)
    q[rng.uniform(size=q.shape[:2]) < 0.2] = (-2 ** 31, 0)
    return {'image': torch.from_numpy(rng.randint(0, 256, (30, 40, 3)).astype(np.uint8)), 'map': torch.from_numpy(q)}


Row('undistort_remap', ('atvs_undistort_remap',), UNDISTORT_SHAPES, _remap_inputs,
    shapes=lambda p: {'image': ((30, 40, 3), U8), 'map': ((p['ho'], p['wo'], 2), I32)},
    run=lambda ops, d, place: ops.undistort_remap(d['image'], d['map']), select=lambda r: [r], names=('out',), outputs=('out = torch.empty',),
    constants='kPix 4 output pixels per thread, three dword stores, the last thread finishes Ho Wo mod 4 pixels by bytes: 1, 3, 255, '
              '256, 257, 713, 1023, 1024, 1025 pixels (every remainder; 1024 = 256 threads x 4)')


# ============================================================================================================ ops/prepare.py
def _prepare_run(ops, d, place):
    centred, quarter = ops.prepare_view(d['image'], d['scale'], d['crop'])
    return centred, quarter


PREPARE_SIZES = collections.OrderedDict((
    ('37x53 whole', {'h': 37, 'w': 53, 'scale': 1.0, 'crop': (0, 0, 37, 53)}),
    ('60x80 scaled, cropped to 23x31', {'h': 60, 'w': 80, 'scale': 0.5, 'crop': (3, 5, 23, 31)}),
    ('16x16 to 1x1', {'h': 16, 'w': 16, 'scale': 1.0, 'crop': (7, 7, 1, 1)}),
    ('64x64 cropped to 16x16', {'h': 64, 'w': 64, 'scale': 1.0, 'crop': (8, 8, 16, 16)}),
))

Row('prepare_view', ('atvs_prepare_resize_u8', 'atvs_prepare_center'), PREPARE_SIZES,
    build=lambda p: {'image': torch.from_numpy(np.random.RandomState(43).randint(0, 256, (p['h'], p['w'], 3)).astype(np.uint8)),
                     'scale': p['scale'], 'crop': p['crop']},
    shapes=lambda p: {'image': ((p['h'], p['w'], 3), U8)}, run=_prepare_run, select=list, names=('centred', 'quarter'),
    outputs=('out = (torch.empty', 'return (torch.empty'),
    excluded=('the cropped uint8 image and the six sums are the workspace of prepare_workspace, not returned: held through the centred '
              'image and the quarter image the launches that read them produce',),
    constants='maps of 1961, 713, 1 and 256 pixels; a 1 x 1 window has no quarter image (0 bytes)')


# ============================================================================== the fusion wrappers (ops/aanet.py) and depth normals
FusionShape = collections.namedtuple('FusionShape', 'n rows cols')
FUSION_SIZES = collections.OrderedDict((
    ('2x1x1', {'n': 2, 'rows': 1, 'cols': 1}), ('2x3x85', {'n': 2, 'rows': 3, 'cols': 85}), ('2x4x64', {'n': 2, 'rows': 4, 'cols': 64}),
    ('3x1x257', {'n': 3, 'rows': 1, 'cols': 257}), ('3x23x31', {'n': 3, 'rows': 23, 'cols': 31}), ('5x33x32', {'n': 5, 'rows': 33, 'cols': 32}),
))
FUSION_CONSTANTS = 'kRun 256 pixels per workgroup (fusion_grid.h): maps of 1, 255, 256, 257 and 713 pixels; 1056 pixels x 5 views: ' \
                   'kScanThreads 1024 of the scene compaction is crossed'


def _fusion_inputs(p):
    import fusion_cases as FC
    from atvsnet_amd.atvsnet import depth_fusion as DF
    Ps, depths, nrm, images, _ = FC.general_scene(p['n'], p['rows'], p['cols'], FC.OFFSETS[0], noise=0.004, seed=44)
    nd, img4 = FC.textures(depths, nrm, images)
    if nd.size >= 64:
        nd.reshape(-1, 4)[::11, 3] = 0.0                     # holes
    rng = np.random.RandomState(45)
    return {'cams': torch.from_numpy(DF.pack_cameras(Ps)), 'nd': torch.from_numpy(nd), 'images': torch.from_numpy(img4),
            'depth': torch.from_numpy(np.ascontiguousarray(1.0 / np.maximum(depths[0], 1e-3)).astype(np.float32)),
            'prob': torch.from_numpy(rng.uniform(0, 1, depths[0].shape).astype(np.float32)),
            'bgr': torch.from_numpy(np.ascontiguousarray(images[0]))}


def _fusion_shapes(p):
    n, r, c = p['n'], p['rows'], p['cols']
    return {'cams': ((n, 28), F32), 'nd': ((n, r, c, 4), F32), 'images': ((n, r, c, 4), F32), 'depth': ((r, c), F32), 'prob': ((r, c), F32),
            'bgr': ((r, c, 3), U8)}


Row('fusibile', ('atvs_fusibile',), FUSION_SIZES, _fusion_inputs, _fusion_shapes,
    run=lambda ops, d, place: ops.fusibile(d['cams'], d['nd'], d['images'], 1, 0.01, 0.5, 1), select=list,
    names=('coord', 'normal', 'texture', 'created'), outputs=('coord, normal, tex = ', 'created = _new'), constants=FUSION_CONSTANTS)


def _stage_run(ops, d, place):
    rows, cols = d['depth'].shape
    nd_out = torch.empty((rows, cols, 4), dtype=torch.float32, device=d['depth'].device)
    img_out = torch.empty((rows, cols, 4), dtype=torch.float32, device=d['depth'].device)
    return ops.fusion_stage(d['depth'], d['prob'], d['bgr'], True, 0.3, nd_out, img_out)


Row('fusion_stage', ('atvs_fusion_stage_f32',), FUSION_SIZES, _fusion_inputs, _fusion_shapes, run=_stage_run, select=list,
    names=('nd_out', 'img_out'), outputs=('nd_out = torch.empty', 'img_out = torch.empty'), constants=FUSION_CONSTANTS)

Row('depth_normals', ('atvs_depth_normals_f32',), FUSION_SIZES, _fusion_inputs, _fusion_shapes,
    run=lambda ops, d, place: ops.depth_normals(d['cams'], d['nd'], step=1, depth_gate=0.05), select=lambda r: [r],
    names=('normals_depths (in place)',), outputs=(), writable=('nd',), constants=FUSION_CONSTANTS)

Row('fusibile_scene', ('atvs_fusibile_scene_scratch_size', 'atvs_fusibile_scene'), FUSION_SIZES, _fusion_inputs, _fusion_shapes,
    run=lambda ops, d, place: ops.fusibile_scene(d['cams'], d['nd'], d['images'], 0.01, 0.5, 1), select=list, names=('points[:M]', 'colors[:M]'),
    outputs=('points = torch.empty', 'colors = torch.empty', 'count = torch.empty'), scratch=('scratch = torch.empty',),
    excluded=('rows M.. of points and colors: "the first *n_points rows written", header line 651',), constants=FUSION_CONSTANTS)

Row('fusibile_scene_normals', ('atvs_fusibile_scene_normals_scratch_size', 'atvs_fusibile_scene_normals'), FUSION_SIZES, _fusion_inputs,
    _fusion_shapes, run=lambda ops, d, place: ops.fusibile_scene(d['cams'], d['nd'], d['images'], 0.01, 0.5, 1, with_normals=True),
    select=list, names=('points[:M]', 'colors[:M]', 'normals[:M]'),
    outputs=('points = torch.empty', 'colors = torch.empty', 'count = torch.empty', 'outputs = [points, colors]'), scratch=('scratch = torch.empty',),
    excluded=('rows M.. of points, colors and normals: "the first *n_points rows written", header line 651, and "for every kept point", '
              'line 658',),
    constants=FUSION_CONSTANTS)

Row('fusion_support', ('atvs_fusion_support',), FUSION_SIZES, _fusion_inputs, _fusion_shapes,
    run=lambda ops, d, place: ops.fusion_support(d['cams'], d['nd'], 0.01, 0.5, 1), select=lambda r: [r['count'], r['depth'], r['weight']],
    names=('count', 'depth', 'weight'), outputs=('out = {w: torch.empty',), constants=FUSION_CONSTANTS)


# ----------------------------------------------------------------------------------------------------- what no row covers, and why
EXCLUDED_ENTRY_POINTS = {}           # nothing: the network side, once listed here, has its own table (tests/network_contract_rows.py)
