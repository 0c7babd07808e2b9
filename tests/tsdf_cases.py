"""Inputs that tell a correct TSDF kernel from the plausible wrong ones, built deterministically (fixed seeds), and for each the
conditions that make it discriminate, asserted on tests/tsdf_restated.py ALONE (`check_*`): tests/test_tsdf_cases_host.py runs
every builder and its conditions without a GPU, so an edit here cannot hollow tests/test_gpu_tsdf_cases.py out.  With them the two
bit-exact comparisons the GPU files share.

Integration cases are `Integration` objects (depths, cams, images and the box; `.want` is the dense restatement, once), extraction
cases are `Dense` objects (dense [z][y][x] arrays for TsdfVolume.from_dense; `.want(min_weight)` is the restated mesh, once)."""
import functools
import itertools

import numpy as np

import tsdf_restated as R
from scan_render_restated import ring_cameras

VOXEL = 0.05
UNEVEN_DIMS = (3, 5, 2)
UNEVEN_ORIGIN = (-0.613, -1.007, -0.391)
INVALID = (0.0, float('nan'), float('inf'), -1.0, float('-inf'))          # the five classes of a depth that is no sample
NO_COLOUR = 1e30                                                           # what the fourth channel holds: no colour can be this


# ----------------------------------------------------------------------------------------------------------------------------------
# the two comparisons: bits
# ----------------------------------------------------------------------------------------------------------------------------------
def _volume_equal(vol, want):
    assert np.array_equal(vol.blocks.cpu().numpy(), want['blocks'])
    f, w, c = vol.to_dense()
    assert np.array_equal(f.view(np.uint32), want['tsdf'].view(np.uint32))
    assert np.array_equal(w, want['weight'])
    if want['color'] is None:
        assert c is None
    else:
        assert np.array_equal(c.view(np.uint32), want['color'].view(np.uint32))
    # exactly the blocks with a voxel of weight > 0
    assert bool((vol.weight.reshape(vol.num_blocks, -1) > 0).any(dim=1).all())


def _mesh_equal(got, want):
    import torch
    v, c, f = got
    assert np.array_equal(v.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    if want[1] is None:
        assert c is None
    else:
        assert c.dtype == torch.uint8 and np.array_equal(c.cpu().numpy(), want[1])
    assert f.dtype == torch.int32 and np.array_equal(f.cpu().numpy(), want[2])


def _mesh_equal_but_for_nan_bits(got, want):
    """_mesh_equal where a vertex coordinate may be a NaN: the same coordinates are NaN and every other one has the same bits (the
    sign and payload of a generated NaN differ between processors); colours and faces exactly."""
    import torch
    v, c, f = got
    v = v.cpu().numpy()
    assert v.dtype == np.float32 and v.shape == want[0].shape
    nan = np.isnan(want[0])
    assert np.array_equal(np.isnan(v), nan)
    assert np.array_equal(v.view(np.uint32)[~nan], want[0].view(np.uint32)[~nan])
    if want[1] is None:
        assert c is None
    else:
        assert c.dtype == torch.uint8 and np.array_equal(c.cpu().numpy(), want[1])
    assert f.dtype == torch.int32 and np.array_equal(f.cpu().numpy(), want[2])


# ----------------------------------------------------------------------------------------------------------------------------------
# integration
# ----------------------------------------------------------------------------------------------------------------------------------
class Integration(object):
    def __init__(self, depths, cams, images, trunc, origin, dims, pixel_centre=0.0, voxel=VOXEL, **notes):
        self.depths = np.ascontiguousarray(depths, np.float32)
        self.cams = np.ascontiguousarray(cams, np.float64)
        self.images = None if images is None else np.ascontiguousarray(images, np.float32)
        self.trunc, self.origin, self.dims, self.pixel_centre, self.voxel = trunc, origin, dims, pixel_centre, voxel
        self.notes = notes                                # what a check needs beside the inputs
        self._want, self._mesh = None, {}

    def restate(self, depths=None, pixel_centre=None):
        return R.integrate(self.depths if depths is None else depths, self.cams, self.voxel, self.trunc, self.origin, self.dims,
                           self.images, self.pixel_centre if pixel_centre is None else pixel_centre)

    @property
    def want(self):
        if self._want is None:
            self._want = self.restate()
        return self._want

    def want_mesh(self, min_weight=1.0):
        if min_weight not in self._mesh:
            w = self.want
            self._mesh[min_weight] = R.mesh(w['tsdf'], w['weight'], w['color'], self.origin, self.voxel, min_weight)
        return self._mesh[min_weight]

    def linear_blocks(self):
        b = self.want['blocks'].astype(np.int64)
        return (b[:, 2] * self.dims[1] + b[:, 1]) * self.dims[0] + b[:, 0]


def marked_blocks(case, centre_in_corners=True):
    """The marking of include/atvsnet_hip.h restated: the sorted linear indices of the blocks that the box of some pixel's frustum
    segment [max(d - trunc, 0), d + trunc], padded by a voxel, meets.  centre_in_corners=False forms the corners at u +- 0.5 without
    the pixel centre: what a marking that forgot it would find."""
    n, rows, cols = case.depths.shape
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    shift = float(case.pixel_centre) if centre_in_corners else 0.0
    org, nb, edge = np.array(case.origin, np.float64), np.array(case.dims), 8.0 * case.voxel
    found = np.zeros(case.dims[::-1], bool)              # [z][y][x]
    for k, c in enumerate(case.cams):
        d = case.depths[k].astype(np.float64)
        with np.errstate(invalid='ignore'):
            live = (case.depths[k] > 0) & np.isfinite(case.depths[k])
        inverse, t = np.linalg.inv(c[:9].reshape(3, 3)), c[9:12]
        lo, hi = np.full((rows, cols, 3), np.inf), np.full((rows, cols, 3), -np.inf)
        for sx, sy, far in itertools.product((-0.5, 0.5), (-0.5, 0.5), (False, True)):
            z = np.where(live, d + case.trunc if far else np.maximum(d - case.trunc, 0.0), 1.0)
            cam = np.stack([((u + shift) + sx - c[14]) / c[12] * z, ((v + shift) + sy - c[15]) / c[13] * z, z], axis=-1)
            P = (cam - t) @ inverse.T
            lo, hi = np.minimum(lo, P), np.maximum(hi, P)
        low = np.floor(((lo - case.voxel) - org) / edge).astype(np.int64)
        high = np.floor(((hi + case.voxel) - org) / edge).astype(np.int64)
        live &= ((high >= 0) & (low <= nb - 1)).all(axis=-1)
        low, high = np.maximum(low, 0), np.minimum(high, nb - 1)
        for y, x in zip(*np.nonzero(live)):
            (x0, y0, z0), (x1, y1, z1) = low[y, x], high[y, x]
            found[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
    return np.flatnonzero(found)


def _same(a, b):
    return np.array_equal(a['weight'], b['weight']) and np.array_equal(a['tsdf'].view(np.uint32), b['tsdf'].view(np.uint32))


UNEVEN_TRUNCS = (0.2, 0.03, 0.9)                         # 4 voxels; below one voxel; above the block edge of 0.4


@functools.lru_cache(maxsize=None)
def uneven(trunc, with_images=True, seed=0):
    """Case 1: the box (3,5,2), per-pixel random depths with about 15 % of the five invalid classes, the left half of the columns
    and the top third of the rows zeroed, pixel centre 0.5, four channels."""
    rows, cols = 23, 31
    n, lo, hi = (3, 3.3, 3.6) if trunc == 0.9 else (5, 2.9, 3.2)
    rng = np.random.RandomState(seed)
    base = rng.uniform(lo, hi, (n, rows, cols)).astype(np.float32)
    cls = np.where(rng.uniform(size=base.shape) < 0.15, rng.randint(0, 5, base.shape), -1)
    depths = base.copy()
    for k, value in enumerate(INVALID):
        depths[cls == k] = value
    for a in (base, depths):
        a[:, :, :cols // 2] = 0
        a[:, :rows // 3, :] = 0
    images = None
    if with_images:
        images = np.full((n, rows, cols, 4), NO_COLOUR, np.float32)
        images[..., :3] = rng.uniform(0, 255, (n, rows, cols, 3))
    return Integration(depths, ring_cameras(n, rows, cols), images, trunc, UNEVEN_ORIGIN, UNEVEN_DIMS, pixel_centre=0.5,
                       base=base, cls=cls)


def check_uneven(case):
    want = case.want
    assert 4 <= len(want['blocks']) < 30
    assert 29 in case.linear_blocks().tolist()
    assert want['weight'].max() >= 3
    assert not _same(want, case.restate(pixel_centre=0.0))
    if case.images is not None:
        assert case.images.shape[-1] == 4 and (case.images[..., 3] == np.float32(NO_COLOUR)).all()
        assert want['color'].max() <= 255.0
    d = case.depths
    live = (slice(None), slice(d.shape[1] // 3, None), slice(d.shape[2] // 2, None))
    for k, value in enumerate(INVALID):
        mine = case.notes['cls'][live] == k
        assert mine.any()
        assert np.array_equal(d[live][mine], np.full(int(mine.sum()), value, np.float32), equal_nan=True)
        healed = np.where(case.notes['cls'] == k, case.notes['base'], d)
        assert not np.array_equal(case.restate(depths=healed)['weight'], want['weight']), value


@functools.lru_cache(maxsize=None)
def lone_pixels(seed=3):
    """Coarse 5 x 7 maps with one live pixel each, pixel centre 0.5: a pixel's footprint at its depth (0.48) is wider than a block
    (0.4), so half a pixel is far more than the voxel the marking box is padded by -- corners formed without the pixel centre leave
    blocks with contributing voxels unmarked.  (At 23 x 31 half a pixel is a voxel, and the padding hides that mistake.)"""
    rows, cols, n = 5, 7, 3
    rng = np.random.RandomState(seed)
    base = rng.uniform(2.9, 3.2, (n, rows, cols)).astype(np.float32)
    depths = np.zeros_like(base)
    for k, (y, x) in enumerate(((2, 3), (1, 4), (3, 2))):
        depths[k, y, x] = base[k, y, x]
    images = rng.uniform(0, 255, (n, rows, cols, 3)).astype(np.float32)
    return Integration(depths, ring_cameras(n, rows, cols), images, 0.2, (-1.013, -0.807, -0.991), (5, 4, 5), pixel_centre=0.5)


def check_lone_pixels(case):
    occupied = set(case.linear_blocks().tolist())
    assert len(occupied) >= 10 and (case.depths > 0).sum(axis=(1, 2)).tolist() == [1, 1, 1]
    assert occupied <= set(marked_blocks(case).tolist())
    assert len(occupied - set(marked_blocks(case, centre_in_corners=False).tolist())) >= 3
    assert not _same(case.want, case.restate(pixel_centre=0.0))


def check_marking_is_a_strict_superset(case):
    """Marking finds every occupied block and some that stay empty: with max_blocks = the marked count the gather path runs."""
    occupied, marked = set(case.linear_blocks().tolist()), set(marked_blocks(case).tolist())
    assert occupied < marked
    return len(marked)


@functools.lru_cache(maxsize=None)
def full_box(seed=1):
    """Case 2: the box (2,1,3) inside the band of every pixel: every block is occupied."""
    rows, cols, n = 23, 31, 3
    rng = np.random.RandomState(seed)
    depths = rng.uniform(2.9, 3.1, (n, rows, cols)).astype(np.float32)
    images = rng.uniform(0, 255, (n, rows, cols, 3)).astype(np.float32)
    return Integration(depths, ring_cameras(n, rows, cols), images, 0.9, (-0.413, -0.207, -0.591), (2, 1, 3))


def check_full_box(case):
    assert case.linear_blocks().tolist() == list(range(6))          # the first and the last directory word, the last slot kept
    assert case.want['weight'].max() >= 2


@functools.lru_cache(maxsize=None)
def camera_inside(seed=2):
    """Case 3: two cameras whose centres lie inside the box, depths below and above trunc."""
    rows, cols, n = 23, 31, 2
    rng = np.random.RandomState(seed)
    depths = rng.uniform(0.05, 0.6, (n, rows, cols)).astype(np.float32)
    images = rng.uniform(0, 255, (n, rows, cols, 3)).astype(np.float32)
    return Integration(depths, ring_cameras(n, rows, cols, radius=0.3, height=0.1), images, 0.2, UNEVEN_ORIGIN, UNEVEN_DIMS)


def check_camera_inside(case):
    want = case.want
    assert (want['weight'] > 0).any()
    org, dims = np.array(case.origin), np.array(case.dims)
    Z, Y, X = np.meshgrid(*[R.centres(case.origin, case.voxel, dims[a] * 8, a) for a in (2, 1, 0)], indexing='ij')
    for c in case.cams:
        centre = -c[:9].reshape(3, 3).T @ c[9:12]
        assert (centre > org).all() and (centre < org + dims * 8 * case.voxel).all()
        c2 = ((c[6] * X + c[7] * Y) + c[8] * Z) + c[11]
        assert (c2 <= 0).any() and (c2 > 0).any()
    # a contributing pixel with d < trunc: d - trunc < 0 is clamped in marking
    near = case.depths < np.float32(case.trunc)
    assert near.any() and (~near).any()
    assert not np.array_equal(case.restate(depths=np.where(near, np.float32(0), case.depths))['weight'], want['weight'])


MASK_LIVE = ((31,), (32,), (63,), (31, 32, 63))


@functools.lru_cache(maxsize=None)
def mask_bits(live):
    """Case 4: 64 ring cameras with 5 x 7 maps of the sphere of radius 0.9, the depths zeroed except in the views `live`."""
    rows, cols, n = 5, 7, 64
    cams = ring_cameras(n, rows, cols)
    depths, images = R.sphere_depths(cams, rows, cols, 0.9)
    keep = np.zeros(n, bool)
    keep[list(live)] = True
    depths[~keep] = 0
    return Integration(depths, cams, images, 0.2, (-1.237, -1.181, -1.213), (6, 6, 6))


def check_mask_bits(case, live):
    top = case.want['weight'].max()
    assert (case.depths.reshape(64, -1) > 0).any(axis=1).nonzero()[0].tolist() == list(live)
    assert top == 1 if len(live) == 1 else top >= 2


@functools.lru_cache(maxsize=None)
def long_directory():
    """Case 5: a directory of 13 * 17 * 11 = 2431 words, longer than one scan tile of 2048, around the sphere of radius 0.9."""
    rows, cols, n = 37, 53, 3
    cams = ring_cameras(n, rows, cols)
    depths, images = R.sphere_depths(cams, rows, cols, 0.9)
    return Integration(depths, cams, images, 0.2, (-2.613, -3.407, -3.191), (13, 17, 11))


def check_long_directory(case):
    lin = case.linear_blocks()
    assert int(np.prod(case.dims)) > 2048
    assert (lin < 2048).sum() >= 8 and (lin >= 2048).sum() >= 8
    org, dims = np.array(case.origin), np.array(case.dims)
    centres = [-c[:9].reshape(3, 3).T @ c[9:12] for c in case.cams]
    assert any((c > org).all() and (c < org + dims * 8 * case.voxel).all() for c in centres)      # a camera stands inside this box


GATHER = ('uneven', 'long_directory')


def gather_case(name):
    """Case 6: the cases whose marking is a strict superset of their occupied blocks."""
    return uneven(0.2) if name == 'uneven' else long_directory()


# ----------------------------------------------------------------------------------------------------------------------------------
# extraction
# ----------------------------------------------------------------------------------------------------------------------------------
class Dense(object):
    """Dense [z][y][x] arrays for TsdfVolume.from_dense.  `ref_weight` is the weight the restatement is given where it must differ:
    from_dense pads to whole blocks and drops the blocks without a weight > 0, and a voxel of a missing block is never valid, which
    under min_weight <= 0 the dense restatement only knows if those voxels carry a NaN weight."""
    def __init__(self, tsdf, weight, color, origin=(0.5, -0.25, 1.0), voxel=0.1, **notes):
        self.tsdf = np.ascontiguousarray(tsdf, np.float32)
        self.weight = np.ascontiguousarray(weight, np.float32)
        self.color = None if color is None else np.ascontiguousarray(color, np.float32)
        self.origin, self.voxel, self.notes = origin, voxel, notes
        self._mesh = {}

    def volume(self, ops, device='cuda'):
        return ops.TsdfVolume.from_dense(self.tsdf, self.weight, self.color, self.origin, self.voxel, 4 * self.voxel, device=device)

    def as_the_volume_holds_it(self):
        """(tsdf, weight, color) padded to whole blocks with zeros, the weight NaN in every block without a weight > 0."""
        nz, ny, nx = self.tsdf.shape
        pad = [(0, -nz % 8), (0, -ny % 8), (0, -nx % 8)]
        f, w = np.pad(self.tsdf, pad), np.pad(self.weight, pad)
        c = None if self.color is None else np.pad(self.color, pad + [(0, 0)])
        bz, by, bx = (s // 8 for s in f.shape)
        with np.errstate(invalid='ignore'):
            present = (w > 0).reshape(bz, 8, by, 8, bx, 8).any(axis=(1, 3, 5))
        present = np.repeat(np.repeat(np.repeat(present, 8, axis=0), 8, axis=1), 8, axis=2)
        return f, np.where(present, w, np.float32('nan')), c

    def want(self, min_weight=1.0, with_edges=False):
        key = (min_weight, with_edges)
        if key not in self._mesh:
            f, w, c = self.as_the_volume_holds_it() if min_weight <= 0 else (self.tsdf, self.weight, self.color)
            self._mesh[key] = R.mesh(f, w, c, self.origin, self.voxel, min_weight, with_edges=with_edges)
        return self._mesh[key]

    def cubes(self, min_weight=1.0):
        """-> (meshed (nz-1,ny-1,nx-1) bool: all 8 corners valid and the signs mixed, pattern: the corners' INSIDE bits, corner
        dx + 2 dy + 4 dz, valid: all 8 corners valid), from the arrays alone."""
        with np.errstate(invalid='ignore'):
            valid, inside = self.weight >= np.float32(min_weight), self.tsdf < 0
        nz, ny, nx = self.tsdf.shape
        ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
        pattern = np.zeros(ok.shape, np.int64)
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
            ok &= valid[sl]
            pattern |= inside[sl].astype(np.int64) << (dx + 2 * dy + 4 * dz)
        return ok & (pattern != 0) & (pattern != 255), pattern, ok

    def at_meshed_corners(self, flags, min_weight=1.0):
        """How many corners of meshed cubes have `flags` (a bool array over the voxels) set."""
        meshed = self.cubes(min_weight)[0]
        nz, ny, nx = self.tsdf.shape
        total = 0
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            total += int((meshed & flags[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]).sum())
        return total

    def colour_expressions(self, min_weight=1.0):
        """(V,3) float64: ca + t * (cb - ca) of every vertex of the restated mesh, b, g, r -- what the colour rule is applied to."""
        f, _, c = self.as_the_volume_holds_it() if min_weight <= 0 else (self.tsdf, self.weight, self.color)
        owned = self.want(min_weight, with_edges=True)[3]
        a = np.array([e[0] for e in owned], np.int64).reshape(-1, 3)
        b = a + np.array([R.EDGES[e[1]] for e in owned], np.int64).reshape(-1, 3)
        fa, fb = f[a[:, 2], a[:, 1], a[:, 0]].astype(np.float64), f[b[:, 2], b[:, 1], b[:, 0]].astype(np.float64)
        ca, cb = c[a[:, 2], a[:, 1], a[:, 0]].astype(np.float64), c[b[:, 2], b[:, 1], b[:, 0]].astype(np.float64)
        with np.errstate(all='ignore'):
            t = fa / (fa - fb)
            return ca + t[:, None] * (cb - ca)


def _random_arrays(shape, seed):
    rng = np.random.RandomState(seed)
    f = rng.uniform(-1, 1, shape).astype(np.float32)
    w = rng.randint(0, 4, shape).astype(np.float32)
    w[rng.uniform(size=shape) < 0.6] = 3
    c = rng.uniform(-40, 300, shape + (3,)).astype(np.float32)
    return rng, f, w, c


RANDOM_MIN_WEIGHTS = (1.0, 2.5)


@functools.lru_cache(maxsize=None)
def random_signs(seed=7):
    """Case 7: random tsdf, weights 0..3 and colours beyond both clamps on the box (3,5,2)."""
    _, f, w, c = _random_arrays((11, 37, 19), seed)
    return Dense(f, w, c)


def check_random_signs(case):
    assert tuple(-(-s // 8) for s in case.tsdf.shape[::-1]) == (3, 5, 2)
    meshed, pattern, valid = case.cubes(1.0)
    assert len(set(pattern[valid].tolist())) == 256                  # every sign pattern of a cube's 8 corners among the valid cubes
    assert len(set(pattern[meshed].tolist())) == 254                 # ... and all but the two without a surface are meshed
    v, col, f = case.want(1.0)
    assert len(v) > 10000 and len(f) > 15000
    assert (col == 0).sum() > 100 and (col == 255).sum() > 100     # both colour clamps
    x = case.colour_expressions(1.0)
    assert (x < -0.5).any() and (x > 255.5).any()
    v2, _, f2 = case.want(2.5)
    assert 0 < len(f2) < len(f) and 0 < len(v2) < len(v)
    for faces in (f, f2):
        directed, undirected = R.edge_stats(faces)
        assert max(undirected.values()) <= 2 and max(directed.values()) == 1


@functools.lru_cache(maxsize=None)
def sphere():
    """Case 8: the exact distance field of a sphere, 32^3, all weights 1."""
    f = R.sphere_field(32)
    return Dense(f, np.ones_like(f), None, origin=(0.0, 0.0, 0.0), voxel=1.0)


def check_sphere(case):
    v, c, f = case.want(1.0)
    directed, undirected = R.edge_stats(f)
    assert c is None and (len(v), len(f)) == (5946, 11888) and len(v) - len(undirected) + len(f) == 2
    assert all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())


ZEROS = ('plus', 'minus', 'denormal')
SMALL = (9, 13, 10)                                     # [z][y][x]: dims (2,2,2) after padding


@functools.lru_cache(maxsize=None)
def zeros(kind, seed=9):
    """Case 9: the random field with about 20 % of the voxels +0.0, -0.0, or float32 denormals of both signs."""
    rng, f, w, c = _random_arrays(SMALL, seed)
    at = rng.uniform(size=SMALL) < 0.2
    if kind == 'plus':
        f[at] = 0.0
    elif kind == 'minus':
        f[at] = -0.0
    else:
        tiny = np.array([1, 0x7fffff, 0x80000001, 0x807fffff, 0x00012345, 0x80054321], np.uint32).view(np.float32)
        f[at] = tiny[rng.randint(0, len(tiny), int(at.sum()))]
    return Dense(f, w, c, at=at)


def check_zeros(case, kind):
    at, f = case.notes['at'], case.tsdf
    assert 0.1 < at.mean() < 0.3
    if kind == 'denormal':
        assert (np.abs(f[at]) < np.finfo(np.float32).tiny).all() and (f[at] != 0).all()
        assert case.at_meshed_corners(at & (f < 0)) > 20 and case.at_meshed_corners(at & (f > 0)) > 20
    else:
        assert (f[at] == 0).all() and (np.signbit(f[at]) == (kind == 'minus')).all()
        assert case.at_meshed_corners(at) > 50
    assert len(case.want(1.0)[2]) > 500


SPECIALS = ('nan_tsdf', 'inf_tsdf', 'only_inf', 'colours', 'weights', 'min_weight_0', 'min_weight_-inf', 'min_weight_+inf')


def special_min_weight(kind):
    return {'min_weight_0': 0.0, 'min_weight_-inf': float('-inf'), 'min_weight_+inf': float('inf')}.get(kind, 1.0)


@functools.lru_cache(maxsize=None)
def special(kind, seed=10):
    """Case 10: NaN and infinite tsdf, colours and weights, and the min_weight that no finite weight passes or fails."""
    nan, inf = np.float32('nan'), np.float32('inf')
    if kind.startswith('min_weight'):
        rng, f, w, c = _random_arrays((16, 16, 16), seed)
        if kind == 'min_weight_+inf':
            w[2:9, 3:10, 1:11] = inf                    # only these are valid
            w[4, 5, 6] = 3
        else:
            w[rng.uniform(size=w.shape) < 0.05] = nan   # not valid under any min_weight
            w[:, 8:, 8:] = 0                            # the blocks (1,1,*) are absent
            f[rng.uniform(size=f.shape) < 0.05] = nan
            c[rng.uniform(size=f.shape) < 0.05] = inf
        return Dense(f, w, c)
    rng, f, w, c = _random_arrays(SMALL, seed)
    u = rng.uniform(size=SMALL)
    if kind == 'nan_tsdf':
        f[u < 0.1] = nan
    elif kind == 'inf_tsdf':
        f[u < 0.2] = inf
        f[u > 0.97] = -inf
    elif kind == 'only_inf':
        f = np.where(u < 0.5, inf, -inf).astype(np.float32)
    elif kind == 'colours':
        u3 = rng.uniform(size=SMALL + (3,))
        c[u3 < 0.1] = rng.choice(np.array([nan, inf, -inf], np.float32), int((u3 < 0.1).sum()))
    elif kind == 'weights':
        w[u < 0.1] = nan
        w[u > 0.9] = inf
    return Dense(f, w, c)


def check_special(case, kind):
    mw = special_min_weight(kind)
    v, col, faces, owned = case.want(mw, with_edges=True)
    assert len(faces) > 0 and len(v) > 0
    x = case.colour_expressions(mw)
    rule = np.where(np.floor(x + 0.5) >= 0, np.floor(x + 0.5), 0.0)
    rule = np.where(rule <= 255, rule, 255.0).astype(np.uint8)[:, ::-1]
    assert np.array_equal(rule, col)                                 # the rule, vectorised
    f, w = case.tsdf, case.weight
    if kind == 'nan_tsdf':
        assert case.at_meshed_corners(np.isnan(f)) > 20 and np.isnan(v).any() and np.isnan(x).any()
    elif kind == 'inf_tsdf':
        assert case.at_meshed_corners(np.isposinf(f)) > 20 and case.at_meshed_corners(np.isneginf(f)) > 0
        assert np.isnan(v).any()                                     # -inf against +inf: t = inf / inf
    elif kind == 'only_inf':
        assert np.isinf(f).all() and np.isnan(v).all() and (col == 0).all()
    elif kind == 'colours':
        assert not np.isnan(v).any()
        assert np.isnan(x).any() and np.isneginf(x).any() and np.isposinf(x).any()
        assert (col[np.isnan(x)[:, ::-1]] == 0).all() and (col[np.isneginf(x)[:, ::-1]] == 0).all()
        assert (col[np.isposinf(x)[:, ::-1]] == 255).all()
    elif kind == 'weights':
        assert np.isnan(w).sum() > 50 and np.isposinf(w).sum() > 50
        assert case.at_meshed_corners(np.isnan(w)) == 0 and case.at_meshed_corners(np.isposinf(w)) > 20
        owners = np.array([e[0] for e in owned])
        assert not np.isnan(w[owners[:, 2], owners[:, 1], owners[:, 0]]).any()
    elif kind in ('min_weight_0', 'min_weight_-inf'):
        fp, wp, _ = case.as_the_volume_holds_it()
        assert np.isnan(wp[:, 8:, 8:]).all() and (w[:, 8:, 8:] == 0).all()          # the absent blocks: never valid
        assert np.isnan(w[:, :8, :]).sum() > 20
        owners = np.array([e[0] for e in owned])
        ow = wp[owners[:, 2], owners[:, 1], owners[:, 0]]
        assert (ow == 0).any() and not np.isnan(ow).any()           # weight 0 is valid here, in a present block
        upper = owners + np.array([R.EDGES[e[1]] for e in owned])
        assert not ((upper[:, 1] >= 8) & (upper[:, 0] >= 8)).any()                  # nothing is meshed towards the absent blocks
        assert ((upper[:, 1] == 7) & (upper[:, 0] >= 8)).any() and ((upper[:, 1] >= 8) & (upper[:, 0] == 7)).any()
        assert np.isnan(v).any() and np.isposinf(x).any()
        assert len(faces) > len(case.want(1.0)[2])
    elif kind == 'min_weight_+inf':
        owners = np.array([e[0] for e in owned])
        assert owners[:, 0].min() >= 1 and owners[:, 0].max() <= 10 and owners[:, 2].min() >= 2 and owners[:, 2].max() <= 8
        meshed = case.cubes(mw)[0]
        assert meshed.any() and not meshed[3:5, 4:6, 5:7].any()      # the finite weight in their middle is not valid


@functools.lru_cache(maxsize=None)
def _corner_field():
    """A 16^3 field with an oblique plane through the corner that the eight blocks share: the cube of voxel (7,7,7) is meshed."""
    rng = np.random.RandomState(11)
    a = np.arange(16, dtype=np.float64)
    Z, Y, X = np.meshgrid(a, a, a, indexing='ij')
    f = (0.11 * (X - 7.6) + 0.07 * (Y - 7.3) - 0.05 * (Z - 7.8)).astype(np.float32)
    return f, rng.uniform(0, 255, (16, 16, 16, 3)).astype(np.float32)


ABSENT = tuple([('one',) + b for b in itertools.product((0, 1), repeat=3)] + [('diagonal', 0, 0, 0)] +
               [('slab', axis, side) for axis in range(3) for side in (0, 1)])


def _absent_blocks(variant):
    """The blocks (x, y, z) a variant takes away."""
    if variant[0] == 'one':
        return [variant[1:]]
    if variant[0] == 'diagonal':
        return [(0, 0, 0), (1, 1, 1)]
    _, axis, side = variant
    return [b for b in itertools.product((0, 1), repeat=3) if b[axis] == side]      # the four blocks that share an axis' edge


@functools.lru_cache(maxsize=None)
def absent(variant):
    """Case 11: the eight blocks of a 16^3 box, some taken away through their weight: each alone (a neighbour missing across a face,
    an edge or the corner, depending on where one stands), a diagonal pair, the four blocks on either side of each axis."""
    f, c = _corner_field()
    w = np.ones_like(f)
    for x, y, z in ([] if variant is None else _absent_blocks(variant)):
        w[z * 8:z * 8 + 8, y * 8:y * 8 + 8, x * 8:x * 8 + 8] = 0
    return Dense(f, w, c)


def check_absent(case, variant):
    whole = absent(None)
    assert whole.cubes()[0][7, 7, 7]
    v, c, f = case.want(1.0)
    assert len(f) > 0 and len(f) < len(whole.want(1.0)[2])
    assert not case.cubes()[0][7, 7, 7]
    gone = _absent_blocks(variant)
    assert case.volume(_host_ops(), device=None).num_blocks == 8 - len(gone)


def _host_ops():
    from atvsnet_amd import ops
    return ops


THIN = ((4, 1, 1), (1, 4, 1), (1, 1, 4))


@functools.lru_cache(maxsize=None)
def thin(dims):
    """Boxes one block thick with a plane oblique to the long axis: each axis' block stride alone."""
    long_axis = dims.index(4)
    n = [8 * d for d in dims]
    axes = [np.arange(s, dtype=np.float64) for s in n]
    Z, Y, X = np.meshgrid(axes[2], axes[1], axes[0], indexing='ij')
    P = [X, Y, Z]
    other = [a for a in range(3) if a != long_axis]
    f = (0.21 * (P[other[0]] - 3.6) + 0.04 * (P[long_axis] - 15.3) + 0.09 * (P[other[1]] - 3.2)).astype(np.float32)
    rng = np.random.RandomState(12)
    return Dense(f, np.ones_like(f), rng.uniform(0, 255, f.shape + (3,)).astype(np.float32))


def check_thin(case, dims):
    assert case.tsdf.shape == (8 * dims[2], 8 * dims[1], 8 * dims[0])
    owned = case.want(1.0, with_edges=True)[3]
    long_axis = dims.index(4)
    assert sorted({e[0][long_axis] >> 3 for e in owned}) == [0, 1, 2, 3]          # the surface runs through all four blocks
    assert len(case.want(1.0)[2]) > 200
