"""-m gpu: scene mode (atvsnet/scene.py, eval_pointcloud --scene_cache).

The view preparation kernels (csrc/prepare.hip) against scale_image / crop_mvs_input / center_image; the scene's maps from cached
tower features bit for bit the per-map captured graph on the same prepared views; one tower pass per image; the driver end to end
against the default driver; the fp32 range rule with cached features."""
import collections
import os

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS, ops, synthetic, variables
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import example as ex
from atvsnet_amd.atvsnet import preprocess as P
from atvsnet_amd.atvsnet import scene as S

pytestmark = pytest.mark.gpu


@pytest.fixture
def flags():
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


def _reference_view(img, scale, max_h, max_w):
    old = (FLAGS.view_num, FLAGS.max_h, FLAGS.max_w)
    FLAGS.view_num, FLAGS.max_h, FLAGS.max_w = 1, max_h, max_w
    try:
        out, _ = P.crop_mvs_input([P.scale_image(img, scale)], [np.zeros((2, 4, 4))], base_image_size=32)
        return out[0]
    finally:
        FLAGS.view_num, FLAGS.max_h, FLAGS.max_w = old


@pytest.mark.parametrize('h,w,scale,max_h,max_w', [
    (490, 940, 0.98, 480, 896),         # the driver's default shape: a crop on both axes
    (131, 203, 1.0, 96, 160),           # odd sizes
    (257, 333, 0.5, 64, 128),
    (517, 611, 0.25, 96, 128),
    (77, 45, 1.0, 1, 1),                # one row / one column
])
def test_resize_and_quarter_image_are_bit_exact(cuda, flags, h, w, scale, max_h, max_w):
    rng = np.random.default_rng(h * w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    FLAGS.max_h, FLAGS.max_w = max_h, max_w
    crop = P.crop_window(*P.scaled_size(h, w, scale))
    want = _reference_view(img, scale, max_h, max_w)
    d = torch.from_numpy(img).to(cuda)
    plan = ops.view_plan(h, w, scale, crop, 0.25, cuda)
    out = (torch.empty(plan.shape, dtype=torch.float32, device=cuda), torch.empty(plan.quarter_shape, dtype=torch.uint8, device=cuda)) \
        + ops.prepare_workspace(plan, cuda)
    centred, quarter = ops.prepare_view(d, scale, crop, out=out)
    assert np.array_equal(out[2].cpu().numpy(), want)
    if min(want.shape[:2]) >= 2:
        assert np.array_equal(quarter.cpu().numpy(), P.scale_image(want, 0.25))
    else:
        assert quarter.numel() == 0
    assert centred.shape == want.shape


@pytest.mark.parametrize('h,w,numpy_bound', [(480, 896, 1e-3), (128, 160, 5e-5)])
def test_centring_is_center_image(cuda, flags, h, w, numpy_bound):
    """Within 1e-6 of center_image's formula with exact moments (float64), on random images.  numpy's center_image reduces over
    axes (0, 1) with sequential float32 sums: at 480 x 896 its mean is off by ~3e-3 and its output by up to ~2.6e-4 (~1e-5 at 128 x 160),
    which is the difference between the two paths."""
    FLAGS.max_h, FLAGS.max_w = h, w
    rng = np.random.default_rng(w)
    for _ in range(3):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        centred, _ = ops.prepare_view(torch.from_numpy(img).to(cuda), 1.0, (0, 0, h, w))
        got = centred.cpu().numpy()
        x = img.astype(np.float64)
        exact = (x - x.mean((0, 1))) / (x.std((0, 1)) + 1e-8)
        d_exact = np.abs(got - exact).max()
        d_numpy = np.abs(got - P.center_image(img)).max()
        print('%dx%d: max |prepare_view - exact| = %.3g, max |prepare_view - center_image| = %.3g' % (w, h, d_exact, d_numpy))
        assert d_exact <= 1e-6
        assert d_numpy <= numpy_bound


def test_a_constant_channel_centres_to_zero(cuda, flags):
    """sigma = 0: (x - mu) / (0 + 1e-8) is exactly 0 when mu is exact -- here always; in numpy only where its float32 sums are
    exact (128 x 160).  At 480 x 896 numpy's mean is off by float32 rounding and center_image returns ~ +-1."""
    h, w = 128, 160
    img = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[:, :, 1] = 251
    img[:, :, 2] = 129
    centred, _ = ops.prepare_view(torch.from_numpy(img).to(cuda), 1.0, (0, 0, h, w))
    got = centred.cpu().numpy()
    assert (got[:, :, 1:] == 0).all()
    assert np.array_equal(P.center_image(img)[:, :, 1:], got[:, :, 1:])
    big = np.full((480, 896, 3), 251, np.uint8)
    c2, _ = ops.prepare_view(torch.from_numpy(big).to(cuda), 1.0, (0, 0, 480, 896))
    assert (c2.cpu().numpy() == 0).all()


def _scene_images(n, rng, sizes):
    """n synthetic BGR uint8 images (the synthetic scene's texture at each size) and ring cameras."""
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        img = synthetic.make_images(1, h, w, seed=i)[0]
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def _ring(n, k):
    return [[i] + [(i + j) % n for j in range(1, k)] for i in range(n)]


def _cams_for(views, n_views, H, W, D):
    cams = synthetic.make_cams(n_views, H // 4, W // 4, D)
    return np.ascontiguousarray(cams[None][:, :len(views)], dtype=np.float32)


@pytest.mark.parametrize('co_resident', [False, 'cu_split'])
def test_scene_maps_from_cached_towers_are_bitwise(cuda, flags, weights, co_resident, monkeypatch):
    """Every scene-mode map (all four outputs) is torch.equal to GraphedInference(out_prob_map=True) on the stacked prepare_view
    outputs of the same views; two slots.  Images of two sizes: the ring's maps mix them (scale 0.9143, two crop windows per map),
    two more maps hold 150x176 views only (0.9091), so images 1 and 3 are prepared, cached and run through the towers at both scales
    with one captured tower graph (its taps are inputs).  Tower passes are counted as replays of the captured tower graphs (not by
    the scene's own counter): one per (image, scale) over the scene, none in a second pass; one map graph replay per map."""
    FLAGS.max_h, FLAGS.max_w, FLAGS.view_num = 128, 160, 3
    D = 16
    imgs = _scene_images(4, np.random.default_rng(0), [(140, 200), (150, 176)])
    sc = S.SceneInference(lambda i: imgs[i], D, slots=2, co_resident=co_resident, device=cuda, view_num=3)
    maps = [S.pad_views(m, 3) for m in _ring(4, 3) + [[1, 3], [3, 1]]]       # [1, 3, 1], [3, 1, 3]: a missing source
    assert len({sc.layout(m)[0] for m in maps}) == 2
    replays = collections.Counter()
    replay = torch.cuda.CUDAGraph.replay

    def counted(g):
        replays[id(g)] += 1
        return replay(g)
    monkeypatch.setattr(torch.cuda.CUDAGraph, 'replay', counted)
    graphs = {}
    for rnd in range(2):
        replays.clear()
        queue, done = [], []
        for views in maps:
            if not sc.room():
                v, c, t = queue.pop(0)
                done.append((v, c, sc.result(t, host=True), sc.reference_image(t)))
            cams = _cams_for(views, 3, 128, 160, D)
            queue.append((views, cams, sc.submit(views, torch.from_numpy(cams))))
        for v, c, t in queue:
            done.append((v, c, sc.result(t, host=True), sc.reference_image(t)))
        tower_graphs = {id(g.graph) for g in sc.towers.values()}
        tower_replays = sum(n for g, n in replays.items() if g in tower_graphs)
        assert tower_replays == (6 if rnd == 0 else 0), (rnd, tower_replays)     # 4 images + images 1 and 3 at a second scale
        assert sum(n for g, n in replays.items() if g not in tower_graphs) == len(maps)
        assert sc.tower_runs == 6
        torch.cuda.synchronize()
        for v, c, got, q in done:                                 # the references after the scene's maps have all been fetched
            _check_map(cuda, sc, v, c, got, q, D, graphs)


def _check_map(cuda, sc, views, cams, got, q, D, graphs):
    scale, crops = sc.layout(views)
    prepared = torch.stack([ops.prepare_view(torch.from_numpy(sc.loader(v)).to(cuda), scale, c)[0] for v, c in zip(views, crops)], 0)[None]
    dc = torch.from_numpy(cams).to(cuda)
    g = graphs.get('g')
    if g is None:
        g = graphs['g'] = ex.GraphedInference(prepared, dc, D, out_prob_map=True)
    want = [t.cpu() for t in g(prepared, dc)]
    assert len(got) == 4
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert np.array_equal(q, ops.prepare_view(torch.from_numpy(sc.loader(views[0])).to(cuda), scale, crops[0])[1].cpu().numpy())


def test_weight_change_invalidates_the_cache(cuda, flags, weights):
    FLAGS.max_h, FLAGS.max_w, FLAGS.view_num = 128, 160, 3
    imgs = _scene_images(3, np.random.default_rng(0), [(128, 160)])
    sc = S.SceneInference(lambda i: imgs[i], 16, slots=1, device=cuda, view_num=3)
    cams = torch.from_numpy(_cams_for([0, 1, 2], 3, 128, 160, 16))
    sc.result(sc.submit([0, 1, 2], cams))
    assert sc.tower_runs == 3
    store = variables.default_store()
    name = 'conv1_x_1/conv1/weights'
    store.set(name, store.host[name])              # same values, a new generation: nothing computed before may be reused
    try:
        sc.result(sc.submit([0, 1, 2], cams))
        assert sc.tower_runs == 6
    finally:
        ops.clear_pack_cache()


def test_overflow_map_is_the_fp32_map_and_drops_its_entries(cuda, flags, weights):
    """A tower weight x2000: the scene map is bit for bit the split16=False map of the same prepared views, and the entries made
    while the flag was up are gone (the next map recomputes its towers)."""
    FLAGS.max_h, FLAGS.max_w, FLAGS.view_num = 128, 160, 3
    D = 16
    imgs = _scene_images(3, np.random.default_rng(0), [(128, 160)])
    store = variables.default_store()
    names = ['conv1_x_1/conv1/weights', 'conv1_x_1/conv2/weights']
    saved = {n: store.host[n].copy() for n in names}
    try:
        for n in names:
            store.set(n, saved[n] * 2000.0)
        ops.clear_pack_cache()
        sc = S.SceneInference(lambda i: imgs[i], D, slots=2, device=cuda, view_num=3)
        views = [0, 1, 2]
        cams = _cams_for(views, 3, 128, 160, D)
        scale, crops = sc.layout(views)
        prepared = torch.stack([ops.prepare_view(torch.from_numpy(imgs[v]).to(cuda), scale, c)[0] for v, c in zip(views, crops)], 0)[None]
        dc = torch.from_numpy(cams).to(cuda)
        ops.nonfinite_seen(cuda)
        ex.infer_multiview(prepared, dc, D, out_prob_map=True)
        assert ops.nonfinite_seen(cuda), 'the scaled weights no longer overflow the split-operand towers'
        with ops.configure(split16=False):
            want = [t.cpu() for t in ex.infer_multiview(prepared, dc, D, out_prob_map=True)]
        assert not ops.nonfinite_seen(cuda)
        ops.nonfinite_seen(cuda)
        got = sc.result(sc.submit(views, torch.from_numpy(cams)), host=True)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert not any(k for k in sc.cache.items if k[0] != 'image'), 'poisoned entries were kept'
        runs = sc.tower_runs
        got = sc.result(sc.submit(views, torch.from_numpy(cams)), host=True)
        assert sc.tower_runs == runs + 3
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    finally:
        for n in names:
            store.set(n, saved[n])
        ops.clear_pack_cache()


# pair.txt of the driver test: maps 0 and 3 mix the two image sizes (scale max(128/140, 160/176) = 0.9143), map 1 holds 150x176 views
# only (0.9091), map 2 140x200 views only (0.9143): images 1 and 3 are prepared and cached at both scales.  Maps 1 and 2 have one
# source: the missing view is the reference.
_PAIRS = [(0, [1, 2]), (1, [3]), (2, [0]), (3, [1, 0])]
_SIZES = [(140, 200), (150, 176), (140, 200), (150, 176)]


def _write_scene_dir(root, rng):
    """ETH3D-style scene: 4 images of two sizes, both above max_h x max_w, with the maps of _PAIRS."""
    from PIL import Image
    scene = os.path.join(root, 'eth3d', 'toy')
    os.makedirs(os.path.join(scene, 'images'))
    os.makedirs(os.path.join(scene, 'cams'))
    for v, (h, w) in enumerate(_SIZES):
        img = np.clip(synthetic.make_images(1, h, w, seed=v)[0], 0, 255).astype(np.uint8)
        Image.fromarray(img[:, :, ::-1]).save(os.path.join(scene, 'images', '%08d.jpg' % v), quality=95)
        cam = synthetic.make_cams(4, h, w, 16)[v].astype(np.float64).copy()
        cam[1, :2, :3] *= 4                       # full-resolution intrinsics; a metric depth range
        cam[1, 3] = (2.0, 0.05, 16, 0.0)
        P.write_cam(os.path.join(scene, 'cams', '%08d_cam.txt' % v), cam)
    with open(os.path.join(scene, 'pair.txt'), 'w') as f:
        f.write('%d\n' % len(_PAIRS) + ''.join('%d\n%d %s\n' % (r, len(src), ' '.join('%d 1.0' % v for v in src)) for r, src in _PAIRS))
    return scene


@pytest.mark.parametrize('mode', ['serial', 'cu_split'])
def test_driver_scene_cache_end_to_end(cuda, tmp_path, weights, mode):
    """--scene_cache writes the default driver's file set; .jpg / .txt byte-identical; the writer thread's files byte-identical to a
    synchronous write.  The centred inputs differ from center_image's in the last bits (exact moments here, float32 sums in numpy), and
    the network amplifies that.  Measured per map: depth 1.8e-6 ... 4.0e-4 relative on average, 8.4e-5 ... 3.8e-2 at the worst pixel;
    probabilities 7.9e-4 ... 1.2e-2 absolute on average (where the estimate moves across a depth bin the probability around it changes
    by up to 1).  The bounds sit about 1.5x above those.  That the maps are otherwise the same computation is
    test_scene_maps_from_cached_towers_are_bitwise's claim (bit for bit on the same prepared views, two sizes, two scales)."""
    root = str(tmp_path)
    _write_scene_dir(root, np.random.default_rng(0))
    FLAGS.reset()
    FLAGS.max_h, FLAGS.max_w = 128, 160
    scales = {}
    for r, src in _PAIRS:
        views = S.pad_views([r] + src, 3)
        for v in views:
            scales.setdefault(v, set()).add(S.adaptive_scale([_SIZES[u] for u in views]))
    FLAGS.reset()
    assert len(scales[1]) == 2 and len(scales[3]) == 2          # the same image at two adaptive scales
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy', '--maps_in_flight', mode]
    runs = {'default': [], 'scene': ['--scene_cache'], 'sync': ['--scene_cache', '--sync_write']}
    files = {}
    try:
        for name, extra in runs.items():
            FLAGS.reset()
            out = os.path.join(root, 'out_' + name)
            E.cli(base + ['--savepath', out] + extra)
            d = os.path.join(out, 'toy', 'depths_atvsnet')
            files[name] = {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    assert set(files['scene']) == set(files['default']) and len(files['default']) == 20
    assert files['scene'] == files['sync']
    for f, data in files['default'].items():
        if f.endswith('.jpg') or f.endswith('.txt'):
            assert files['scene'][f] == data, f
        elif f.endswith('.pfm'):
            import io
            a, b = P.load_pfm(io.BytesIO(data)), P.load_pfm(io.BytesIO(files['scene'][f]))
            # the centred inputs differ from center_image's in the last bits (exact moments here, float32 sums in numpy): the maps
            # agree to 1e-5 relative on average; isolated pixels move more (the refinement's discontinuous steps)
            if f.endswith('_prob.pfm'):                    # probabilities in [0, 1]: near-zero ones have no meaningful relative error
                err = np.abs(a - b)
                print('%s: absolute difference mean %.2e, max %.2e' % (f, err.mean(), err.max()))
                assert err.mean() <= 2e-2, f
            else:
                rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-12)
                print('%s: relative difference mean %.2e, max %.2e' % (f, rel.mean(), rel.max()))
                assert rel.mean() <= 6e-4 and rel.max() <= 6e-2, f
