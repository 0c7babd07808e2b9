"""-m gpu: the in-run scene fusion (csrc/fusion_scene.hip, depth_fusion.SceneFusion, eval_pointcloud --fuse).

The staging kernel bit for bit against numpy restating _write_map -> probability_filter -> fake_colmap_normal; the whole-scene
fusion bit for bit against the per-camera path (fuse_views) and the oracle; the driver's PLY against the two-step file pipeline in
the default mode and in scene mode (serial and cu_split); the fp32 range rule: an overflowed map is staged from its fp32 rerun."""
import io
import os

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
import fusion_cases as FC
import numerics
from atvsnet_amd import FLAGS, ops, synthetic, variables
from atvsnet_amd.atvsnet import depth_fusion as DF
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import example as ex
from atvsnet_amd.atvsnet import preprocess as P
from atvsnet_amd.atvsnet import scene as S
from atvsnet_amd.tools import ply

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ staging

def _stage_numpy(depth, prob, bgr, inverse_depth, thr):
    """_write_map's inverse-depth step, probability_filter and fake_colmap_normal, as the file pipeline runs them."""
    d = depth.copy()
    if inverse_depth:
        d[d <= 0] = float('inf')
        d = 1.0 / d
    d = np.array(d, np.float32)
    d[prob < thr] = 0
    normal = np.ones(d.shape + (3,), np.float32) / 1.732050808
    mask = (d > 0).astype(np.float32)[..., None]
    nd = np.concatenate([np.float32(normal * mask), d[..., None]], -1)
    img = np.concatenate([bgr.astype(np.float32), np.zeros(bgr.shape[:2] + (1,), np.float32)], -1)
    return nd, img


@pytest.mark.parametrize('inverse_depth', [True, False])
def test_stage_kernel_is_the_file_pipeline(cuda, inverse_depth):
    rng = np.random.default_rng(3)
    rows, cols, thr = 37, 53, 0.8
    depth = rng.uniform(-0.5, 3.0, (rows, cols)).astype(np.float32)
    flat = depth.reshape(-1)
    flat[:8] = [0.0, -0.0, -1e-30, 1e-39, 1e-45, 2e-39, 3e38, np.float32(1.0) / np.float32(3.0)]   # <= 0, tiny (-> inf), huge
    prob = rng.uniform(0, 1, (rows, cols)).astype(np.float32)
    prob.reshape(-1)[::7] = np.float32(thr)                      # exactly at the threshold: kept
    prob.reshape(-1)[3::11] = np.nextafter(np.float32(thr), np.float32(0))
    prob.reshape(-1)[:8] = 1.0                                   # the special depths are not filtered away
    bgr = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
    want_nd, want_img = _stage_numpy(depth, prob, bgr, inverse_depth, thr)
    nd = torch.full((2, rows, cols, 4), float('nan'), device=cuda)
    img = torch.full((2, rows, cols, 4), float('nan'), device=cuda)
    up = lambda a: torch.from_numpy(a).to(cuda)                  # noqa: E731
    ops.fusion_stage(up(depth), up(prob), up(bgr), inverse_depth, thr, nd[1], img[1])
    got_nd, got_img = nd[1].cpu().numpy(), img[1].cpu().numpy()
    assert got_nd.tobytes() == want_nd.tobytes()
    assert got_img.tobytes() == want_img.tobytes()
    assert torch.isnan(nd[0]).all() and torch.isnan(img[0]).all()      # the other slot is untouched
    if inverse_depth:
        assert np.isinf(want_nd[..., 3]).any() and (want_nd[..., 3] == 0).any()
    assert ((prob == np.float32(thr)) & (want_nd[..., 3] != 0)).any()


# ------------------------------------------------------------------------------------------------------------- scene fusion

def _scene(n, rows, cols, step_deg=3.0, baseline=0.4, seed=0, noise=0.004):
    """A tilted plane seen by n pinhole cameras (tests/fusion_scene.py's construction), camera 0 at the origin looking down +z,
    K with power-of-two focal length and principal point: the pixel column x = 32 of camera 0 back-projects to X = 0 exactly."""
    rng = np.random.default_rng(seed)
    K = np.array([[64.0, 0, 32.0], [0, 64.0, 16.0], [0, 0, 1]])
    nrm = np.array([0.1, -0.05, -1.0])
    nrm /= np.linalg.norm(nrm)
    d0 = 5.0
    ys, xs = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    Ps, depths, normals, images = [], [], [], []
    for i in range(n):
        ang = np.deg2rad(step_deg * i)
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        C = np.array([baseline * i, 0.1 * baseline * i, 0.0])
        Ps.append(K @ np.concatenate([R, (-R @ C)[:, None]], 1))
        rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T @ R
        s = -(nrm @ C + d0) / (rays @ nrm)
        depths.append(s.astype(np.float32))
        normals.append(np.broadcast_to((R @ nrm).astype(np.float32), (rows, cols, 3)).copy())
        X = C + s[..., None] * rays
        img = 127.0 + 100.0 * np.stack([np.sin(X[..., 0] * 2.0), np.cos(X[..., 1] * 3.0), np.sin(X[..., 0] + X[..., 1])], -1)
        images.append(np.clip(img + rng.uniform(0, 4, img.shape), 0, 255).astype(np.uint8))
    depths = np.stack(depths)
    depths = depths * (1.0 + noise * rng.normal(size=depths.shape)).astype(np.float32)       # some views disagree
    depths[:, 3:9, 10:20] = 0                                                                  # filtered pixels
    return np.stack(Ps), depths, np.stack(normals), np.stack(images)


def _textures(depths, normals, images):
    nd = np.ascontiguousarray(np.concatenate([normals, depths[..., None]], -1).astype(np.float32))
    img4 = np.ascontiguousarray(np.concatenate([images.astype(np.float32), np.zeros(images.shape[:3] + (1,), np.float32)], -1))
    return nd, img4


def _scene_fuse(cuda, Ps, nd, img4, disp, nthr, ncons):
    cams = torch.from_numpy(DF.pack_cameras(Ps)).to(cuda)
    pts, cols = ops.fusibile_scene(cams, torch.from_numpy(nd).to(cuda), torch.from_numpy(img4).to(cuda), disp, nthr, ncons)
    return pts.cpu().numpy(), cols.cpu().numpy()


@pytest.mark.parametrize('n,rows,cols,ncons', [(2, 48, 64, 1), (3, 37, 53, 2), (5, 41, 45, 2), (9, 33, 70, 3)])
def test_scene_fusion_is_fuse_views(cuda, n, rows, cols, ncons):
    Ps, depths, normals, images = _scene(n, rows, cols, seed=n)
    nd, img4 = _textures(depths, normals, images)
    disp, nthr = 0.01, DF.NORMAL_THRESHOLD
    got_p, got_c = _scene_fuse(cuda, Ps, nd, img4, disp, nthr, ncons)
    want_p, want_c = DF.fuse_views(Ps, depths, normals, images, disp, nthr, ncons, device=cuda)
    assert 0 < len(want_p) < n * rows * cols                     # the case decides something
    assert got_p.shape == want_p.shape and got_p.tobytes() == want_p.tobytes()
    assert got_c.tobytes() == want_c.tobytes()
    from oracle import fusibile as F
    ora_p, ora_c = F.fuse(Ps, depths, normals, images, disp, nthr, ncons)
    assert got_p.tobytes() == ora_p.tobytes() and got_c.tobytes() == ora_c.tobytes()


def _nan_canonical(a):
    """The bytes of a float array with every NaN replaced by one NaN.  Only the sign and payload of a NaN are forgiven (which
    NaN an invalid operation returns is the platform's choice: x86 sets the sign bit of a default NaN, the GPU does not); where
    the NaNs are, and every other value, the sign of a zero included, is compared bit for bit.  For the comparison with the CPU
    oracle only: the two device paths are compared on their raw bytes."""
    return np.where(np.isnan(a), np.float32(np.nan), a).tobytes()


@pytest.mark.parametrize('case', FC.SCENE_CASES, ids=FC.case_id)
def test_scene_fusion_general_cases(cuda, case):
    """general_scene with full cameras, occlusion and (where the case says so) hard_maps' special values: the whole-scene kernel
    equals the per-camera path byte for byte, and both equal the oracle.  num_consistent = 0 keeps the NaN points and the points
    at a camera centre (the host filter is != 0, reference fusibile.cu:309)."""
    from oracle import fusibile as F
    assert (case.rows, case.cols) in FC.FUSION_SHAPES['scene'], 'shape is not listed in fusion_cases.FUSION_SHAPES'
    Ps, depths, normals, images, _ = FC.case_inputs(case)
    nd, img4 = FC.textures(depths, normals, images)
    disp, nthr = case.thresholds
    dev = [numerics.nan_bordered(torch.from_numpy(a).to(cuda)) for a in (DF.pack_cameras(Ps), nd, img4)]
    numerics.poison_allocator(cuda)
    pts, cols = ops.fusibile_scene(dev[0], dev[1], dev[2], disp, nthr, case.ncons)
    got_p, got_c = pts.cpu().numpy(), cols.cpu().numpy()
    want_p, want_c = DF.fuse_views(Ps, depths, normals, images, disp, nthr, case.ncons, device=cuda)
    if 0 < case.ncons < case.n:
        assert 0 < len(want_p) < case.n * case.rows * case.cols             # the case decides something
    elif case.ncons >= case.n:
        assert len(want_p) == 0                                              # there are only n - 1 other views: an empty cloud
    assert got_p.shape == want_p.shape and got_p.tobytes() == want_p.tobytes()
    assert got_c.tobytes() == want_c.tobytes()
    ora_p, ora_c = F.fuse(Ps, depths, normals, images, disp, nthr, case.ncons)
    assert got_p.shape == ora_p.shape and _nan_canonical(got_p) == _nan_canonical(ora_p)
    assert got_c.tobytes() == ora_c.tobytes()
    if case.ncons == 0:
        assert np.isnan(got_p).any(-1).sum() > 0                 # NaN points are kept
        assert len(got_p) > 0.99 * case.n * case.rows * case.cols


def test_created_point_with_a_zero_coordinate_is_dropped(cuda):
    Ps, depths, normals, images = _scene(3, 37, 53, noise=0.0)
    nd, img4 = _textures(depths, normals, images)
    cams = torch.from_numpy(DF.pack_cameras(Ps)).to(cuda)
    ndd, imd = torch.from_numpy(nd).to(cuda), torch.from_numpy(img4).to(cuda)
    coord, _, _, created = [t.cpu().numpy() for t in ops.fusibile(cams, ndd, imd, 0, 0.01, DF.NORMAL_THRESHOLD, 1)]
    zero = (created > 0) & (coord[..., :3] == 0).any(-1)
    assert zero.any(), 'the case no longer has a created point with a zero coordinate'
    got_p, got_c = _scene_fuse(cuda, Ps, nd, img4, 0.01, DF.NORMAL_THRESHOLD, 1)
    want_p, want_c = DF.fuse_views(Ps, depths, normals, images, 0.01, DF.NORMAL_THRESHOLD, 1, device=cuda)
    assert got_p.tobytes() == want_p.tobytes() and got_c.tobytes() == want_c.tobytes()
    assert (got_p != 0).all()


def test_scene_fusion_many_views(cuda):
    """300 views of 30x40: 1500 workgroups, so the scan runs over two chunks of 1024 counts."""
    n, rows, cols = 300, 30, 40
    Ps, depths, normals, images = _scene(n, rows, cols, step_deg=0.02, baseline=0.004, seed=1)
    nd, img4 = _textures(depths, normals, images)
    got_p, got_c = _scene_fuse(cuda, Ps, nd, img4, 0.01, DF.NORMAL_THRESHOLD, 2)
    want_p, want_c = DF.fuse_views(Ps, depths, normals, images, 0.01, DF.NORMAL_THRESHOLD, 2, device=cuda)
    assert 0 < len(want_p) < n * rows * cols
    assert got_p.tobytes() == want_p.tobytes() and got_c.tobytes() == want_c.tobytes()


def test_scene_fusion_object_orders_by_out_index(cuda):
    """SceneFusion.add in shuffled order, raw network-style maps (inverse depth) -> fuse_views of the staged maps in out_index
    order."""
    n, rows, cols = 5, 37, 53
    Ps, depths, normals, images = _scene(n, rows, cols, seed=11)
    rng = np.random.default_rng(5)
    inv = (1.0 / depths).astype(np.float32)                      # what the network returns with FLAGS.inverse_depth
    inv[depths == 0] = 0
    prob = rng.uniform(0.5, 1, depths.shape).astype(np.float32)
    cams = []
    for P_ in Ps:                                                # write_cam's camera whose projection_matrix is P_
        cam = np.zeros((2, 4, 4))
        cam[0] = np.eye(4)
        cam[0, :3, :] = P_
        cam[1, :3, :3] = np.eye(3)
        cam[1, 3] = (2.0, 0.05, 16, 2.8)
        cams.append(cam)
    ids = [40, 7, 19, 3, 25]
    f = DF.SceneFusion(n, rows, cols, cuda, prob_threshold=0.8, disp_threshold=0.01, num_consistent=2, inverse_depth=True)
    for k in rng.permutation(n):
        f.add(ids[k], inv[k][None, ..., None], prob[k][None, ..., None], images[k], cams[k])
    got_p, got_c = f.run()
    order = np.argsort(ids)
    staged = [_stage_numpy(inv[k], prob[k], images[k], True, 0.8)[0] for k in order]
    Ps_f = [DF.projection_matrix(P.load_cam(io.StringIO(P.cam_text(cams[k])))) for k in order]
    want_p, want_c = DF.fuse_views(Ps_f, np.stack([s[..., 3] for s in staged]), np.stack([s[..., :3] for s in staged]),
                                   images[order], 0.01, DF.NORMAL_THRESHOLD, 2, device=cuda)
    assert 0 < len(want_p)
    assert got_p.tobytes() == want_p.tobytes() and got_c.tobytes() == want_c.tobytes()


# ---------------------------------------------------------------------------------------------------------- driver, end to end

_N_IMAGES, _H, _W = 5, 140, 200


def _write_scene_dir(root):
    """ETH3D-style scene: 5 images of one size above max_h x max_w, ring pair.txt with two sources each."""
    from PIL import Image
    scene = os.path.join(root, 'eth3d', 'toy')
    os.makedirs(os.path.join(scene, 'images'))
    os.makedirs(os.path.join(scene, 'cams'))
    cams = synthetic.make_cams(_N_IMAGES, _H, _W, 16)
    for v in range(_N_IMAGES):
        img = np.clip(synthetic.make_images(1, _H, _W, seed=v)[0], 0, 255).astype(np.uint8)
        Image.fromarray(img[:, :, ::-1]).save(os.path.join(scene, 'images', '%08d.jpg' % v), quality=95)
        cam = cams[v].astype(np.float64).copy()
        cam[1, :2, :3] *= 4
        cam[1, 3] = (2.0, 0.05, 16, 0.0)
        P.write_cam(os.path.join(scene, 'cams', '%08d_cam.txt' % v), cam)
    with open(os.path.join(scene, 'pair.txt'), 'w') as f:
        f.write('%d\n' % _N_IMAGES)
        for v in range(_N_IMAGES):
            f.write('%d\n2 %d 1.0 %d 1.0\n' % (v, (v + 1) % _N_IMAGES, (v + 2) % _N_IMAGES))
    return scene


def _files(d):
    return {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize('mode', ['default', 'serial', 'cu_split'])
def test_driver_fuse_is_the_two_step_pipeline(cuda, tmp_path, weights, mode):
    root = str(tmp_path)
    scene = _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy']
    if mode != 'default':
        base += ['--scene_cache', '--maps_in_flight', mode]
    fuse_args = ['--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1']
    runs = {'plain': [], 'fuse': ['--fuse'] + fuse_args, 'nofiles': ['--fuse', '--no_map_files'] + fuse_args}
    out = {}
    try:
        for name, extra in runs.items():
            FLAGS.reset()
            out[name] = os.path.join(root, 'out_' + name, 'toy')
            E.cli(base + ['--savepath', os.path.dirname(out[name])] + extra)
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    maps = lambda n: _files(os.path.join(out[n], 'depths_atvsnet'))        # noqa: E731
    plain = maps('plain')
    assert len(plain) == 5 * _N_IMAGES
    assert not os.path.exists(os.path.join(out['plain'], 'final3d_model.ply'))
    assert maps('fuse') == plain                                 # --fuse changes none of the map files
    assert maps('nofiles') == {}
    assert os.path.exists(os.path.join(out['nofiles'], 'zz_runtime.txt'))
    with open(os.path.join(out['fuse'], 'final3d_model.ply'), 'rb') as f:
        fused_bytes = f.read()
    with open(os.path.join(out['nofiles'], 'final3d_model.ply'), 'rb') as f:
        assert f.read() == fused_bytes
    # the two-step pipeline on the plain run's files
    DF.main(['--dense_folder', out['plain'], '--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1'])
    want_p, _ = ply.read_ply(os.path.join(out['plain'], 'final3d_model.ply'))
    got_p, got_c = ply.read_ply(os.path.join(out['fuse'], 'final3d_model.ply'))
    assert len(got_p) > 0
    assert len(got_p) == len(want_p) and got_p.tobytes() == want_p.tobytes()
    # colours: the file pipeline colours from the re-decoded JPEG; the in-run path from the exact 1/4 images load_data gives
    pf = os.path.join(out['plain'], 'points_atvsnet')
    names = ['%08d' % i for i in range(_N_IMAGES)]
    Ps = [DF.read_p_file(os.path.join(pf, 'cams', s + '.jpg.P')) for s in names]
    depths = np.stack([DF.read_gipuma_dmb(os.path.join(pf, '2333__' + s, 'disp.dmb')) for s in names])
    normals = np.stack([DF.read_gipuma_dmb(os.path.join(pf, '2333__' + s, 'normals.dmb')) for s in names])
    FLAGS.reset()
    try:
        FLAGS.view_num, FLAGS.max_d, FLAGS.max_h, FLAGS.max_w = 3, 16, 128, 160
        mvs = E.gen_data_list(scene)
        quarters = {}
        for i in range(len(mvs)):
            raw, _, _, _, idx = E.load_data(mvs, i)
            quarters[idx] = raw[0, 0]
    finally:
        FLAGS.reset()
    images = np.stack([quarters[i] for i in range(_N_IMAGES)])
    ref_p, ref_c = DF.fuse_views(Ps, depths, normals, images, 0.5, DF.NORMAL_THRESHOLD, 1, device=cuda)
    assert ref_p.tobytes() == got_p.tobytes() and ref_c.tobytes() == got_c.tobytes()


# ------------------------------------------------------------------------------------------------------------ fp32 range rule

def test_overflow_map_is_staged_from_its_fp32_rerun(cuda, weights):
    """A tower weight x2000 (as test_gpu_scene's overflow test): the slab row staged from result() equals the one staged from the
    split16=False outputs of the same prepared views, not from the overflowed replay's buffers."""
    FLAGS.reset()
    FLAGS.max_h, FLAGS.max_w, FLAGS.view_num = 128, 160, 3
    D = 16
    imgs = [np.clip(synthetic.make_images(1, 128, 160, seed=i)[0], 0, 255).astype(np.uint8) for i in range(3)]
    store = variables.default_store()
    names = ['conv1_x_1/conv1/weights', 'conv1_x_1/conv2/weights']
    saved = {n: store.host[n].copy() for n in names}
    try:
        for n in names:
            store.set(n, saved[n] * 2000.0)
        ops.clear_pack_cache()
        sc = S.SceneInference(lambda i: imgs[i], D, slots=2, device=cuda, view_num=3)
        views = [0, 1, 2]
        cams = np.ascontiguousarray(synthetic.make_cams(3, 32, 40, D)[None], dtype=np.float32)
        scale, crops = sc.layout(views)
        prepared = torch.stack([ops.prepare_view(torch.from_numpy(imgs[v]).to(cuda), scale, c)[0] for v, c in zip(views, crops)], 0)[None]
        dc = torch.from_numpy(cams).to(cuda)
        with ops.configure(split16=False):
            want = ex.infer_multiview(prepared, dc, D, out_prob_map=True)
        ops.nonfinite_seen(cuda)
        t = sc.submit(views, torch.from_numpy(cams))
        out = sc.result(t)
        quarter = sc.reference_image(t, host=False)
        rows, cols = quarter.shape[:2]
        got = DF.SceneFusion(1, rows, cols, cuda, prob_threshold=0.3)
        got.add(0, out[0], out[2], quarter, cams[0, 0], stream=sc.slot_stream(t))
        ref = DF.SceneFusion(1, rows, cols, cuda, prob_threshold=0.3)
        ref.add(0, want[0], want[2], quarter, cams[0, 0])
        torch.cuda.synchronize()
        assert torch.equal(got.nd, ref.nd) and torch.equal(got.img, ref.img)
        replay = sc.pipelines[(3, crops[0][2], crops[0][3])].graphs[t[1]].out
        assert not torch.equal(replay[0], want[0]), 'the replay buffers hold the fp32 map: the case does not bite'
    finally:
        for n in names:
            store.set(n, saved[n])
        ops.clear_pack_cache()
        FLAGS.reset()
