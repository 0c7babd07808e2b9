"""-m gpu: normals from depth maps (csrc/depth_normals.hip) and the fusion that tests and returns them.

The kernel against the float64 restatement (tests/depth_normals_restated.py) within one float32 rounding; the fusion with the
kernel's normals bit for bit against the oracle (oracle/fusibile.py), for the scene kernel and the per-camera path; the effect on
the sawtooth scene; the driver's PLY against the two-step file pipeline, normals included."""
import os

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
import depth_normals_restated as R
import numerics
from atvsnet_amd import FLAGS, ops, synthetic
from atvsnet_amd.atvsnet import depth_fusion as DF
from atvsnet_amd.atvsnet import eval_pointcloud as E
from atvsnet_amd.atvsnet import preprocess as P
from atvsnet_amd.tools import ply

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------- kernel

def _maps(kind):
    """-> (projection matrices, depths (N,rows,cols) float32)"""
    if kind == 'plane':
        return R.plane_scene()[0], R.plane_scene()[1]
    if kind == 'sawtooth':
        return R.plane_scene()[0], R.sawtooth_depths()
    n, rows, cols = {'planted_37x53': (3, 37, 53), 'planted_5x7': (1, 5, 7), 'planted_48x64': (4, 48, 64)}[kind]
    return R.cameras(n, rows, cols), R.planted_depths(n, rows, cols, seed=n)


def _kernel_normals(cuda, cams, depths, step, gate):
    """The kernel on a slab whose normal floats start as NaN -> (normals (N,rows,cols,3), depth plane after the launch)."""
    nd = np.full(depths.shape + (4,), np.nan, np.float32)
    nd[..., 3] = depths
    slab = numerics.nan_bordered(torch.from_numpy(nd).to(cuda))
    out = ops.depth_normals(numerics.nan_bordered(torch.from_numpy(cams).to(cuda)), slab, step, gate)
    assert out is slab
    got = slab.cpu().numpy()
    return got[..., :3], got[..., 3]


@pytest.mark.parametrize('step', [1, 2])
@pytest.mark.parametrize('kind,gate', [('plane', 0.02), ('sawtooth', 0.05), ('planted_48x64', 0.02), ('planted_37x53', 0.02),
                                       ('planted_37x53', 0.05), ('planted_5x7', 0.02)])
def test_kernel_is_the_restatement(cuda, kind, gate, step):
    """Both sides evaluate one float64 expression from the same float32 inputs; what cancellation leaves (about 1e-11) can only
    show where the final rounding to float32 straddles a boundary: one ulp of a value <= 1, 2^-23 absolute.  The zero pattern
    (no depth, no usable quadrant) is exact, and the depth plane keeps its bits."""
    Ps, depths = _maps(kind)
    cams = DF.pack_cameras(Ps)
    want = R.depth_normals(cams, depths, step, gate)
    got, w_after = _kernel_normals(cuda, cams, depths, step, gate)
    assert w_after.tobytes() == np.ascontiguousarray(depths).tobytes()
    assert np.isfinite(got).all()                                             # every normal float was written
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print('%s step %d gate %g: largest component difference %.3e' % (kind, step, gate, err))
    assert np.array_equal((got == 0).all(-1), (want == 0).all(-1))
    assert (got[~(depths > 0)] == 0).all()
    assert err <= 2.0 ** -23
    if kind.startswith('planted'):
        assert ((want == 0).all(-1) & (depths > 0)).any()                     # a pixel with depth and no usable quadrant
    length = np.linalg.norm(got.astype(np.float64), axis=-1)
    assert np.abs(length[(got != 0).any(-1)] - 1.0).max() < 1e-6


# ------------------------------------------------------------------------------------------------------------------- fusion

def _oracle_fuse(cams, nd, img4, disp, nthr, ncons):
    """oracle.fusibile.fuse with packed cameras, keeping the averaged normals and each reference's created mask."""
    from oracle import fusibile as F
    pts, cols, nrms, created_masks = [], [], [], []
    for ref in range(len(cams)):
        X, cn, tex, created = F.fuse_reference(cams, nd, img4, ref, disp, nthr, ncons)
        keep = created & (X[..., 0] != 0) & (X[..., 1] != 0) & (X[..., 2] != 0)
        pts.append(X[keep])
        nrms.append(cn[keep])
        t = tex[keep]
        cols.append(np.stack([t[:, 2], t[:, 1], t[:, 0]], -1).astype(np.int32).astype(np.uint8))
        created_masks.append(keep)
    return np.concatenate(pts, 0), np.concatenate(cols, 0), np.concatenate(nrms, 0), np.stack(created_masks)


def _img4(images):
    return np.ascontiguousarray(np.concatenate([images.astype(np.float32), np.zeros(images.shape[:3] + (1,), np.float32)], -1))


@pytest.mark.parametrize('kind,disp,deg', [('sawtooth', 0.01, 30.0), ('sawtooth', 0.05, 30.0), ('plane', 0.01, 360.0)])
def test_fusion_with_kernel_normals_is_the_oracle(cuda, kind, disp, deg):
    Ps, depths = _maps(kind)
    images = R.plane_scene()[3]
    cams = DF.pack_cameras(Ps)
    normals, _ = _kernel_normals(cuda, cams, depths, 1, 0.05)
    nd = np.ascontiguousarray(np.concatenate([normals, depths[..., None]], -1))
    img4 = _img4(images)
    nthr = DF.normal_threshold_radians(deg)
    want_p, want_c, want_n, _ = _oracle_fuse(cams, nd, img4, disp, nthr, 2)
    assert 0 < len(want_p) < depths.size
    dev = [torch.from_numpy(a).to(cuda) for a in (cams, nd, img4)]
    numerics.poison_allocator(cuda)
    got = [t.cpu().numpy() for t in ops.fusibile_scene(dev[0], dev[1], dev[2], disp, nthr, 2, with_normals=True)]
    assert got[0].shape == want_p.shape and got[0].tobytes() == want_p.tobytes()
    assert got[1].tobytes() == want_c.tobytes()
    assert got[2].shape == want_n.shape and got[2].tobytes() == want_n.tobytes()
    plain = [t.cpu().numpy() for t in ops.fusibile_scene(dev[0], dev[1], dev[2], disp, nthr, 2)]
    assert len(plain) == 2 and plain[0].tobytes() == got[0].tobytes() and plain[1].tobytes() == got[1].tobytes()
    views = DF.fuse_views(Ps, depths, normals, images, disp, nthr, 2, device=cuda, return_normals=True)
    assert views[0].tobytes() == want_p.tobytes() and views[1].tobytes() == want_c.tobytes() and views[2].tobytes() == want_n.tobytes()
    two = DF.fuse_views(Ps, depths, normals, images, disp, nthr, 2, device=cuda)
    assert len(two) == 2 and two[0].tobytes() == want_p.tobytes()


# ------------------------------------------------------------------------------------------------------------------- effect

def _write_cam_of(P_):
    """write_cam's (2,4,4) camera whose projection_matrix is P_."""
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[0, :3, :] = P_
    cam[1, :3, :3] = np.eye(3)
    cam[1, 3] = (2.0, 0.05, 16, 2.8)
    return cam


def _scene_fusion(cuda, Ps, depths, images, **options):
    n, rows, cols = depths.shape
    f = DF.SceneFusion(n, rows, cols, cuda, prob_threshold=0.5, disp_threshold=0.01, num_consistent=2, inverse_depth=False, **options)
    for k in range(n):
        f.add(k, np.ascontiguousarray(depths[k]), np.ones((rows, cols), np.float32), images[k], _write_cam_of(Ps[k]))
    return f


def test_depth_normals_remove_the_sawtooth_patch(cuda):
    """View 1's patch of 45 degree facets agrees with the other views in disparity at half of its pixels; its normals agree
    nowhere.  The CPU oracle gives 128 reference-1 points in the patch with fake normals, 0 with depth normals at 30 degrees."""
    Ps, _, _, images = R.plane_scene()[:4]
    depths = R.sawtooth_depths()
    img4 = _img4(images)
    results = {}
    for source in ('fake', 'depth'):
        f = _scene_fusion(cuda, Ps, depths, images, normals=source, normal_depth_gate=0.05,
                          normal_threshold=30.0 if source == 'depth' else None)
        pts, cols = f.run()
        assert f.nd[..., 3].cpu().numpy().tobytes() == np.ascontiguousarray(depths).tobytes()        # the depth planes are kept
        nd = f.nd.cpu().numpy()                                      # the normals the fusion read: fake, or the kernel's
        nthr = DF.normal_threshold_radians(f.normal_threshold)
        want_p, want_c, want_n, masks = _oracle_fuse(f.cams, nd, img4, 0.01, nthr, 2)
        # point for point the oracle's cloud: the two created masks differ exactly where the oracle with these normals says so
        assert pts.shape == want_p.shape and pts.tobytes() == want_p.tobytes() and cols.tobytes() == want_c.tobytes()
        if source == 'depth':
            assert f.normals().tobytes() == DF.unit_normals(want_n).tobytes()
            restated = R.depth_normals(f.cams, depths, 1, 0.05)
            assert np.abs(nd[..., :3].astype(np.float64) - restated).max() <= 2.0 ** -23
        results[source] = masks[1]
    in_patch = {k: int(m[R.PATCH].sum()) for k, m in results.items()}
    print('reference-1 points inside the patch:', in_patch)
    assert in_patch['fake'] >= 1
    assert in_patch['depth'] == 0
    outside = np.ones(results['fake'].shape, bool)
    outside[R.PATCH] = False
    assert (results['depth'] & outside).sum() > 0.5 * (results['fake'] & outside).sum()          # the plane around it stays


def test_depth_normals_at_360_degrees_are_the_fake_cloud(cuda, tmp_path):
    Ps, depths, _, images = R.plane_scene()[:4]
    fake = _scene_fusion(cuda, Ps, depths, images)
    real = _scene_fusion(cuda, Ps, depths, images, normals='depth', normal_threshold=360)
    fp, fc = fake.run()
    rp, rc = real.run()
    assert len(fp) > 0 and fp.tobytes() == rp.tobytes() and fc.tobytes() == rc.tobytes()
    # without the option the PLY is the six-property file, with it the normals ride along
    a, b = str(tmp_path / 'fake.ply'), str(tmp_path / 'real.ply')
    fake.write_ply(a)
    real.write_ply(b)
    plain = str(tmp_path / 'plain.ply')
    ply.write_ply(plain, fp, fc)
    with open(a, 'rb') as fa, open(plain, 'rb') as fb:
        assert fa.read() == fb.read()
    got_p, got_c, got_n = ply.read_ply_normals(b)
    assert got_p.tobytes() == fp.tobytes() and got_c.tobytes() == fc.tobytes() and got_n.tobytes() == real.normals().tobytes()
    length = np.linalg.norm(got_n.astype(np.float64), axis=-1)
    assert (np.abs(length - 1.0) <= 2.0 ** -23).all()               # a plane: every point has a normal
    with pytest.raises(RuntimeError):
        fake.normals()


# ---------------------------------------------------------------------------------------------------------------- pipelines

_N_IMAGES, _H, _W = 5, 140, 200


def _write_scene_dir(root):
    """ETH3D-style scene (tests/test_gpu_fusion_scene.py's): 5 images, ring pair.txt with two sources each."""
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


def test_driver_and_two_step_pipeline_write_the_same_normals(cuda, tmp_path, weights):
    """eval_pointcloud --fuse --fuse_normals depth against depth_fusion --normals depth on the files of a plain run: the same
    points and normals byte for byte.  The colours are compared as tests/test_gpu_fusion_scene.py compares them: the file pipeline
    colours from the re-decoded JPEG, the in-run path from the exact 1/4 images, so the in-run colours are those of fuse_views on
    the file pipeline's maps and normals with the in-run images."""
    root = str(tmp_path)
    scene = _write_scene_dir(root)
    base = ['--data_root', root, '--view_num', '3', '--max_d', '16', '--max_w', '160', '--max_h', '128', '--synthetic_weights',
            '--scenes', 'toy']
    fuse_args = ['--prob_threshold', '0.5', '--disp_threshold', '0.5', '--num_consistent', '1']
    runs = {'plain': [], 'normals': ['--fuse', '--no_map_files'] + fuse_args + [
        '--fuse_normals', 'depth', '--fuse_normal_threshold', '80', '--fuse_normal_step', '2', '--fuse_normal_depth_gate', '0.5']}
    out = {}
    try:
        for name, extra in runs.items():
            FLAGS.reset()
            out[name] = os.path.join(root, 'out_' + name, 'toy')
            E.cli(base + ['--savepath', os.path.dirname(out[name])] + extra)
    finally:
        FLAGS.reset()
        E._Pipelines.CO_RESIDENT = False
    two_step = os.path.join(out['plain'], 'final3d_model.ply')
    DF.main(['--dense_folder', out['plain']] + fuse_args)            # without the new options: the six-property file
    old_p, old_c, old_n = ply.read_ply_normals(two_step)
    assert old_n is None and len(old_p) > 0
    with open(two_step, 'rb') as f:
        assert f.read(200).count(b'property') == 6
    DF.main(['--dense_folder', out['plain']] + fuse_args + ['--normals', 'depth', '--normal_threshold', '80', '--normal_step', '2',
                                                            '--normal_depth_gate', '0.5'])
    want_p, want_c, want_n = ply.read_ply_normals(two_step)
    got_p, got_c, got_n = ply.read_ply_normals(os.path.join(out['normals'], 'final3d_model.ply'))
    assert 0 < len(got_p) < len(old_p)                               # the normal test decided something
    assert got_p.shape == want_p.shape and got_p.tobytes() == want_p.tobytes()
    assert got_n.tobytes() == want_n.tobytes()
    length = np.linalg.norm(got_n.astype(np.float64), axis=-1)
    zero = (got_n == 0).all(-1)
    assert (np.abs(length[~zero] - 1.0) <= 2.0 ** -23).all() and (~zero).any()
    # colours, and the normals once more, from the file pipeline's maps with the in-run images
    pf = os.path.join(out['plain'], 'points_atvsnet')
    names = ['%08d' % i for i in range(_N_IMAGES)]
    Ps = [DF.read_p_file(os.path.join(pf, 'cams', s + '.jpg.P')) for s in names]
    depths = np.stack([DF.read_gipuma_dmb(os.path.join(pf, '2333__' + s, 'disp.dmb')) for s in names])
    normals = np.stack([DF.read_gipuma_dmb(os.path.join(pf, '2333__' + s, 'normals.dmb')) for s in names])
    restated = R.depth_normals(DF.pack_cameras(Ps), depths, 2, 0.5)
    assert np.abs(normals.astype(np.float64) - restated).max() <= 2.0 ** -23 and (normals != 0).any()
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
    ref_p, ref_c, ref_n = DF.fuse_views(Ps, depths, normals, images, 0.5, DF.normal_threshold_radians(80), 1, device=cuda,
                                        return_normals=True)
    assert ref_p.tobytes() == got_p.tobytes() and ref_c.tobytes() == got_c.tobytes()
    assert DF.unit_normals(ref_n).tobytes() == got_n.tobytes()
