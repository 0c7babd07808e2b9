"""The reference's two real 5-view scenes as inputs of small tests: their ten cameras (tests/golden/example{0,1}_{0..4}_cam.npy,
(2,4,4) float64 as the reference ships them), scaled to a small map.  Plain helpers, no fixtures.

What these cameras have that synthetic.make_cams and geometry_cases.general_cams do not: rotations of tens of degrees between the
views, so that a third to two thirds of every plane sweep leaves the source image; a depth_start of its own in every view (the
pipeline uses the reference view's for every pair, quirk C11); one K shared by the views.  tests/test_real_cams_host.py pins these
properties on the CPU oracle, tests/test_gpu_real_cams.py runs the HIP path on them.

The images are synthetic.make_inputs' (seeded noise-free renderings, no JPEG decoder): the cameras are what is real here.
tests/golden/make_real_cams_golden.py evaluates the multi-view pipeline on them; load() reads what it wrote.
"""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# the grid the shipped intrinsics are for (the reference's 640x960 images at 1/4 resolution)
CAM_H, CAM_W = 160, 240
# the plane count the shipped depth_interval is for
CAM_D = 128
# (h, w, D) of the checked-in evaluation and the views of each scene it uses: all five of scene 0; of scene 1 the reference view and
# two sources neither of which is the scene's view 1, so the visual hull's camera (quirk C6: view 1 of the list) is a re-indexed one
H, W, D = 24, 40, 16
VIEWS = {0: None, 1: [0, 3, 4]}


def raw_cams(scene):
    """(5, 2, 4, 4) float64, as shipped."""
    return np.stack([np.load(os.path.join(GOLDEN, 'example%d_%d_cam.npy' % (scene, v))) for v in range(5)])


def cams(scene, h, w, D, views=None):
    """(1, N, 2, 4, 4) float32 cameras of `scene` for an (h, w) map swept in D planes: K's row 0 scaled by w / 240 and row 1 by
    h / 160 (at 24 x 40 this makes fx != fy), depth_interval by 128 / D so that D planes span the scene's own range.  views: the
    views to keep, in this order (default all five)."""
    c = raw_cams(scene)
    if views is not None:
        c = c[list(views)]
    c = c.copy()
    c[:, 1, 0, :3] *= w / float(CAM_W)
    c[:, 1, 1, :3] *= h / float(CAM_H)
    c[:, 1, 3, 1] *= float(CAM_D) / D
    return torch.from_numpy(c.astype(np.float32))[None]


def images(n, h, w, D):
    """(1, n, 4h, 4w, 3) float32 seeded images for an (h, w) map."""
    from atvsnet_amd import synthetic
    return torch.from_numpy(synthetic.make_inputs(n, 4 * h, 4 * w, D)[0])


def inputs(scene):
    """(images, cams) of the checked-in evaluation of `scene`."""
    c = cams(scene, H, W, D, VIEWS[scene])
    return images(c.shape[1], H, W, D), c


class float64_networks(object):
    """Context in which the CPU oracle evaluates its NETWORKS in float64 on float64 tensors while its geometry -- sampling
    coordinates, masks, nearest picks, the hull's comparisons -- stays float32, so that the same pixels are sampled (the patching
    of tests/golden/make_truth64_golden.py)."""

    NAMES = ('homography_warping', 'homography_warping_by_depth', 'transform_depth', 'get_visual_hull')

    @staticmethod
    def _f32_boundary(fn):
        def wrapped(*args, **kw):
            args = [a.float() if isinstance(a, torch.Tensor) and a.dtype == torch.float64 else a for a in args]
            out = fn(*args, **kw)
            if isinstance(out, tuple):
                return tuple(o.double() if o.dtype == torch.float32 else o for o in out)
            return out.double() if out.dtype == torch.float32 else out
        return wrapped

    def __enter__(self):
        from oracle import homography_warping as G
        from oracle import tf_ops as T
        self.saved = {name: getattr(G, name) for name in self.NAMES}
        for name, fn in self.saved.items():
            setattr(G, name, self._f32_boundary(fn))
        self.linspace = T.linspace
        T.linspace = lambda a, b, n: self.linspace(float(a), float(b), n).double()
        return self

    def __exit__(self, *exc):
        from oracle import homography_warping as G
        from oracle import tf_ops as T
        for name, fn in self.saved.items():
            setattr(G, name, fn)
        T.linspace = self.linspace
        return False


def forced_refinement(imgs, cams, Wt, D, depth_agg_init, depth_views, prob_volume_agg, cost_volume_agg, sources=None):
    """The oracle's stages after AAM1 (run_multiview's second half) on GIVEN stage inputs -> (refined cost volume of every source
    in `sources` (default all), AAM2 cost, AAM2 prob, final depth (1,4h,4w,1)); the last three are None for a subset of sources."""
    from oracle import model as OM
    from oracle import nets
    ds, di = OM.depth_start_interval(cams)
    n = cams.shape[1]
    rc = [OM.TVSNet_refine(depth_agg_init, depth_views[v - 1], prob_volume_agg, cost_volume_agg, imgs, cams, D, ds, di, Wt,
                           view_i=v, ref_i=0)[1] for v in (range(1, n) if sources is None else sources)]
    if sources is not None:
        return rc, None, None, None
    rcagg = OM.cost_volume_aggregation_refine(torch.stack(rc, -1), Wt)
    rpagg = nets.output_conv(rcagg, Wt, 'attention_prob_vol_refine')
    return rc, rcagg, rpagg, OM.prob2depth_upsample(rpagg, D, ds, di)[1]


def vol_dist(got, ref):
    """max|got - ref| / max|ref|: the distance of a volume from its float64 value."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max())


def rel_l1(got, ref):
    """mean(|got - ref| / |ref|): the distance of a depth map from its float64 value."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / ref.abs().clamp(min=1e-12)).mean())


def load(scene):
    """Everything tests/golden/make_real_cams_golden.py wrote for `scene` as {name: numpy array}: real_cams_scene<scene>.npz and its
    real_cams_scene<scene>_vol<k>.npz parts (the 8-channel volumes, two to a file)."""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'real_cams_scene%d*.npz' % scene))):
        with np.load(path) as z:
            for k in z.files:
                assert k not in out, k
                out[k] = z[k]
    return out
