"""Generates tests/golden/real_cams_scene{0,1}.npz and their real_cams_scene{0,1}_vol<k>.npz parts: the multi-view pipeline on the
reference's real 5-view cameras (tests/real_cams.py) at a 24x40 map with 16 planes, evaluated by the CPU oracle in float32 and
with its networks in float64 (geometry stays float32, as in make_truth64_golden.py).  Scene 0: all five views; scene 1: views
[0, 3, 4].  Run from the repository root (about ten seconds on 8 cores).

Per scene:
  depth_views (S,h,w), depth_agg_init (h,w), prob_volume_agg (D,h,w), cost_volume_agg (D,h,w,8)
      the float32 oracle's free-running base stage and AAM1: the FORCED INPUTS of the refinement below
  depth_views64 ... cost_volume_agg64
      the same stages with float64 networks, free-running (nothing upstream of them is discrete beyond the warp coordinates)
  refined_cost64_<v> (D,h,w,8) per source v, refined_cost_volume_agg64, refined_prob_volume_agg64, depth_final64 (4h,4w)
      the refinement, AAM2 and the final depth with float64 networks ON THE FORCED INPUTS (the float32 ones above, so that the
      nearest picks, masks and hull voxels are those of the float32 run)
  refined_cost32_<last source>
      the float32 oracle's forced refinement of the last source (tests/test_real_cams_host.py re-runs it: no stale fixture)
  depth_free32, depth_free64 (4h,4w)
      the final depth of the free-running float32 / float64-network pipelines
  e32_<name>
      the float32 oracle's own distance from every float64 quantity above (max|x32 - x64| / max|x64| for volumes, rel-L1 for
      depth maps), computed before the float64 values are rounded to float32 for storage (6e-8 relative)
No file may exceed 1 MiB: the 8-channel volumes go two to a part.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import atvsnet_amd                                     # noqa: E402,F401
from atvsnet_amd import variables                      # noqa: E402
from oracle import model as OM                         # noqa: E402
import real_cams as RC                                 # noqa: E402

torch.set_num_threads(min(os.cpu_count() or 1, 32))     # as tests/conftest.py
PART_BYTES = 1000000


def evaluate(scene, W32, W64):
    h, w, D = RC.H, RC.W, RC.D
    imgs, cams = RC.inputs(scene)
    n = cams.shape[1]
    S32, S64 = {}, {}
    free32 = OM.run_multiview(imgs, cams, W32, D, S32)
    with RC.float64_networks():
        free64 = OM.run_multiview(imgs.double(), cams, W64, D, S64)
    forced = (S32['depth_agg_init'], S32['depth_views'], S32['prob_volume_agg'], S32['cost_volume_agg'])
    rc32, rcagg32, rpagg32, final32 = RC.forced_refinement(imgs, cams, W32, D, *forced)
    with RC.float64_networks():
        f64 = (forced[0].double(), [d.double() for d in forced[1]], forced[2].double(), forced[3].double())
        rc64, rcagg64, rpagg64, final64 = RC.forced_refinement(imgs.double(), cams, W64, D, *f64)
    # forcing the float32 stage's own outputs reproduces the free-running float32 pipeline
    assert torch.equal(final32, free32) and torch.equal(rcagg32, S32['refined_cost_volume_agg'])

    out = {}

    def both(name, x32, x64, depth, keep32=True, name64=None):
        out['e32_' + name] = np.float64(RC.rel_l1(x32, x64) if depth else RC.vol_dist(x32, x64))
        out[name64 or name + '64'] = x64.float().numpy()
        if keep32:
            out[name] = x32.numpy()

    both('depth_views', torch.stack(S32['depth_views'])[:, 0, ..., 0], torch.stack(S64['depth_views'])[:, 0, ..., 0], True)
    for i in range(n - 1):
        out['e32_depth_views_%d' % (i + 1)] = np.float64(RC.rel_l1(S32['depth_views'][i], S64['depth_views'][i]))
    both('depth_agg_init', S32['depth_agg_init'][0, ..., 0], S64['depth_agg_init'][0, ..., 0], True)
    both('prob_volume_agg', S32['prob_volume_agg'][0], S64['prob_volume_agg'][0], False)
    both('cost_volume_agg', S32['cost_volume_agg'][0], S64['cost_volume_agg'][0], False)
    for i in range(n - 1):
        both('refined_cost_%d' % (i + 1), rc32[i][0], rc64[i][0], False, keep32=False, name64='refined_cost64_%d' % (i + 1))
    out['refined_cost32_%d' % (n - 1)] = rc32[-1][0].numpy()
    both('refined_cost_volume_agg', rcagg32[0], rcagg64[0], False, keep32=False)
    both('refined_prob_volume_agg', rpagg32[0], rpagg64[0], False, keep32=False)
    both('depth_final', final32[0, ..., 0], final64[0, ..., 0], True, keep32=False)
    out['depth_free32'] = free32[0, ..., 0].numpy()
    out['depth_free64'] = free64[0, ..., 0].float().numpy()
    out['e32_depth_free'] = np.float64(RC.rel_l1(free32, free64))
    assert out['cost_volume_agg'].shape == (D, h, w, 8) and out['depth_free32'].shape == (4 * h, 4 * w)
    return out


def write(scene, out):
    """Small arrays into real_cams_scene<scene>.npz, the 8-channel volumes greedily into parts of at most PART_BYTES."""
    big = sorted(k for k, v in out.items() if v.nbytes > PART_BYTES // 4)
    main = {k: v for k, v in out.items() if k not in big}
    parts, size = [{}], 0
    for k in big:
        if parts[-1] and size + out[k].nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = out[k]
        size += out[k].nbytes
    files = [('real_cams_scene%d.npz' % scene, main)] + [('real_cams_scene%d_vol%d.npz' % (scene, i), p)
                                                          for i, p in enumerate(parts)]
    for name, arrays in files:
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) <= 1 << 20, name
        print('%s: %d bytes (%s)' % (name, os.path.getsize(path), ', '.join(sorted(arrays))))


def main():
    store = variables.VariableStore().init_synthetic(1234)
    W32 = {k: torch.from_numpy(v) for k, v in store.host.items()}
    W64 = {k: v.double() for k, v in W32.items()}
    for scene in (0, 1):
        out = evaluate(scene, W32, W64)
        for k in sorted(out):
            if k.startswith('e32_'):
                print('scene %d %-32s %.3e' % (scene, k, float(out[k])))
        write(scene, out)


if __name__ == '__main__':
    main()
