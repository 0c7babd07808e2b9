"""Scene driver rates: eval_pointcloud's default mode against --scene_cache on one synthetic ETH3D-style scene.

Writes a scene of --views images at 940x490 (ETH3D low-res size) with a ring pair.txt of 7 sources each, then runs the driver
(--view_num 8 --max_d 128, synthetic weights) in the default mode and with --scene_cache, alternating, --reps times each, in this
process.  Reports maps/s per mode (median, min, max), the per-map host time split (prepare, submit, wait, write) and the largest
relative depth difference between the two modes' PFMs; --out writes the same as JSON.  Each run processes the scene twice under
two names: the first pass carries the run's graph captures; maps/s and the per-map split are the second pass's (zz_runtime.txt,
eth3d_maps.TIMES).  The split: prepare, submit (scene mode: of which upload), wait, write (scene mode: the hand-off to the writer
thread), writer_busy (the writer thread's own time), and in scene mode gpu_ms (each map's GPU time on its slot's stream, median).

    python tools_dev/scene_rate.py --out profiles/scene_rate.json [--maps_in_flight cu_split]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import atvsnet_amd  # noqa: E402,F401
from atvsnet_amd import FLAGS, synthetic  # noqa: E402
from atvsnet_amd.atvsnet import eval_pointcloud as E, preprocess as P  # noqa: E402


def write_scene(root, name, n, h=490, w=940, sources=7):
    from PIL import Image
    scene = os.path.join(root, 'eth3d', name)
    os.makedirs(os.path.join(scene, 'images'))
    os.makedirs(os.path.join(scene, 'cams'))
    cams = synthetic.make_cams(n, h, w, 128)
    for v in range(n):
        img = np.clip(synthetic.make_images(1, h, w, seed=v)[0], 0, 255).astype(np.uint8)
        Image.fromarray(img[:, :, ::-1]).save(os.path.join(scene, 'images', '%08d.jpg' % v), quality=95)
        cam = cams[v].astype(np.float64).copy()
        cam[1, :2, :3] *= 4
        cam[1, 3] = (2.0, 0.05, 128, 0.0)
        P.write_cam(os.path.join(scene, 'cams', '%08d_cam.txt' % v), cam)
    with open(os.path.join(scene, 'pair.txt'), 'w') as f:
        f.write('%d\n' % n)
        for v in range(n):
            f.write('%d\n%d %s\n' % (v, sources, ' '.join('%d 1.0' % ((v + k) % n) for k in range(1, sources + 1))))
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=24)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--maps_in_flight', choices=('serial', 'cu_split'), default='serial')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = tempfile.mkdtemp(prefix='scene_rate_')
    # the same scene twice under two names: the first carries the graph captures of the run, the rate is the second's wall clock
    n = write_scene(root, 'warm', max(a.views, 24))
    write_scene(root, 'ring', n)
    rows = {'default': [], 'scene_cache': []}
    outs = {}
    for rep in range(a.reps):
        for mode in ('default', 'scene_cache'):
            FLAGS.reset()
            save = os.path.join(root, 'out_%s' % mode)
            argv = ['--data_root', root, '--savepath', save, '--view_num', '8', '--max_d', '128', '--synthetic_weights',
                    '--scenes', 'warm,ring', '--maps_in_flight', a.maps_in_flight] + (['--scene_cache'] if mode == 'scene_cache' else [])
            E.cli(argv)
            with open(os.path.join(save, 'ring', 'zz_runtime.txt')) as f:
                dt = float(f.read().split()[1])
            t = dict(E.TIMES)                     # the ring pass alone
            m = t.pop('maps')
            gpu = t.pop('gpu_ms', None)
            row = dict(maps=n, seconds=dt, maps_per_s=n / dt, **{k + '_ms_per_map': 1e3 * v / m for k, v in t.items()})
            if gpu:
                row['gpu_ms_per_map'] = float(np.median(gpu))
                row['gpu_ms_per_map_max'] = float(np.max(gpu))
            rows[mode].append(row)
            outs[mode] = os.path.join(save, 'ring', 'depths_atvsnet')
            print(mode, rep, json.dumps(rows[mode][-1]), flush=True)
    rel, rel_mean = 0.0, []
    for i in range(n):
        with open(os.path.join(outs['default'], '%08d.pfm' % i), 'rb') as f:
            d0 = P.load_pfm(f)
        with open(os.path.join(outs['scene_cache'], '%08d.pfm' % i), 'rb') as f:
            d1 = P.load_pfm(f)
        ok = np.isfinite(d0) & np.isfinite(d1) & (d0 != 0)
        r = np.abs(d1 - d0)[ok] / np.abs(d0[ok])
        rel = max(rel, float(r.max()))
        rel_mean.append(float(r.mean()))
    summary = {'views': n, 'view_num': 8, 'max_d': 128, 'size': '940x490', 'maps_in_flight': a.maps_in_flight,
               'max_rel_depth_diff': rel, 'mean_rel_depth_diff': float(np.mean(rel_mean)), 'runs': rows}
    for mode, r in rows.items():
        rates = [x['maps_per_s'] for x in r]
        summary[mode] = {'maps_per_s_median': float(np.median(rates)), 'min': min(rates), 'max': max(rates),
                         **{k: float(np.median([x[k] for x in r])) for k in r[0] if '_ms_per_map' in k}}
    print(json.dumps({k: v for k, v in summary.items() if k != 'runs'}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
