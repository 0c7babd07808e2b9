"""Fusion rates: the per-camera loop (depth_fusion.fuse_views) against the whole-scene pass (depth_fusion.SceneFusion.run).

A synthetic N-view plane scene at 120x224 (the driver's depth-map size, 896x480 / 4) for each N of --views: a tilted plane seen
by N pinhole cameras on an arc, exact depth maps with 0.4 % noise, smooth colour images.  Every map is staged with
SceneFusion.add as a network output (inverse depth, probability map, 1/4 image, write_cam camera); then, --reps times each after
one warm-up:

    fuse_views       the per-camera loop on the staged maps (one atvs_fusibile launch per camera, each followed by a blocking
                     download and the host filter; the upload of the maps included)
    scene            SceneFusion.run() (one atvs_fusibile_scene pass: count, scan, scatter; one download of the points)

and the two results are compared byte for byte.  --kernel-stats DIR merges the kernel times of a rocprofv3 --kernel-trace --stats
run of this tool (one per N, `<DIR>/n<N>/**/*kernel_stats.csv`) into the JSON.

    python tools_dev/fusion_rate.py --out profiles/fusion_rate.json [--kernel-stats DIR]
"""
import argparse
import csv
import glob
import hashlib
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import atvsnet_amd  # noqa: E402,F401
from atvsnet_amd.atvsnet import depth_fusion as DF  # noqa: E402

ROWS, COLS = 120, 224
MEASURED = ['a-tvsnet_amd/csrc/fusion.hip', 'a-tvsnet_amd/csrc/fusion_scene.hip', 'a-tvsnet_amd/csrc/fusion_pixel.h',
            'a-tvsnet_amd/atvsnet/depth_fusion.py', 'a-tvsnet_amd/ops/aanet.py', 'tools_dev/fusion_rate.py']


def plane_scene(n, rows=ROWS, cols=COLS, seed=0):
    """-> (write_cam cameras (n,2,4,4), inverse-depth maps (n,rows,cols), probabilities, BGR uint8 images): a tilted plane z ~ 5
    seen by n cameras spread over a 12-degree arc and a 1.6-unit baseline."""
    rng = np.random.default_rng(seed)
    f = 0.9 * cols
    K = np.array([[f, 0, cols / 2.0], [0, f, rows / 2.0], [0, 0, 1]])
    nrm = np.array([0.1, -0.05, -1.0])
    nrm /= np.linalg.norm(nrm)
    d0 = 5.0
    ys, xs = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    cams, inv, images = [], [], []
    for i in range(n):
        u = i / max(n - 1, 1) - 0.5
        ang = np.deg2rad(12.0 * u)
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        C = np.array([1.6 * u, 0.1 * u, 0.0])
        cam = np.zeros((2, 4, 4))
        cam[0, :3, :3], cam[0, :3, 3], cam[0, 3, 3] = R, -R @ C, 1.0
        cam[1, :3, :3] = K
        cam[1, 3] = (0.1, 0.01, 128, 0.5)
        cams.append(cam)
        rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T @ R
        s = -(nrm @ C + d0) / (rays @ nrm)
        inv.append((1.0 / (s * (1.0 + 0.004 * rng.normal(size=s.shape)))).astype(np.float32))
        X = C + s[..., None] * rays
        img = 127.0 + 100.0 * np.stack([np.sin(X[..., 0] * 2.0), np.cos(X[..., 1] * 3.0), np.sin(X[..., 0] + X[..., 1])], -1)
        images.append(np.clip(img + rng.uniform(0, 4, img.shape), 0, 255).astype(np.uint8))
    prob = rng.uniform(0.6, 1.0, (n, rows, cols)).astype(np.float32)
    return np.stack(cams), np.stack(inv), prob, np.stack(images)


def measured_head():
    try:
        return subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                              check=True).stdout.decode().strip()
    except (OSError, subprocess.CalledProcessError):
        try:
            with open(os.path.join(ROOT, 'profiles', '.measured_head')) as f:
                return f.read().strip()
        except OSError:
            return None


def sources_sha1():
    h = hashlib.sha1()
    for p in MEASURED:
        with open(os.path.join(ROOT, p), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def kernel_stats(path):
    rows = []
    for f in sorted(glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if 'fusi' in r['Name']:
                    rows.append({'name': r['Name'], 'calls': int(r['Calls']), 'total_ms': float(r['TotalDurationNs']) / 1e6,
                                 'average_us': float(r['AverageNs']) / 1e3})
    return rows


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', default='16,64,256')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-stats', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    disp, ncons = 0.01, 2
    results = []
    for n in [int(v) for v in a.views.split(',')]:
        cams, inv, prob, images = plane_scene(n)
        fusion = DF.SceneFusion(n, ROWS, COLS, dev, prob_threshold=0.8, disp_threshold=disp, num_consistent=ncons, inverse_depth=True)
        for i in range(n):
            fusion.add(i, inv[i], prob[i], images[i], cams[i])
        torch.cuda.synchronize()
        nd, img = fusion.nd.cpu().numpy(), fusion.img.cpu().numpy()
        Ps = [DF.projection_matrix(DF.load_cam(io.StringIO(DF.cam_text(c)))) for c in cams]
        depths, normals, bgr = nd[..., 3], nd[..., :3], img[..., :3].astype(np.uint8)

        def per_camera():
            return DF.fuse_views(Ps, depths, normals, bgr, disp, DF.NORMAL_THRESHOLD, ncons, device=dev)

        def scene():
            fusion.result = None
            return fusion.run()

        times = {'fuse_views': [], 'scene': []}
        out = {}
        for name, fn in (('fuse_views', per_camera), ('scene', scene)):
            out[name] = fn()                                     # warm-up
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append(1e3 * (time.perf_counter() - t0))
        (pa, ca), (pb, cb) = out['fuse_views'], out['scene']
        same = pa.tobytes() == pb.tobytes() and ca.tobytes() == cb.tobytes()
        row = {'views': n, 'size': '%dx%d' % (COLS, ROWS), 'points': int(len(pb)), 'bitwise_equal': same,
               'fuse_views_ms': float(np.median(times['fuse_views'])), 'scene_ms': float(np.median(times['scene'])),
               'fuse_views_ms_all': times['fuse_views'], 'scene_ms_all': times['scene']}
        row['speedup'] = row['fuse_views_ms'] / row['scene_ms']
        if a.kernel_stats:
            row['kernels'] = kernel_stats(os.path.join(a.kernel_stats, 'n%d' % n))
        results.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith('_all')}), flush=True)
        if not same:
            raise SystemExit('n=%d: the scene pass and fuse_views differ' % n)
        del fusion
    summary = {'parent_commit': measured_head(), 'measured_sources_sha1': sources_sha1(), 'measured_sources': MEASURED,
               'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'disp_threshold': disp, 'num_consistent': ncons,
               'normal_threshold_rad': DF.NORMAL_THRESHOLD, 'results': results}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
