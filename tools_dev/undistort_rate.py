"""Undistortion rate at ETH3D's DSLR size: a 6048 x 4032 THIN_PRISM_FISHEYE camera.

    map_ms, remap_ms   ops.undistort_map / ops.undistort_remap alone (HIP events around one launch, after a warm-up; median of
                       --reps), with the bytes each must move (map: 8 B written per output pixel; remap: 8 B of map read, 3 B
                       written and 12 B of taps gathered per output pixel, the taps mostly from cache) over that time
    numpy_*_s          the float64 numpy restatement of the same arithmetic (tests/undistort_restated.py) on the same camera, and
                       whether the GPU results equal it (the map up to atan's ties: see tests/test_gpu_undistort.py)
    import             colmap.make_scene(sparse, image_path) of --images synthetic photographs of that camera, with 1 worker (the
                       phases then add up to the wall clock, so the codec's share is a share of it) and with 16 workers: wall
                       seconds and the seconds spent in JPEG decode, on the GPU (upload, launch, download) and in JPEG encode

No rate here is a pass / fail bar.

    python tools_dev/undistort_rate.py --out profiles/undistort.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import atvsnet_amd  # noqa: E402,F401
from atvsnet_amd.atvsnet import colmap as C  # noqa: E402
from atvsnet_amd.atvsnet import undistort as U  # noqa: E402
import undistort_restated as R  # noqa: E402
from colmap_model import write_text  # noqa: E402
from colmap_rate import _events_ms  # noqa: E402
from fusion_rate import measured_head  # noqa: E402

W, H = 6048, 4032
# of the kind of ETH3D's DSLR calibrations: a 3400-pixel focal length on a rectilinear lens, so k1, k2 are mostly tan's series
# (theta + theta^3 / 3 + 2 theta^5 / 15) and what is left is a barrel distortion of a few per cent at the corner
PARAMS = (3410.0, 3408.0, 3040.5, 2010.25, 0.29, 0.11, 0.0004, -0.0003, 0.02, 0.003, 0.0005, -0.0004)
MODEL = 'THIN_PRISM_FISHEYE'


def photographs(root, n_images, seed=0):
    """n_images smooth-texture JPEGs of W x H and a text model that sees 200 points in each."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, 'photos'))
    base = rng.integers(0, 256, (H // 16 + 2, W // 16 + 2, 3), dtype=np.uint8)
    images = []
    for i in range(n_images):
        tile = np.kron(base[i % 2:i % 2 + H // 16, :W // 16], np.ones((16, 16, 1), np.uint8))
        Image.fromarray(tile).save(os.path.join(root, 'photos', 'dslr_%02d.jpg' % i), quality=95)
        images.append((i + 1, (1.0, 0.0, 0.0, 0.0), (0.05 * i, 0.0, 0.0), 1, 'dslr_%02d.jpg' % i, [(0.0, 0.0, p + 1) for p in range(200)]))
    xyz = np.concatenate([rng.uniform(-1.0, 1.0, (200, 2)), rng.uniform(4.0, 6.0, (200, 1))], 1)
    points = [(p + 1, tuple(xyz[p]), [(i + 1, p) for i in range(n_images)]) for p in range(200)]
    write_text(os.path.join(root, 'sparse'), [(1, MODEL, W, H, PARAMS)], images, points)


def main():
    import torch
    from atvsnet_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    t0 = time.perf_counter()
    camera = U.undistorted_camera(MODEL, PARAMS, W, H)
    camera_s = time.perf_counter() - t0
    (_, (wo, ho)) = camera
    n_out = wo * ho
    print('output camera %s in %.2f s (host)' % (camera, camera_s), flush=True)
    rng = np.random.default_rng(1)
    src = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    m, map_ms = _events_ms(lambda: ops.undistort_map(MODEL, PARAMS, W, H, camera), a.reps)
    out, remap_ms = _events_ms(lambda: ops.undistort_remap(src, m), a.reps)
    print('map %.3f ms, remap %.3f ms (medians of %d)' % (np.median(map_ms), np.median(remap_ms), a.reps), flush=True)
    t0 = time.perf_counter()
    want_q, tie = R.sampling_map(MODEL, PARAMS, W, H, camera)
    numpy_map_s = time.perf_counter() - t0
    got_q = m.cpu().numpy()
    t0 = time.perf_counter()
    want_img = R.sample(src.cpu().numpy(), got_q)
    numpy_remap_s = time.perf_counter() - t0
    dq = np.abs(got_q.astype(np.int64) - want_q.astype(np.int64))
    differ = dq != 0
    row = {'model': MODEL, 'source': [W, H], 'output': [wo, ho], 'output_camera_host_s': camera_s,
           'map_ms': float(np.median(map_ms)), 'remap_ms': float(np.median(remap_ms)), 'map_ms_all': map_ms, 'remap_ms_all': remap_ms,
           'map_written_GB_per_s': 8.0 * n_out / np.median(map_ms) / 1e6,
           'remap_map_plus_output_GB_per_s': 11.0 * n_out / np.median(remap_ms) / 1e6,
           'numpy_map_s': numpy_map_s, 'numpy_remap_s': numpy_remap_s,
           'map_coordinates': int(dq.size), 'map_coordinates_differing': int(differ.sum()),
           'map_max_abs_difference': int(dq.max()),
           'map_differences_all_within_1e-6_of_a_tie': bool((tie[differ] < 1e-6).all()),
           'restatement_coordinates_within_1e-6_of_a_tie': int((tie < 1e-6).sum()),
           'remap_equal_on_the_same_map': bool(np.array_equal(out.cpu().numpy(), want_img))}
    del want_q, tie, got_q, want_img, dq, differ
    root = tempfile.mkdtemp(prefix='undistort_rate_')
    t0 = time.time()
    photographs(root, a.images)
    print('%d photographs written in %.1f s' % (a.images, time.time() - t0), flush=True)
    imports = {}
    for workers in (1, 16):
        dst = os.path.join(root, 'scene_%d' % workers)
        t0 = time.perf_counter()
        r = C.make_scene(None, dst, sparse=os.path.join(root, 'sparse'), image_path=os.path.join(root, 'photos'), workers=workers)
        wall = time.perf_counter() - t0
        s = r['seconds']
        imports['workers_%d' % workers] = {
            'images': len(r['undistorted']), 'wall_s': wall, 'decode_s': s['decode'], 'gpu_upload_launch_download_s': s['gpu'],
            'encode_s': s['encode'], 'codec_share_of_wall': (s['decode'] + s['encode']) / wall if workers == 1 else None,
            'jpeg_bytes_per_image': os.path.getsize(os.path.join(dst, 'images', '00000000.jpg'))}
        print(json.dumps(imports['workers_%d' % workers]), flush=True)
    row['import'] = imports
    print(json.dumps({k: v for k, v in row.items() if not k.endswith('_all')}), flush=True)
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'result': row}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)
    shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
