"""COLMAP import rate: a large synthetic model (default 2000 images, 10^6 points, 8 observers per point) imported with
colmap.make_scene, its two GPU passes timed alone, and both compared with a vectorised numpy restatement of the same arithmetic.

The model is written in COLMAP's binary format (one PINHOLE camera, 2000 cameras on a ring looking at a ball of points; each point
observed by 8 distinct random images) next to one tiny JPEG that every image name links to.  Then, after one warm-up:

    read_s          colmap.read_model (binary parse, rotations, track CSR)
    import_s        colmap.make_scene(link=True): read, depth ranges, co-visibility, sources, every file written
    depth_range_ms  ops.colmap_depth_range alone (HIP events; 8 radix passes over all image x point pairs), median of --reps
    covis_ms        ops.colmap_covisibility alone (HIP events), median of --reps
    numpy_*_s       the restatement: per image the projection in the same order, np.sort and the two ranks (tests/colmap_model.py's
                    ranges_numpy); the pair counts as one np.bincount over every ordered pair of every track

and checks that the GPU results equal the restatement (bit for bit; counts exactly).  --numpy_images N restates the depth range on
the first N images only (the time is then reported for N and scaled to all images, and named so).

    python tools_dev/colmap_rate.py --out profiles/colmap_import.json
"""
import argparse
import json
import os
import shutil
import struct
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
from colmap_model import ranges_numpy  # noqa: E402
from fusion_rate import measured_head  # noqa: E402

W, H, F = 1600, 1200, 1400.0


def synthetic_model(root, n_images, n_points, observers, seed=0):
    rng = np.random.default_rng(seed)
    sparse, images = os.path.join(root, 'sparse'), os.path.join(root, 'images')
    os.makedirs(sparse)
    os.makedirs(images)
    with open(os.path.join(sparse, 'cameras.bin'), 'wb') as f:
        f.write(struct.pack('<QiiQQ4d', 1, 1, 1, W, H, F, F, W / 2.0, H / 2.0))
    # cameras on a ring of radius 10 around the origin, looking at it (world to camera R, t), a little jitter
    ang = 2 * np.pi * np.arange(n_images) / n_images
    centres = np.stack([10 * np.cos(ang), rng.uniform(-1, 1, n_images), 10 * np.sin(ang)], 1)
    z = -centres / np.linalg.norm(centres, axis=1, keepdims=True)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 1)
    t = -np.einsum('kij,kj->ki', R, centres)
    q = np.array([_quat(r) for r in R])
    xyz = rng.normal(size=(n_points, 3)) * 2.0
    # `observers` distinct images per point: a random start and increasing strides that stay below one turn of the ring
    steps = np.cumsum(rng.integers(1, max(2, n_images // observers), (n_points, observers)), 1)
    obs_img = (rng.integers(0, n_images, (n_points, 1)) + steps - steps[:, :1]) % n_images
    pid = np.repeat(np.arange(1, n_points + 1), observers)
    img = obs_img.reshape(-1)
    order = np.argsort(img, kind='stable')
    counts = np.bincount(img, minlength=n_images)
    rec = np.dtype([('x', '<f8'), ('y', '<f8'), ('id', '<i8')])
    with open(os.path.join(sparse, 'images.bin'), 'wb') as f:
        f.write(struct.pack('<Q', n_images))
        start = 0
        for k in range(n_images):
            o = np.zeros(counts[k], rec)
            o['id'] = pid[order[start:start + counts[k]]]
            start += counts[k]
            name = 'img_%05d.jpg' % k
            f.write(struct.pack('<i4d3di', k + 1, *(list(q[k]) + list(t[k]) + [1])) + name.encode() + b'\0')
            f.write(struct.pack('<Q', counts[k]) + o.tobytes())
            os.symlink(os.path.join(root, 'tiny.jpg'), os.path.join(images, name))
    pt = np.dtype([('id', '<u8'), ('xyz', '<f8', 3), ('rgb', 'u1', 3), ('err', '<f8'), ('n', '<u8'), ('track', '<i4', (observers, 2))])
    p = np.zeros(n_points, pt)
    p['id'], p['xyz'], p['n'] = np.arange(1, n_points + 1), xyz, observers
    p['track'][..., 0] = obs_img + 1
    with open(os.path.join(sparse, 'points3D.bin'), 'wb') as f:
        f.write(struct.pack('<Q', n_points) + p.tobytes())
    from PIL import Image
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(os.path.join(root, 'tiny.jpg'))


def _quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    x = np.copysign(np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2.0, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2.0, R[1, 0] - R[0, 1])
    return (w, x, y, z)


def covis_numpy(offsets, observers, n_images, chunk=65536):
    """Every ordered pair (i != j) of every track counted with np.bincount, tracks in chunks."""
    out = np.zeros(n_images * n_images, np.int64)
    for t0 in range(0, len(offsets) - 1, chunk):
        off = offsets[t0:t0 + chunk + 1].astype(np.int64)
        lens = np.diff(off)
        sq = lens * lens
        start, L = np.repeat(off[:-1], sq), np.repeat(lens, sq)
        q = np.arange(len(L)) - np.repeat(np.cumsum(sq) - sq, sq)
        i, j = q // np.maximum(L, 1), q % np.maximum(L, 1)
        keep = i != j
        a, b = observers[(start + i)[keep]].astype(np.int64), observers[(start + j)[keep]].astype(np.int64)
        out += np.bincount(a * n_images + b, minlength=n_images * n_images)
    return out.reshape(n_images, n_images)


def _events_ms(fn, reps):
    import torch
    out, times = fn(), []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return out, times


def main():
    import torch
    from atvsnet_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=2000)
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--observers', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--numpy_images', type=int, default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    root = tempfile.mkdtemp(prefix='colmap_rate_')
    t0 = time.time()
    synthetic_model(root, a.images, a.points, a.observers)
    print('model written in %.1f s' % (time.time() - t0), flush=True)
    C.make_scene(root, os.path.join(root, 'warm'), link=True)                 # warm-up: code objects, allocator
    t0 = time.perf_counter()
    m = C.read_model(os.path.join(root, 'sparse'))
    read_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    r = C.make_scene(root, os.path.join(root, 'scene'), link=True)
    import_s = time.perf_counter() - t0
    print('read %.2f s, import %.2f s' % (read_s, import_s), flush=True)
    pts = torch.from_numpy(m.xyz).to(dev)
    cams = torch.from_numpy(C.camera_rows(m)).to(dev)
    off, obs = torch.from_numpy(m.offsets).to(dev), torch.from_numpy(m.observers).to(dev)
    (n, lo, hi), dr_ms = _events_ms(lambda: ops.colmap_depth_range(pts, cams, 0.99), a.reps)
    covis, cv_ms = _events_ms(lambda: ops.colmap_covisibility(off, obs, len(m.image_ids)), a.reps)
    print('depth range %.2f ms, covisibility %.2f ms (medians)' % (np.median(dr_ms), np.median(cv_ms)), flush=True)
    k = a.numpy_images or len(m.image_ids)
    t0 = time.perf_counter()
    wn, wlo, whi = ranges_numpy(m.xyz, m.R[:k], m.t[:k], m.intrinsics[:k], m.size[:k], 0.99)
    np_range_s = time.perf_counter() - t0
    print('numpy depth range on %d images: %.1f s' % (k, np_range_s), flush=True)
    N = len(m.image_ids)
    t0 = time.perf_counter()
    want_cov = covis_numpy(m.offsets, m.observers, N)
    np_covis_s = time.perf_counter() - t0
    print('numpy covisibility: %.1f s' % np_covis_s, flush=True)
    same_range = (np.array_equal(n.cpu().numpy()[:k], wn) and lo.cpu().numpy()[:k].tobytes() == wlo.tobytes()
                  and hi.cpu().numpy()[:k].tobytes() == whi.tobytes())
    same_cov = np.array_equal(covis.cpu().numpy(), want_cov) and np.array_equal(r['shared'], want_cov)
    row = {'images': len(m.image_ids), 'points': int(len(m.xyz)), 'observations': int(m.offsets[-1]),
           'pairs_projected_per_pass': int(len(m.image_ids)) * int(len(m.xyz)), 'points_in_view_median': float(np.median(r['n'])),
           'read_s': read_s, 'import_s': import_s, 'depth_range_ms': float(np.median(dr_ms)), 'covis_ms': float(np.median(cv_ms)),
           'depth_range_ms_all': dr_ms, 'covis_ms_all': cv_ms, 'numpy_depth_range_images': k, 'numpy_depth_range_s': np_range_s,
           'numpy_depth_range_s_all_images': np_range_s * len(m.image_ids) / k, 'numpy_covis_s': np_covis_s,
           'depth_range_bitwise_equal': bool(same_range), 'covis_equal': bool(same_cov)}
    print(json.dumps({kk: v for kk, v in row.items() if not kk.endswith('_all')}), flush=True)
    if not (same_range and same_cov):
        raise SystemExit('the GPU results differ from the numpy restatement')
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'percentile': 0.99,
               'result': row}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)
    shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
