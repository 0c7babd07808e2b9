"""Test-side COLMAP model writers (text and binary, COLMAP's documented layouts) and restatements of the reference's
arithmetic, written from the reference's atvsnet/colmap_helpers.py, not from the product's code."""
import os
import struct

import numpy as np

MODEL_IDS = {'SIMPLE_PINHOLE': 0, 'PINHOLE': 1, 'SIMPLE_RADIAL': 2, 'RADIAL': 3, 'OPENCV': 4}


def write_text(sparse, cameras, images, points):
    """cameras: [(id, model, width, height, params)]; images: [(id, (qw,qx,qy,qz), (tx,ty,tz), camera_id, name,
    [(x, y, point3d_id)])]; points: [(id, (X,Y,Z), [(image_id, point2d_idx)])]."""
    os.makedirs(sparse, exist_ok=True)
    with open(os.path.join(sparse, 'cameras.txt'), 'w') as f:
        f.write('# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n')
        f.write('# Number of cameras: %d\n' % len(cameras))
        for cid, model, w, h, params in cameras:
            f.write('%d %s %d %d %s\n' % (cid, model, w, h, ' '.join(repr(float(p)) for p in params)))
    with open(os.path.join(sparse, 'images.txt'), 'w') as f:
        f.write('# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n'
                '#   POINTS2D[] as (X, Y, POINT3D_ID)\n# Number of images: %d, mean observations per image: 0\n' % len(images))
        for iid, q, t, cid, name, obs in images:
            f.write('%d %s %s %d %s\n' % (iid, ' '.join(repr(float(v)) for v in q), ' '.join(repr(float(v)) for v in t), cid, name))
            f.write(' '.join('%r %r %d' % (float(x), float(y), p) for x, y, p in obs) + '\n')
    with open(os.path.join(sparse, 'points3D.txt'), 'w') as f:
        f.write('# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, '
                'POINT2D_IDX)\n# Number of points: %d, mean track length: 0\n' % len(points))
        for pid, X, track in points:
            f.write('%d %s 128 64 32 0.5 %s\n' % (pid, ' '.join(repr(float(v)) for v in X), ' '.join('%d %d' % o for o in track)))


def write_binary(sparse, cameras, images, points):
    os.makedirs(sparse, exist_ok=True)
    with open(os.path.join(sparse, 'cameras.bin'), 'wb') as f:
        f.write(struct.pack('<Q', len(cameras)))
        for cid, model, w, h, params in cameras:
            f.write(struct.pack('<iiQQ', cid, MODEL_IDS[model], w, h) + struct.pack('<%dd' % len(params), *params))
    with open(os.path.join(sparse, 'images.bin'), 'wb') as f:
        f.write(struct.pack('<Q', len(images)))
        for iid, q, t, cid, name, obs in images:
            f.write(struct.pack('<i4d3di', iid, *(list(q) + list(t) + [cid])) + name.encode() + b'\0')
            f.write(struct.pack('<Q', len(obs)) + b''.join(struct.pack('<ddq', x, y, p) for x, y, p in obs))
    with open(os.path.join(sparse, 'points3D.bin'), 'wb') as f:
        f.write(struct.pack('<Q', len(points)))
        for pid, X, track in points:
            f.write(struct.pack('<Q3d3Bd', pid, X[0], X[1], X[2], 128, 64, 32, 0.5) + struct.pack('<Q', len(track)))
            f.write(b''.join(struct.pack('<ii', *o) for o in track))


def quat_rotation(q):
    """The closed-form rotation of the normalised quaternion (w, x, y, z) -- the formula of the issue, in float64."""
    q = np.asarray(q, np.float64)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)], -1),
                     np.stack([2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)], -1),
                     np.stack([2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)], -1)], -2)


def rotation_quat(R):
    """A unit quaternion (w, x, y, z) of the rotation matrix R (Shepperd's method)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q = (0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s)
    else:
        i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        v = [0.0, 0.0, 0.0]
        v[i] = 0.25 * s
        v[j] = (R[j, i] + R[i, j]) / s
        v[k] = (R[k, i] + R[i, k]) / s
        q = ((R[k, j] - R[j, k]) / s, v[0], v[1], v[2])
    return np.array(q)


def ranges_numpy(xyz, R, t, intr, size, p):
    """colmap_helpers.py:317-331 vectorised per image, in the arithmetic order c_k = ((R_k0 X + R_k1 Y) + R_k2 Z) + t_k,
    x = (c_0 / c_2) fx + cx, y = (c_1 / c_2) fy + cy, d = 1 / c_2 -> (n, d[int(n (1 - p))], d[int(n p)]) per image."""
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    ns, los, his = [], [], []
    with np.errstate(divide='ignore', invalid='ignore'):
        for k in range(len(R)):
            c = [((R[k, i, 0] * X + R[k, i, 1] * Y) + R[k, i, 2] * Z) + t[k, i] for i in range(3)]
            x = (c[0] / c[2]) * intr[k, 0] + intr[k, 2]
            y = (c[1] / c[2]) * intr[k, 1] + intr[k, 3]
            d = 1.0 / c[2]
            m = (x >= 0.0) & (x < size[k, 0]) & (y >= 0.0) & (y < size[k, 1]) & (d > 0.0)
            ds = np.sort(d[m])
            n = ds.shape[0]
            ns.append(n)
            los.append(ds[int(n * (1.0 - p))] if n else 0.0)
            his.append(ds[int(n * p)] if n else 0.0)
    return np.array(ns, np.int32), np.array(los, np.float64), np.array(his, np.float64)


def neighbours_restated(sets, keep, num):
    """generate_neighbor_list (colmap_helpers.py:341-371) on Python sets, its tie order pinned (stable argsort, reversed) and
    its fallback by scene index without self-listing, skipping left-out images -> pair.txt text."""
    N = len(sets)
    lines = []
    for r in range(N):
        if not keep[r]:
            continue
        shared = [0 if (j == r or not keep[j]) else len(sets[r] & sets[j]) for j in range(N)]
        lst = []
        for idx in np.argsort(np.array(shared), kind='stable')[::-1]:
            if shared[idx] == 0 or len(lst) == num:
                break
            lst.append((int(idx), shared[idx]))
        i = 1
        while len(lst) < num and i <= 10 * num:
            for j in (r + i, r - i):
                if len(lst) < num and 0 <= j < N and keep[j] and j != r and j not in [a for a, _ in lst]:
                    lst.append((j, 0))
            i += 1
        lines.append('%d\n%d%s\n' % (r, len(lst), ''.join(' %d %d' % s for s in lst)))
    return '%d\n' % len(lines) + ''.join(lines)
