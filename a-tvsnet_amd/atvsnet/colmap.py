"""COLMAP reconstruction -> the scene layout the drivers read (pair.txt, cams/%08d_cam.txt, images/%08d.jpg).

The test-time part of the reference's COLMAP path, gen_pipeline_mvs_list (the reference's atvsnet/preprocess_colmap.py:513-535):
ColmapSparse (colmap_helpers.py:255-371) reads the model, estimate_max_disparities gives each image a depth range,
generate_neighbor_list its source views, load_cam (preprocess_colmap.py:168-236) its camera.  Here:

    read_model        cameras / images / points3D in COLMAP's text or binary format (binary when cameras.bin exists), parsed by
                      content; PINHOLE and SIMPLE_PINHOLE cameras only (the output of `colmap image_undistorter`) unless
                      allow_distorted: then every model but FOV, each as the pinhole camera its images are undistorted into
                      (atvsnet/undistort.py)
    depth_ranges      ops.colmap_depth_range: every point projected into every image in float64, exact rank statistics
    covisibility      ops.colmap_covisibility: shared-point counts of every image pair from the tracks (CSR)
    select_sources    ranking by shared count (ties: higher scene index first), zero stops it, fallback around the reference
    make_scene        all of it, written for eval_pointcloud; from a sparse model and its image folder, the
                      images of distorted cameras are undistorted on the GPU on the way

Images are ordered by ascending image_id; an image's position in that order is its scene index (%08d).  numpy only: no
pyquaternion (R is the closed form of the normalised quaternion), and no Python loop per observation.
"""
from __future__ import print_function

import os
import shutil
import struct

import numpy as np

from .preprocess import write_cam

UNDISTORTED_MODELS = ('SIMPLE_PINHOLE', 'PINHOLE')
# COLMAP's camera model ids and parameter counts (src/colmap/sensor/models.h)
_MODELS = {0: ('SIMPLE_PINHOLE', 3), 1: ('PINHOLE', 4), 2: ('SIMPLE_RADIAL', 4), 3: ('RADIAL', 5), 4: ('OPENCV', 8),
           5: ('OPENCV_FISHEYE', 8), 6: ('FULL_OPENCV', 12), 7: ('FOV', 5), 8: ('SIMPLE_RADIAL_FISHEYE', 4), 9: ('RADIAL_FISHEYE', 5),
           10: ('THIN_PRISM_FISHEYE', 12)}


class Model(object):
    """A COLMAP model with its images in scene order (ascending image_id).

    image_ids (N,) int64, names [N], camera_ids (N,) int64, qvec (N,4) (w, x, y, z as stored), R (N,3,3), t (N,3) world to
    camera; intrinsics (N,4) fx, fy, cx, cy and size (N,2) width, height of each image's camera; xyz (P,3) of points3D in
    ascending POINT3D_ID order; tracks: offsets (T+1,) int32 and observers (offsets[-1],) int32, for every POINT3D_ID some
    image observes, the distinct scene indices observing it, ascending (PointList, colmap_helpers.py:18-27: -1 dropped, a
    point seen twice by one image counted once).

    read_model(allow_distorted=True) adds models [N] (the camera model's name), params [N] (its raw parameter tuple) and
    source_size (N,2) (the size of the image as taken); intrinsics and size are then those of the UNDISTORTED camera
    (undistort.undistorted_camera).  None otherwise."""
    __slots__ = ('image_ids', 'names', 'camera_ids', 'qvec', 'R', 't', 'intrinsics', 'size', 'xyz', 'offsets', 'observers',
                 'models', 'params', 'source_size')


def quaternion_to_rotation(q):
    """(..., 4) quaternions (w, x, y, z), any norm -> (..., 3, 3) rotation matrices of the normalised quaternions (float64)."""
    q = np.asarray(q, np.float64)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1.0 - 2.0 * (y * y + z * z)
    R[..., 0, 1] = 2.0 * (x * y - w * z)
    R[..., 0, 2] = 2.0 * (x * z + w * y)
    R[..., 1, 0] = 2.0 * (x * y + w * z)
    R[..., 1, 1] = 1.0 - 2.0 * (x * x + z * z)
    R[..., 1, 2] = 2.0 * (y * z - w * x)
    R[..., 2, 0] = 2.0 * (x * z - w * y)
    R[..., 2, 1] = 2.0 * (y * z + w * x)
    R[..., 2, 2] = 1.0 - 2.0 * (x * x + y * y)
    return R


def _camera(camera_id, model, width, height, params, undistort=None):
    """-> ((fx, fy, cx, cy), (width, height)[, model, params, (source width, source height)]); undistort: None, or the
    (blank_pixels, min_scale, max_scale) of allow_distorted."""
    if undistort is not None:
        from . import undistort as U
        if model not in U.PARAM_COUNT:
            raise ValueError('camera %d has the %s model: it is not undistorted here (FOV is out of scope); run `colmap '
                             'image_undistorter` on the reconstruction first and import its output folder' % (camera_id, model))
        p = tuple(float(v) for v in params)
        K, size = U.undistorted_camera(model, p, int(width), int(height), *undistort, camera='camera %d' % camera_id)
        return K, size, model, p, (int(width), int(height))
    if model not in UNDISTORTED_MODELS:
        raise ValueError('camera %d has the %s model: only PINHOLE and SIMPLE_PINHOLE cameras are read; run `colmap '
                         'image_undistorter` on the reconstruction first and import its output folder' % (camera_id, model))
    p = [float(v) for v in params]
    fx, fy, cx, cy = (p[0], p[0], p[1], p[2]) if model == 'SIMPLE_PINHOLE' else p[:4]
    return (fx, fy, cx, cy), (int(width), int(height))


def _content_lines(path):
    with open(path) as f:
        return [ln.rstrip('\r\n') for ln in f if not ln.lstrip().startswith('#')]


def _read_text(sparse, undistort=None):
    cameras = {}
    for ln in _content_lines(os.path.join(sparse, 'cameras.txt')):
        w = ln.split()
        if w:
            cameras[int(w[0])] = _camera(int(w[0]), w[1], w[2], w[3], w[4:], undistort)
    lines = _content_lines(os.path.join(sparse, 'images.txt'))
    images, i = [], 0
    while i < len(lines):
        w = lines[i].split(None, 9)
        i += 1
        if not w:                                        # blank lines between records; the points line after a header may be blank
            continue
        tok = lines[i].split() if i < len(lines) else []
        i += 1
        pid = np.array(tok[2::3], dtype=np.int64)
        images.append((int(w[0]), [float(v) for v in w[1:5]], [float(v) for v in w[5:8]], int(w[8]), w[9].strip(), pid))
    ids, xyz = [], []
    for ln in _content_lines(os.path.join(sparse, 'points3D.txt')):
        w = ln.split(None, 4)
        if w:
            ids.append(int(w[0]))
            xyz.append((float(w[1]), float(w[2]), float(w[3])))
    return cameras, images, np.array(ids, np.int64), np.array(xyz, np.float64).reshape(-1, 3)


def _read_binary(sparse, undistort=None):
    """COLMAP's binary model (src/colmap/scene/reconstruction_io.cc): little-endian, counts as uint64."""
    with open(os.path.join(sparse, 'cameras.bin'), 'rb') as f:
        buf = f.read()
    cameras, pos = {}, 8
    for _ in range(struct.unpack_from('<Q', buf, 0)[0]):
        cid, mid, width, height = struct.unpack_from('<iiQQ', buf, pos)
        pos += 24
        name, npar = _MODELS.get(mid, ('model id %d' % mid, None))
        if npar is None or (name not in UNDISTORTED_MODELS and (undistort is None or name == 'FOV')):
            _camera(cid, name, width, height, (), undistort)     # raises
        cameras[cid] = _camera(cid, name, width, height, struct.unpack_from('<%dd' % npar, buf, pos), undistort)
        pos += 8 * npar
    with open(os.path.join(sparse, 'images.bin'), 'rb') as f:
        buf = f.read()
    images, pos = [], 8
    obs = np.dtype([('x', '<f8'), ('y', '<f8'), ('id', '<i8')])
    for _ in range(struct.unpack_from('<Q', buf, 0)[0]):
        v = struct.unpack_from('<i7di', buf, pos)
        pos += 64
        end = buf.index(b'\0', pos)
        name = buf[pos:end].decode('utf-8')
        n2d = struct.unpack_from('<Q', buf, end + 1)[0]
        pos = end + 9
        pid = np.frombuffer(buf, obs, n2d, pos)['id'].astype(np.int64)
        pos += n2d * obs.itemsize
        images.append((v[0], list(v[1:5]), list(v[5:8]), v[8], name, pid))
    with open(os.path.join(sparse, 'points3D.bin'), 'rb') as f:
        buf = f.read()
    n = struct.unpack_from('<Q', buf, 0)[0]
    ids, xyz, pos = np.empty(n, np.int64), np.empty((n, 3), np.float64), 8
    head = struct.Struct('<Q3d3Bd')
    for k in range(n):
        r = head.unpack_from(buf, pos)
        ids[k], xyz[k] = r[0], r[1:4]
        track = struct.unpack_from('<Q', buf, pos + head.size)[0]
        pos += head.size + 8 + 8 * track
    return cameras, images, ids, xyz


def read_model(sparse, allow_distorted=False, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """<sparse>/{cameras,images,points3D}.bin, else .txt -> Model.  allow_distorted: cameras of COLMAP's distorted models (all
    but FOV) are read as the pinhole cameras undistort.undistorted_camera(blank_pixels, min_scale, max_scale) gives them -- what
    their images are resampled into -- and the Model carries models, params and source_size."""
    undistort = (blank_pixels, min_scale, max_scale) if allow_distorted else None
    binary = os.path.exists(os.path.join(sparse, 'cameras.bin'))
    for name in ('cameras', 'images', 'points3D'):
        path = os.path.join(sparse, name + ('.bin' if binary else '.txt'))
        if not os.path.exists(path):
            raise ValueError('%s does not exist: not a COLMAP sparse model folder' % path)
    cameras, images, point_ids, xyz = (_read_binary if binary else _read_text)(sparse, undistort)
    images.sort(key=lambda r: r[0])
    m = Model()
    m.image_ids = np.array([r[0] for r in images], np.int64)
    if len(np.unique(m.image_ids)) != len(m.image_ids):
        raise ValueError('%s: an IMAGE_ID appears twice' % sparse)
    m.names = [r[4] for r in images]
    m.camera_ids = np.array([r[3] for r in images], np.int64)
    missing = sorted(set(m.camera_ids.tolist()) - set(cameras))
    if missing:
        raise ValueError('%s: images refer to cameras %s that cameras.* does not list' % (sparse, missing[:5]))
    m.qvec = np.array([r[1] for r in images], np.float64).reshape(-1, 4)
    m.R = quaternion_to_rotation(m.qvec)
    m.t = np.array([r[2] for r in images], np.float64).reshape(-1, 3)
    m.intrinsics = np.array([cameras[c][0] for c in m.camera_ids.tolist()], np.float64).reshape(-1, 4)
    m.size = np.array([cameras[c][1] for c in m.camera_ids.tolist()], np.int64).reshape(-1, 2)
    m.models = m.params = m.source_size = None
    if allow_distorted:
        m.models = [cameras[c][2] for c in m.camera_ids.tolist()]
        m.params = [cameras[c][3] for c in m.camera_ids.tolist()]
        m.source_size = np.array([cameras[c][4] for c in m.camera_ids.tolist()], np.int64).reshape(-1, 2)
    order = np.argsort(point_ids, kind='stable')
    m.xyz = np.ascontiguousarray(xyz[order])
    m.offsets, m.observers = _tracks([r[5] for r in images])
    return m


def _tracks(point_ids_per_image):
    """POINT3D_IDs seen by each image (scene order) -> CSR (offsets, observers) of the distinct observing images per point id."""
    n = len(point_ids_per_image)
    pid = np.concatenate([np.asarray(p, np.int64) for p in point_ids_per_image]) if n else np.zeros(0, np.int64)
    img = np.repeat(np.arange(n, dtype=np.int64), [len(p) for p in point_ids_per_image])
    keep = pid != -1
    pid, img = pid[keep], img[keep]
    ids, inv = np.unique(pid, return_inverse=True)
    key = np.unique(inv.astype(np.int64) * max(n, 1) + img)          # distinct (point, image), sorted by point then image
    track, observer = key // max(n, 1), key % max(n, 1)
    offsets = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(np.bincount(track, minlength=len(ids)), out=offsets[1:])
    if offsets[-1] > 0x7fffffff:
        raise ValueError('%d observations: beyond the int32 track index' % offsets[-1])
    return offsets.astype(np.int32), observer.astype(np.int32)


def camera_rows(m):
    """(N,18) float64 per image: R row-major, t, fx, fy, cx, cy, width, height (atvs_colmap_depth_range's layout)."""
    return np.ascontiguousarray(np.concatenate([m.R.reshape(-1, 9), m.t, m.intrinsics, m.size.astype(np.float64)], 1))


def depth_ranges(m, percentile=0.99, device=None):
    """-> (n (N,) points in view, d_lo (N,), d_hi (N,)) numpy: the disparities of rank int(n * (1 - percentile)) and
    int(n * percentile) among each image's points in view (colmap_helpers.py:317-331 before its stretch)."""
    import torch
    from .. import ops
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    pts = torch.from_numpy(np.ascontiguousarray(m.xyz, np.float64)).to(dev)
    cams = torch.from_numpy(camera_rows(m)).to(dev)
    n, lo, hi = ops.colmap_depth_range(pts, cams, percentile)
    return n.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()


def covisibility(m, device=None):
    """(N,N) int32 numpy: the number of distinct 3-D points each pair of images shares (colmap_helpers.py:333-347)."""
    import torch
    from .. import ops
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    off = torch.from_numpy(m.offsets).to(dev)
    obs = torch.from_numpy(m.observers).to(dev)
    return ops.colmap_covisibility(off, obs, len(m.image_ids)).cpu().numpy()


def select_sources(shared, keep, num_neighbors):
    """shared (N,N) counts, keep (N,) bool (images in the scene) -> {ref: [(src, score), ...]} for every kept ref.
    generate_neighbor_list (colmap_helpers.py:341-371) with its order pinned: descending shared count, ties to the higher scene
    index first (np.argsort(kind='stable')[::-1]), stop at the first zero, at most num_neighbors; then, while short, r + i and
    r - i for i = 1 .. 10 * num_neighbors by SCENE INDEX, skipping the reference, images already listed and images left out
    (score 0)."""
    keep = np.asarray(keep, bool)
    N = len(keep)
    out = {}
    for r in np.flatnonzero(keep).tolist():
        counts = np.asarray(shared[r], np.int64).copy()
        counts[r] = 0
        counts[~keep] = 0
        chosen = []
        for j in np.argsort(counts, kind='stable')[::-1][:num_neighbors].tolist():
            if counts[j] == 0:
                break
            chosen.append((j, int(counts[j])))
        listed = set(j for j, _ in chosen) | {r}
        i = 1
        while len(chosen) < num_neighbors and i <= 10 * num_neighbors:
            for j in (r + i, r - i):
                if len(chosen) < num_neighbors and 0 <= j < N and keep[j] and j not in listed:
                    chosen.append((j, 0))
                    listed.add(j)
            i += 1
        out[r] = chosen
    return out


def pair_text(sources):
    """{ref: [(src, score)]} -> pair.txt: the count, then per reference `ref` and `n src score src score ...`."""
    text = '%d\n' % len(sources)
    for r in sorted(sources):
        text += '%d\n%d%s\n' % (r, len(sources[r]), ''.join(' %d %d' % s for s in sources[r]))
    return text


def scene_camera(R, t, intrinsics, d_lo, d_hi, max_d, stretch):
    """write_cam's (2,4,4) camera: [R | t], K, and the depth row (DEPTH_MIN, interval, max_d, DEPTH_MAX) of
    preprocess_colmap.load_cam:204-214 with max_disp = d_hi * stretch, min_disp = d_lo / stretch (colmap_helpers.py:329-331)."""
    cam = np.zeros((2, 4, 4))
    cam[0, :3, :3], cam[0, :3, 3], cam[0, 3, 3] = R, t, 1.0
    fx, fy, cx, cy = intrinsics
    cam[1, 0, 0], cam[1, 1, 1], cam[1, 0, 2], cam[1, 1, 2], cam[1, 2, 2] = fx, fy, cx, cy, 1.0
    max_disp, min_disp = d_hi * stretch, d_lo / stretch
    depth_min = 1.0 / float(max_disp)
    if (1.0 / float(min_disp)) <= depth_min:
        depth_interval = 0.02
        depth_max = depth_interval * float(max_d - 1) + depth_min
    else:
        depth_max = 1.0 / float(min_disp)
        depth_interval = (depth_max - depth_min) / float(max_d - 1)
    cam[1, 3] = (depth_min, depth_interval, max_d, depth_max)
    return cam


def _check_jpeg(path):
    if not os.path.splitext(path)[1].lower() in ('.jpg', '.jpeg'):
        raise ValueError('%s is not a JPEG: the scene layout stores images/%%08d.jpg and this importer copies bytes (no lossy '
                         're-encode); convert the images and rerun colmap image_undistorter' % path)
    with open(path, 'rb') as f:
        if f.read(3) != b'\xff\xd8\xff':
            raise ValueError('%s has a JPEG name but no JPEG signature' % path)


def _undistort_images(m, todo, srcs, out, jpeg_quality, workers, device):
    """Images `todo` (scene indices) of distorted cameras: decoded with PIL, warped on the GPU, written as images/%08d.jpg.  Decode
    and encode run on a pool of `workers` threads, at most that many images ahead of / behind the GPU, which sees one upload, one
    launch and one download per image (and one map launch per camera).  -> seconds spent in decode, gpu, encode (summed over
    the threads)."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from PIL import Image
    from . import undistort as U
    spent = dict(decode=0.0, gpu=0.0, encode=0.0)

    def decode(k):
        t0 = time.time()
        with Image.open(srcs[k]) as im:
            a = np.array(im.convert('RGB'))
        return a, time.time() - t0

    def encode(k, a):
        t0 = time.time()
        Image.fromarray(a).save(os.path.join(out, 'images', '%08d.jpg' % k), quality=jpeg_quality, subsampling=0)
        return time.time() - t0

    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    with ThreadPoolExecutor(workers) as pool, torch.cuda.device(dev):
        decoding = {k: pool.submit(decode, k) for k in todo[:workers]}
        encoding = []
        for i, k in enumerate(todo):
            a, dt = decoding.pop(k).result()
            spent['decode'] += dt
            if i + workers < len(todo):
                decoding[todo[i + workers]] = pool.submit(decode, todo[i + workers])
            t0 = time.time()
            K, size = tuple(m.intrinsics[k].tolist()), tuple(m.size[k].tolist())
            try:
                warped = U.undistort_image(a, m.models[k], m.params[k], int(m.source_size[k, 0]), int(m.source_size[k, 1]), (K, size))
            except ValueError as e:
                raise ValueError('%s: %s' % (srcs[k], e))
            spent['gpu'] += time.time() - t0
            encoding.append(pool.submit(encode, k, warped))
            if len(encoding) > workers:
                spent['encode'] += encoding.pop(0).result()
        for f in encoding:
            spent['encode'] += f.result()
    return spent


def make_scene(dense_folder, out, max_d=128, num_neighbors=10, percentile=0.99, stretch=1.33333, link=False, device=None,
               sparse=None, image_path=None, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, jpeg_quality=100, workers=16):
    """<dense_folder> (sparse/ + images/, the output of `colmap image_undistorter`), or, with dense_folder None, a sparse model
    `sparse` of any camera models but FOV and its images under `image_path` -> <out>/{cams/%08d_cam.txt, images/%08d.jpg,
    pair.txt, colmap_images.txt}.  Images of pinhole cameras are copied (or linked); images of distorted cameras are undistorted
    on the GPU into the camera undistort.undistorted_camera(blank_pixels, min_scale, max_scale) gives, which cams/ then holds,
    and written as JPEG of `jpeg_quality` without chroma subsampling.  Images with no point in view are left out (reported) but
    keep their scene index.  -> dict(model, n, d_lo, d_hi, shared, sources, skipped, undistorted, seconds)."""
    if max_d < 2:
        raise ValueError('max_d must be at least 2, got %d' % max_d)
    if (dense_folder is None) == (sparse is None and image_path is None) or (sparse is None) != (image_path is None):
        raise ValueError('give either dense_folder, or sparse and image_path')
    if not 1 <= jpeg_quality <= 100:
        raise ValueError('jpeg_quality must lie in [1, 100], got %r' % jpeg_quality)
    workers = min(max(int(workers), 1), 16)
    if dense_folder is not None:
        m = read_model(os.path.join(dense_folder, 'sparse'))
        image_path = os.path.join(dense_folder, 'images')
    else:
        m = read_model(sparse, True, blank_pixels, min_scale, max_scale)
        dense_folder = sparse
    if len(m.image_ids) == 0:
        raise ValueError('%s: the model has no images' % dense_folder)
    srcs = [os.path.join(image_path, name) for name in m.names]
    distorted = [m.models is not None and m.models[k] not in UNDISTORTED_MODELS for k in range(len(srcs))]
    if link and any(distorted):
        raise ValueError('%s has cameras of distorted models: their images are resampled, not linked (drop --link)' % dense_folder)
    for p, d in zip(srcs, distorted):
        if d and not os.path.isfile(p):
            raise ValueError('%s does not exist' % p)
        if not d:
            _check_jpeg(p)
    n, d_lo, d_hi = depth_ranges(m, percentile, device)
    keep = n > 0
    skipped = np.flatnonzero(~keep).tolist()
    for k in skipped:
        print('colmap import: image %08d (IMAGE_ID %d, %s) has no 3-D point in view: left out of the scene' %
              (k, m.image_ids[k], m.names[k]))
    shared = covisibility(m, device)
    sources = select_sources(shared, keep, num_neighbors)
    os.makedirs(os.path.join(out, 'cams'), exist_ok=True)
    os.makedirs(os.path.join(out, 'images'), exist_ok=True)
    for k in np.flatnonzero(keep).tolist():
        write_cam(os.path.join(out, 'cams', '%08d_cam.txt' % k),
                  scene_camera(m.R[k], m.t[k], m.intrinsics[k], d_lo[k], d_hi[k], max_d, stretch))
        dst = os.path.join(out, 'images', '%08d.jpg' % k)
        if os.path.lexists(dst):
            os.remove(dst)
        if distorted[k]:
            continue
        if link:
            os.symlink(os.path.abspath(srcs[k]), dst)
        else:
            shutil.copyfile(srcs[k], dst)
    todo = [k for k in np.flatnonzero(keep).tolist() if distorted[k]]
    seconds = _undistort_images(m, todo, srcs, out, jpeg_quality, workers, device) if todo else dict(decode=0.0, gpu=0.0, encode=0.0)
    with open(os.path.join(out, 'pair.txt'), 'w') as f:
        f.write(pair_text(sources))
    with open(os.path.join(out, 'colmap_images.txt'), 'w') as f:
        f.write('# scene index, COLMAP IMAGE_ID, NAME; images with no 3-D point in view are commented out\n')
        for k in range(len(m.image_ids)):
            f.write('%s%08d %d %s\n' % ('' if keep[k] else '# ', k, m.image_ids[k], m.names[k]))
    return dict(model=m, n=n, d_lo=d_lo, d_hi=d_hi, shared=shared, sources=sources, skipped=skipped, undistorted=todo,
                seconds=seconds)
