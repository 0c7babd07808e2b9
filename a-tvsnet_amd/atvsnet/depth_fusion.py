#!/usr/bin/env python
"""Depth-map filtering and fusion into a point cloud, mirroring the reference's ``atvsnet/depth_fusion.py`` (CLI, file
layout, function names) with the external ``fusibile`` executable replaced by the HIP kernel behind
``atvs_fusibile`` (include/atvsnet_hip.h; reference fusibile/fusibile.cu:138-277, host side fusibile/main.cpp:559-845).

    python -m atvsnet_amd.atvsnet.depth_fusion --dense_folder <scene> [--prob_threshold 0.8]
        [--disp_threshold 0.01] [--num_consistent 2]
        [--normals {fake,depth}] [--normal_threshold DEG] [--normal_step S] [--normal_depth_gate G]

reads  <dense_folder>/depths_atvsnet/{%08d.pfm, %08d_prob.pfm, %08d.jpg, %08d.txt}   (written by eval_pointcloud)
writes <dense_folder>/depths_atvsnet/%08d_prob_filtered.pfm                          (probability_filter, :185-206)
       <dense_folder>/points_atvsnet/{cams/*.P, images/*.jpg, 2333__%08d/{disp,normals}.dmb}   (atvsnet_to_gipuma, :115-182)
       <dense_folder>/points_atvsnet/consistencyCheck-<date>-<time>/final3d_model.ply          (fusibile main.cpp:600-604, 838-842)
       <dense_folder>/final3d_model.ply                                              (:262-267)

The gipuma-format intermediate files are kept (same bytes as the reference writes) so that either fusion back-end can
consume them; ``--fusibile_exe_path`` is accepted and ignored.

``--normals depth`` (not in the reference, whose normals are fake_colmap_normal's constant): every normals.dmb is estimated from
its disp.dmb and camera on the MI355X (atvs_depth_normals_f32), the fusion's normal test runs with
``--normal_threshold`` degrees (default 30) instead of 360, and the PLY carries the unit normal of every point.
"""
from __future__ import print_function

import argparse
import io
import os
import shutil
import time

import numpy as np

from .preprocess import cam_text, load_cam, load_pfm, write_pfm
from ..tools import ply


_DMB_HEADER = np.dtype([('type', '<i4'), ('height', '<i4'), ('width', '<i4'), ('channels', '<i4')])


def read_gipuma_dmb(path):
    """Gipuma .dmb image -> (h, w) or (h, w, c) float32 (reference :24-35).  File = 16-byte header
    (int32 type, height, width, channels) + float32 channel PLANES, each plane row-major (h, w)."""
    raw = np.fromfile(path, dtype=np.uint8)
    head = raw[:_DMB_HEADER.itemsize].view(_DMB_HEADER)[0]
    h, w, c = int(head['height']), int(head['width']), int(head['channels'])
    planes = raw[_DMB_HEADER.itemsize:].view('<f4').reshape(c, h, w)
    return np.moveaxis(planes, 0, -1).squeeze()


def write_gipuma_dmb(path, image):
    """(h, w) or (h, w, c) -> Gipuma .dmb (reference :37-58): header with type = 1, then the channel planes."""
    image = np.asarray(image, np.float32)
    planes = image[None] if image.ndim == 2 else np.moveaxis(image, -1, 0)
    head = np.zeros(1, _DMB_HEADER)
    head['type'], head['height'], head['width'], head['channels'] = (1,) + planes.shape[1:] + planes.shape[:1]
    with open(path, 'wb') as fid:
        fid.write(head.tobytes())
        fid.write(np.ascontiguousarray(planes, '<f4').tobytes())


def atvsnet_to_gipuma_dmb(in_path, out_path):
    '''convert atvsnet .pfm output to Gipuma .dmb format (reference :60-68; also saves a viridis .png)'''
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as matplt
    with open(in_path, 'rb') as f:
        image = load_pfm(f)
    matplt.imsave(out_path[0:-4] + '.png', np.squeeze(image), cmap='viridis')
    write_gipuma_dmb(out_path, image)


def projection_matrix(cam):
    '''P = (K with its fourth row zeroed) @ extrinsic, first three rows (reference :75-83)'''
    extrinsic = np.array(cam[0], dtype=np.float64)
    intrinsic = np.array(cam[1], dtype=np.float64)
    intrinsic[3, :] = 0
    return np.matmul(intrinsic, extrinsic)[0:3]


def atvsnet_to_gipuma_cam(in_path, out_path):
    '''convert atvsnet camera to gipuma camera format (reference :70-93): 3 rows of `str(value) ` + blank line'''
    with open(in_path) as f:
        cam = load_cam(f)
    P = projection_matrix(cam)
    with open(out_path, "w") as f:
        for i in range(0, 3):
            for j in range(0, 4):
                f.write(str(P[i][j]) + ' ')
            f.write('\n')
        f.write('\n')


def fake_colmap_normal(in_depth_path, out_normal_path):
    '''(1,1,1)/sqrt(3) normals where the depth is positive, 0 elsewhere (reference :95-113)'''
    depth_image = read_gipuma_dmb(in_depth_path)
    h, w = depth_image.shape[:2]
    normal_image = np.ones((h, w, 3), np.float32) / 1.732050808
    mask = (depth_image > 0).astype(np.float32).reshape(h, w, 1)
    write_gipuma_dmb(out_normal_path, np.float32(normal_image * mask))


NORMAL_SOURCES = ('fake', 'depth')
# --normals depth: the default normal threshold in degrees.  fusibile's own default neighbourhood (0.52 rad,
# algorithmparameters.h:89), a default and not a measurement.
DEPTH_NORMAL_THRESHOLD_DEG = 30.0


def check_normal_options(normals='fake', normal_threshold=None, normal_step=1, normal_depth_gate=0.02):
    """The normal options of SceneFusion / main, checked before any launch -> (normals, threshold in degrees, step, gate).
    normal_threshold None: 360 (the reference's: the test rejects nothing) with 'fake', DEPTH_NORMAL_THRESHOLD_DEG with 'depth'."""
    if normals not in NORMAL_SOURCES:
        raise ValueError('normals must be one of %s, got %r' % (', '.join(NORMAL_SOURCES), normals))
    if normal_threshold is None:
        normal_threshold = 360.0 if normals == 'fake' else DEPTH_NORMAL_THRESHOLD_DEG
    normal_threshold = float(normal_threshold)
    if not (0.0 < normal_threshold <= 360.0):
        raise ValueError('normal_threshold must be in (0, 360] degrees, got %r' % (normal_threshold,))
    if int(normal_step) != normal_step or int(normal_step) < 1:
        raise ValueError('normal_step must be an integer >= 1, got %r' % (normal_step,))
    normal_depth_gate = float(normal_depth_gate)
    if not (0.0 <= normal_depth_gate < float('inf')):
        raise ValueError('normal_depth_gate must be >= 0 and finite, got %r' % (normal_depth_gate,))
    return normals, normal_threshold, int(normal_step), normal_depth_gate


def normal_threshold_radians(degrees):
    """fusibile's --normal_thresh=<degrees> as it reaches the kernel (main.cpp:346-348): the float it scans, times pi / 180 in
    double (rounded to float32 where it is passed on)."""
    return float(np.float32(degrees)) * np.pi / 180.0


def unit_normals(normals):
    """(M,3) averaged normals of the fusion -> (M,3) float32 unit normals: the float64 norm, one division, one cast; a zero (or
    non-finite) normal stays as it is.  The one place both pipelines restore unit length."""
    n = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all='ignore'):
        length = np.sqrt((n * n).sum(-1, keepdims=True))
        return np.where(length > 0, n / length, n).astype(np.float32)


def depth_normal(in_depth_path, in_p_path, out_normal_path, normal_step=1, normal_depth_gate=0.02, device=None):
    """normals.dmb of one map from its disp.dmb and its .P camera on the MI355X (atvs_depth_normals_f32): what
    SceneFusion(normals='depth') computes for the map's slot of the slab."""
    import torch
    from .. import ops
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    depth = np.asarray(read_gipuma_dmb(in_depth_path), np.float32)
    depth = depth.reshape(depth.shape[:2])
    nd = np.zeros((1,) + depth.shape + (4,), np.float32)
    nd[0, ..., 3] = depth
    cams = torch.from_numpy(pack_cameras([read_p_file(in_p_path)])).to(dev)
    out = ops.depth_normals(cams, torch.from_numpy(nd).to(dev), normal_step, normal_depth_gate)
    write_gipuma_dmb(out_normal_path, out[0, ..., :3].cpu().numpy())


def atvsnet_to_gipuma(dense_folder, gipuma_point_folder, normals='fake', normal_step=1, normal_depth_gate=0.02):
    '''(reference :115-182)  normals='depth': normals.dmb from the map and its camera (depth_normal) instead of fake_colmap_normal'''
    depth_folder = os.path.join(dense_folder, 'depths_atvsnet')
    gipuma_cam_folder = os.path.join(gipuma_point_folder, 'cams')
    gipuma_image_folder = os.path.join(gipuma_point_folder, 'images')
    for d in (gipuma_point_folder, gipuma_cam_folder, gipuma_image_folder):
        if not os.path.isdir(d):
            os.mkdir(d)
    image_names = sorted(os.listdir(depth_folder))
    for image_name in image_names:
        if not ('jpg' in image_name or 'png' in image_name):
            continue
        image_prefix = os.path.splitext(image_name)[0]
        in_cam_file = os.path.join(depth_folder, image_prefix + '.txt')
        atvsnet_to_gipuma_cam(in_cam_file, os.path.join(gipuma_cam_folder, image_name + '.P'))
        with open(in_cam_file) as f:
            cam = load_cam(f)
        intrinsic = np.array(cam[1])
        intrinsic[3, :] = 0
        np.save(os.path.join(gipuma_cam_folder, image_name[:-4] + '_intr.npy'), intrinsic)
        np.save(os.path.join(gipuma_cam_folder, image_name[:-4] + '_extr.npy'), np.array(cam[0]))
        np.save(os.path.join(gipuma_cam_folder, image_name[:-4] + '_proj.npy'), projection_matrix(cam))
    for image_name in image_names:
        if 'jpg' not in image_name:
            continue
        shutil.copy(os.path.join(depth_folder, image_name), os.path.join(gipuma_image_folder, image_name))
    gipuma_prefix = '2333__'
    for image_name in image_names:
        if not ('jpg' in image_name or 'png' in image_name):
            continue
        image_prefix = os.path.splitext(image_name)[0]
        sub_depth_folder = os.path.join(gipuma_point_folder, gipuma_prefix + image_prefix)
        if not os.path.isdir(sub_depth_folder):
            os.mkdir(sub_depth_folder)
        in_depth_pfm = os.path.join(depth_folder, image_prefix + '_prob_filtered.pfm')
        out_depth_dmb = os.path.join(sub_depth_folder, 'disp.dmb')
        atvsnet_to_gipuma_dmb(in_depth_pfm, out_depth_dmb)
        out_normal_dmb = os.path.join(sub_depth_folder, 'normals.dmb')
        if normals == 'depth':
            depth_normal(out_depth_dmb, os.path.join(gipuma_cam_folder, image_name + '.P'), out_normal_dmb, normal_step,
                         normal_depth_gate)
        else:
            fake_colmap_normal(out_depth_dmb, out_normal_dmb)


def probability_filter(dense_folder, prob_threshold):
    '''depth := 0 where the probability map is under the threshold (reference :185-206)'''
    depth_folder = os.path.join(dense_folder, 'depths_atvsnet')
    for image_name in sorted(os.listdir(depth_folder)):
        if not ('jpg' in image_name or 'png' in image_name):
            continue
        image_prefix = os.path.splitext(image_name)[0]
        with open(os.path.join(depth_folder, image_prefix + '.pfm'), 'rb') as f:
            depth_map = load_pfm(f)
        with open(os.path.join(depth_folder, image_prefix + '_prob.pfm'), 'rb') as f:
            prob_map = load_pfm(f)
        depth_map = np.array(depth_map)
        depth_map[prob_map < prob_threshold] = 0
        write_pfm(os.path.join(depth_folder, image_prefix + '_prob_filtered.pfm'), depth_map)


# --------------------------------------------------------------------------- the fusibile executable, in process

def _rq(M):
    """M = K R, K upper triangular with a positive diagonal (cv::RQDecomp3x3 as decomposeProjectionMatrix uses it)."""
    Q, U = np.linalg.qr(np.flipud(M).T)
    K = np.flipud(np.fliplr(U.T))
    R = np.flipud(Q.T)
    S = np.diag(np.sign(np.diag(K)))
    return K @ S, S @ R


def pack_cameras(Ps):
    """(N,28) float32 per camera: P[12] | M_inv[9] | C[3] | P_col34[3] | f -- the fields of Camera_cu the kernel reads
    (fusibile/cameraGeometryUtils.h:377-433 with transformP = false, cam_scale = 1): P as read from the .P file,
    M_inv = inverse of its left 3x3, C = camera centre from the signed minors of P (:20-50), f = K[0,0] of its RQ
    decomposition."""
    out = np.zeros((len(Ps), 28), np.float32)
    for i, P in enumerate(Ps):
        P32 = np.asarray(P, np.float32).reshape(3, 4)
        P64 = P32.astype(np.float64)
        K, _ = _rq(P64[:, :3])
        det = lambda cols: np.linalg.det(P64[:, cols])      # noqa: E731
        C4 = np.array([det([1, 2, 3]), -det([0, 2, 3]), det([0, 1, 3]), -det([0, 1, 2])])
        out[i, 0:12] = P32.reshape(12)
        out[i, 12:21] = np.linalg.inv(P64[:, :3]).astype(np.float32).reshape(9)
        out[i, 21:24] = (C4[:3] / C4[3]).astype(np.float32)
        out[i, 24:27] = P32[:, 3]
        out[i, 27] = np.float32(K[0, 0] / K[2, 2])
    return out


def read_p_file(path):
    """3x4 projection matrix of a gipuma .P file (whitespace-separated, fusibile/fileIoUtils.h readPFileStrechaPmvs)."""
    with open(path) as f:
        vals = [float(v) for v in f.read().split()]
    return np.array(vals[:12], np.float64).reshape(3, 4)


def fuse_views(Ps, depths, normals, images_bgr, disp_thresh, normal_thresh, num_consistent, device=None, return_normals=False):
    """runcuda + copy_point_cloud_to_host (fusibile/fusibile.cu:279-325, 422-427) on the MI355X: every camera in turn
    is the reference of one atvs_fusibile launch; its created points whose three coordinates are all non-zero are
    appended (camera-major, row-major).  -> (points (M,3) float32, colors (M,3) uint8 r,g,b); return_normals: and the kernel's
    averaged (not normalised) normal of every point, (M,3) float32."""
    import torch
    from .. import ops
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    cams = torch.from_numpy(pack_cameras(Ps)).to(dev)
    nd = np.concatenate([np.asarray(normals, np.float32), np.asarray(depths, np.float32)[..., None]], -1)
    img = np.asarray(images_bgr)
    img4 = np.concatenate([img.astype(np.float32), np.zeros(img.shape[:3] + (1,), np.float32)], -1)
    nd_d, img_d = torch.from_numpy(np.ascontiguousarray(nd)).to(dev), torch.from_numpy(np.ascontiguousarray(img4)).to(dev)
    pts, cols, nrms = [], [], []
    for ref in range(len(Ps)):
        coord, normal, tex, created = ops.fusibile(cams, nd_d, img_d, ref, float(disp_thresh), float(normal_thresh),
                                              int(num_consistent))
        X = coord[..., :3]
        keep = (created > 0) & (X[..., 0] != 0) & (X[..., 1] != 0) & (X[..., 2] != 0)
        pts.append(X[keep].cpu().numpy())
        if return_normals:
            nrms.append(normal[..., :3][keep].cpu().numpy())
        t = tex[keep].cpu().numpy()
        # (char)(int) of channels 2, 1, 0 of the averaged texture (fusibile/displayUtils.h:109-111)
        cols.append(np.stack([t[:, 2], t[:, 1], t[:, 0]], -1).astype(np.int32).astype(np.uint8))
    if return_normals:
        return np.concatenate(pts, 0), np.concatenate(cols, 0), np.concatenate(nrms, 0)
    return np.concatenate(pts, 0), np.concatenate(cols, 0)


# depth_map_fusion's normal threshold: 360 degrees, in radians as it passes it to fuse_views
NORMAL_THRESHOLD = 360 * np.pi / 180.0


def camera_row(cam):
    """The 28 floats fuse_views packs for a camera that eval_pointcloud writes with write_cam, derived the way the file pipeline
    derives them -- write_cam's text, load_cam, projection_matrix, the .P file (str() of each float64 value, which float() reads
    back exactly) and pack_cameras -- in memory."""
    return pack_cameras([projection_matrix(load_cam(io.StringIO(cam_text(cam))))])[0]


def _plane(t, what):
    """A depth / probability map as (rows, cols): the network's (1, rows, cols, 1) or any squeezable form of it."""
    while t.ndim > 2 and t.shape[0] == 1:
        t = t[0]
    while t.ndim > 2 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.ndim != 2:
        raise ValueError('SceneFusion.add: %s must be a (rows, cols) map, got shape %s' % (what, tuple(t.shape)))
    return t


class SceneFusion(object):
    """The point-cloud stage of a scene on the device, without the files: every depth map is staged into a scene-resident slab as
    it is finished (`add`, atvs_fusion_stage_f32: the inverse-depth step of eth3d_maps._write_map, probability_filter and
    fake_colmap_normal), and `run` fuses all reference cameras in one pass (atvs_fusibile_scene) into the points and colours
    fuse_views computes on the same maps, in the same order.  The cameras are ordered by `out_index` ascending, as the sorted
    2333__%08d folders of depth_map_fusion order them.

        fusion = SceneFusion(len(maps), rows, cols, device)
        fusion.add(out_index, depth, prob, image_bgr_u8, cam)          # per map, any order
        fusion.write_ply(path)                                         # = run() + tools/ply.write_ply

    depth, prob: the network's outputs (host numpy or device tensors, any squeezable form of (rows, cols)); image_bgr_u8: the
    1/4-scale reference image (rows, cols, 3) uint8; cam: the (2,4,4) camera eval_pointcloud writes with write_cam.  `stream`:
    the stream the staging is enqueued on (default: the current one); run() orders itself after every staging.

    normals='depth' (default 'fake': the file pipeline's constant normal and its 360 degree threshold, which rejects nothing):
    run() first estimates the normals of the staged slab from its depth planes (atvs_depth_normals_f32 with normal_step and
    normal_depth_gate), fuses with normal_threshold degrees (default DEPTH_NORMAL_THRESHOLD_DEG) and keeps the
    unit normal of every point for normals() and write_ply -- depth_fusion.main --normals depth on the same maps."""

    def __init__(self, n_maps, rows, cols, device=None, prob_threshold=0.8, disp_threshold=0.01, num_consistent=2,
                 inverse_depth=None, normals='fake', normal_threshold=None, normal_step=1, normal_depth_gate=0.02):
        import torch
        from ..flags import FLAGS
        self.normal_source, self.normal_threshold, self.normal_step, self.normal_depth_gate = check_normal_options(
            normals, normal_threshold, normal_step, normal_depth_gate)
        for name, v in (('n_maps', n_maps), ('rows', rows), ('cols', cols)):
            if int(v) != v or int(v) <= 0:
                raise ValueError('SceneFusion: %s must be a positive integer, got %r' % (name, v))
        self.n_maps, self.rows, self.cols = int(n_maps), int(rows), int(cols)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type not in ('cuda', 'meta'):         # meta: the host code alone (shape checks, camera order), no launch
            raise RuntimeError('SceneFusion runs on the MI355X only (no CPU fallback), got device %s' % self.device)
        self.prob_threshold, self.disp_threshold = float(prob_threshold), float(disp_threshold)
        self.num_consistent = int(num_consistent)
        self.inverse_depth = FLAGS.inverse_depth if inverse_depth is None else bool(inverse_depth)
        shape = (self.n_maps, self.rows, self.cols, 4)
        self.nd = torch.empty(shape, dtype=torch.float32, device=self.device)
        self.img = torch.empty(shape, dtype=torch.float32, device=self.device)
        self.cams = np.zeros((self.n_maps, 28), np.float32)
        self.index, self.events = [], []          # out_index and staging event of each slot, in add() order
        self.result = self.result_normals = None

    def _check_size(self, what, shape, want):
        if tuple(int(s) for s in shape) != want:
            raise RuntimeError('depth maps %s and %s %s differ in size: one scene fuses maps of one size'
                               % ((self.rows, self.cols), what, tuple(int(s) for s in shape)))

    def add(self, out_index, depth, prob, image_bgr_u8, cam, stream=None):
        import torch
        from .. import ops
        out_index = int(out_index)
        if len(self.index) == self.n_maps:
            raise ValueError('SceneFusion.add: all %d slots are taken' % self.n_maps)
        if out_index in self.index:
            raise ValueError('SceneFusion.add: map %d was added before' % out_index)
        depth, prob = _plane(depth, 'depth'), _plane(prob, 'prob')
        self._check_size('depth map', depth.shape, (self.rows, self.cols))
        self._check_size('probability map', prob.shape, (self.rows, self.cols))
        self._check_size('image', tuple(image_bgr_u8.shape)[:2], (self.rows, self.cols))
        row = camera_row(cam)
        slot = len(self.index)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device) if isinstance(a, np.ndarray) else a    # noqa: E731
        stage = lambda: ops.fusion_stage(up(depth), up(prob), up(image_bgr_u8), self.inverse_depth, self.prob_threshold,  # noqa: E731
                                         self.nd[slot], self.img[slot])
        ev = None
        if self.device.type == 'meta':
            stage()
        else:
            st = torch.cuda.current_stream(self.device) if stream is None else stream
            with torch.cuda.stream(st):
                stage()
                ev = torch.cuda.Event()
                ev.record(st)
        self.cams[slot] = row
        self.index.append(out_index)
        self.events.append(ev)
        self.result = self.result_normals = None

    def order(self):
        """The slots in fusion order: by out_index ascending."""
        return np.argsort(np.asarray(self.index, np.int64), kind='stable')

    def run(self):
        """-> (points (M,3) float32, colors (M,3) uint8 r,g,b) as numpy arrays: fuse_views of the staged maps."""
        import torch
        from .. import ops
        k = len(self.index)
        if k == 0:
            raise RuntimeError('SceneFusion.run: no depth map was added')
        if self.result is None:
            cur = torch.cuda.current_stream(self.device)
            for ev in self.events:
                cur.wait_event(ev)
            order = self.order()
            nd, img = self.nd[:k], self.img[:k]
            depth = self.normal_source == 'depth'
            if depth:            # in slot order, in place: only the normal floats change, the staged depth planes stay
                ops.depth_normals(torch.from_numpy(np.ascontiguousarray(self.cams[:k])).to(self.device), nd, self.normal_step,
                                  self.normal_depth_gate)
            if not np.array_equal(order, np.arange(k)):
                idx = torch.from_numpy(order).to(self.device)
                nd, img = nd.index_select(0, idx), img.index_select(0, idx)
            cams = torch.from_numpy(np.ascontiguousarray(self.cams[:k][order])).to(self.device)
            out = ops.fusibile_scene(cams, nd, img, self.disp_threshold, normal_threshold_radians(self.normal_threshold),
                                     self.num_consistent, with_normals=depth)
            self.result = (out[0].cpu().numpy(), out[1].cpu().numpy())
            self.result_normals = unit_normals(out[2].cpu().numpy()) if depth else None
        return self.result

    def support(self, want=('count', 'depth', 'weight')):
        """run(), then the fusion's agreement count of every staged pixel under the scene's own disp_threshold, num_consistent and
        normal options (ops.fusion_support, one launch) -> a dict of device tensors, each (k,rows,cols) in fusion order (order()):
        count int32, depth float32 (the staged depth where count >= num_consistent, 0 elsewhere: the plane as the fusion masks its
        points), weight float32 ((1 + count) / (1 + num_consistent)).  It comes after run(), so with normals='depth' the slab already
        carries the estimated normals and their threshold applies."""
        import torch
        from .. import ops
        self.run()
        k = len(self.index)
        order = self.order()
        nd = self.nd[:k]
        if not np.array_equal(order, np.arange(k)):
            nd = nd.index_select(0, torch.from_numpy(order).to(self.device))
        cams = torch.from_numpy(np.ascontiguousarray(self.cams[:k][order])).to(self.device)
        return ops.fusion_support(cams, nd, self.disp_threshold, normal_threshold_radians(self.normal_threshold), self.num_consistent,
                                  want=want)

    def normals(self):
        """-> (M,3) float32: the unit normal of every point of run() (the fusion's average over the agreeing views, brought back to
        unit length by unit_normals; a zero normal stays zero).  normals='depth' only."""
        if self.normal_source != 'depth':
            raise RuntimeError("SceneFusion.normals: the scene is fused with normals='fake', there are no normals to return")
        self.run()
        return self.result_normals

    def write_ply(self, path):
        """run() into a binary PLY at `path` (the layout depth_fusion.main copies to <dense_folder>/final3d_model.ply; with
        normals='depth' every vertex carries its normal)."""
        pts, cols = self.run()
        ply.write_ply(path, pts, cols, self.result_normals)
        return len(pts)


def _imread_bgr(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))[:, :, ::-1].copy()


def depth_map_fusion(point_folder, fusibile_exe_path, disp_thresh, num_consistent, normal_thresh=360, ply_normals=False):
    '''(reference :209-231 + fusibile/main.cpp:559-845) fuses the gipuma-format folder on the MI355X and writes
    <point_folder>/consistencyCheck-<date>-<time>/final3d_model.ply.  normal_thresh: degrees, 360 as the reference passes it
    (:216); ply_normals: the PLY carries the unit normal of every point (unit_normals of the fusion's average).'''
    cam_folder = os.path.join(point_folder, 'cams')
    image_folder = os.path.join(point_folder, 'images')
    # sub-folders `<prefix>__<id>` whose name starts with '2' and has two underscores (main.cpp:619-649), sorted
    ids = []
    for sub in sorted(os.listdir(point_folder)):
        if not os.path.isdir(os.path.join(point_folder, sub)) or sub.count('_') < 2 or sub[0] != '2':
            continue
        first = sub.find('_') + 1
        ident = sub[first + sub[first:].find('_') + 1:]
        for ext in ('.png', '.jpg', '.ppm'):
            if os.path.exists(os.path.join(image_folder, ident + ext)):
                ids.append((sub, ident, ident + ext))
                break
    if not ids:
        raise RuntimeError('%s: no gipuma depth folders with matching images' % point_folder)
    Ps = [read_p_file(os.path.join(cam_folder, name + '.P')) for _, _, name in ids]
    images = np.stack([_imread_bgr(os.path.join(image_folder, name)) for _, _, name in ids], 0)
    depths = np.stack([read_gipuma_dmb(os.path.join(point_folder, sub, 'disp.dmb')) for sub, _, _ in ids], 0)
    normals = np.stack([read_gipuma_dmb(os.path.join(point_folder, sub, 'normals.dmb')) for sub, _, _ in ids], 0)
    if depths.shape[1:3] != images.shape[1:3]:
        raise RuntimeError('depth maps %s and images %s differ in size' % (depths.shape[1:3], images.shape[1:3]))
    fused = fuse_views(Ps, depths, normals, images, disp_thresh, normal_threshold_radians(normal_thresh), int(num_consistent),
                       return_normals=ply_normals)
    pts, cols = fused[:2]
    out = os.path.join(point_folder, 'consistencyCheck-' + time.strftime('%Y%m%d-%H%M%S'))
    os.makedirs(out, exist_ok=True)
    print('Found %.2f million points' % (len(pts) / 1e6))
    ply.write_ply(os.path.join(out, 'final3d_model.ply'), pts, cols, unit_normals(fused[2]) if ply_normals else None)
    return out


def add_options(parser, prefix='', defaults=True):
    """The normal options, named --<prefix>normals, --<prefix>normal_threshold, --<prefix>normal_step, --<prefix>normal_depth_gate.
    defaults: this tool's form, where normals, normal_step and normal_depth_gate default to check_normal_options' own; False: the
    ETH3D driver's (prefix 'fuse_'), where every one defaults to None and only what is given is passed on."""
    parser.add_argument('--%snormals' % prefix, choices=NORMAL_SOURCES, default='fake' if defaults else None,
                        help='fake (the default): the constant normal of the reference; depth: estimated from each depth map on the '
                             'GPU, tested in the fusion and written into the PLY')
    parser.add_argument('--%snormal_threshold' % prefix, type=float, default=None, metavar='DEG',
                        help='largest angle between the normals of two agreeing views (default: 360 with normals fake, %g with '
                             'normals depth)' % DEPTH_NORMAL_THRESHOLD_DEG)
    parser.add_argument('--%snormal_step' % prefix, type=int, default=1 if defaults else None, metavar='S',
                        help='normals depth: pixel distance of the neighbours (default 1)')
    parser.add_argument('--%snormal_depth_gate' % prefix, type=float, default=0.02 if defaults else None, metavar='G',
                        help='normals depth: a neighbour counts when its depth is within G * depth (default 0.02)')


def options(parser, args, prefix=''):
    """The options of add_options that were given, as SceneFusion's / check_normal_options' keyword arguments ({} when none was); a bad
    one is an argument error.  parser None: nothing is checked, and an option `args` lacks is not given.  This is the ETH3D driver's
    fuse_normals (with fuse only): with normals='depth' its fusion estimates each map's normals from its depths, tests them and writes
    them into final3d_model.ply -- what main --normals depth makes from the written files; scoring and cleaning read the points as before."""
    out = {name: getattr(args, prefix + name) for name in ('normals', 'normal_threshold', 'normal_step', 'normal_depth_gate')
           if getattr(args, prefix + name, None) is not None}
    if parser is not None:
        try:
            check_normal_options(**out)
        except ValueError as e:
            parser.error(str(e))
    return out


def normal_rules(fuse_normals, fuse):
    """The ETH3D driver's rule for its fuse_normals, as (broken, message) rows: listed for a caller that gives fuse_normals --
    without it there is nothing the row could refuse."""
    return [] if fuse_normals is None else [
        (fuse is None, '--fuse_normals, --fuse_normal_threshold, --fuse_normal_step and --fuse_normal_depth_gate need --fuse '
                       '(fuse_normals needs fuse): there is no fusion whose normals they could set')]


def make_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--dense_folder', type=str, default='../eval/pointcloud/lakeside')
    parser.add_argument('--fusibile_exe_path', type=str, default='../fusibile/build/fusibile')
    parser.add_argument('--prob_threshold', type=float, default=0.8)
    parser.add_argument('--disp_threshold', type=float, default=0.01)
    parser.add_argument('--num_consistent', type=float, default=2)
    add_options(parser)
    return parser


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    normals, normal_threshold, normal_step, normal_depth_gate = check_normal_options(**options(parser, args))
    dense_folder = args.dense_folder
    point_folder = os.path.join(dense_folder, 'points_atvsnet')
    if not os.path.isdir(point_folder):
        os.mkdir(point_folder)
    print('filter depth map with probability map')
    probability_filter(dense_folder, args.prob_threshold)
    print('Convert atvsnet output to gipuma input')
    atvsnet_to_gipuma(dense_folder, point_folder, normals, normal_step, normal_depth_gate)
    print('Run depth map fusion & filter')
    depth_map_fusion(point_folder, args.fusibile_exe_path, args.disp_threshold, args.num_consistent, normal_threshold,
                     ply_normals=normals == 'depth')
    cloudlist = sorted(name for name in os.listdir(point_folder) if 'consistency' in name)
    shutil.copyfile(os.path.join(point_folder, cloudlist[-1], 'final3d_model.ply'),
                    os.path.join(dense_folder, 'final3d_model.ply'))


if __name__ == '__main__':
    main()
