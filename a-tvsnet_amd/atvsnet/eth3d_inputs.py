"""The ETH3D driver's inputs: one pair.txt entry -> images and cameras (reference eval_pointcloud.py: gen_data_list :60-94, load_data
:97-203).  load_cams is the host part of load_data for --scene_cache, whose images are prepared on the GPU (atvsnet/scene.py)."""
from __future__ import print_function

import os
import sys

import numpy as np

from ..flags import FLAGS
from . import example, scene
from .preprocess import (center_image, crop_mvs_input, crop_window, gen_pipeline_mvs_list, load_cam, scale_camera, scale_image,
                         scale_mvs_camera, scale_mvs_input, scaled_size)


def gen_data_list(dense_folder):
    """ mvs input path list (reference :60-94) """
    return gen_pipeline_mvs_list(dense_folder)


def _inverse_depth_range(cam):
    """Depth range row of a camera -> inverse-depth sweep (reference :155-170)."""
    depth_min, depth_interval = cam[1][3][0], cam[1][3][1]
    if cam[1][3][2] > 0 and cam[1][3][3] > 0:
        depth_max = cam[1][3][3]
    else:
        depth_max = depth_min + float(FLAGS.max_d - 1) * depth_interval
    disp_min, disp_max = 1.0 / depth_max, 1.0 / depth_min
    cam[1][3][:] = (disp_min, (disp_max - disp_min) / FLAGS.max_d, FLAGS.max_d, disp_max)


def _ground_truth_depth_range(ref_image, cams):
    """use ground truth depth range (reference :170-192): `<ref image>.txt` names the original image; when
    `<its folder with /images/ -> /depths/>/<name>.exr` exists, the (inverse-)depth sweep of EVERY view becomes
    [min, max] of that map over FLAGS.max_d hypotheses.  The EXR is read by tools/exr.py; an EXR that exists but cannot
    be decoded raises (a silently different sweep would change every depth map)."""
    note = ref_image[0:ref_image.rfind('.') + 1] + 'txt'
    if not os.path.exists(note):
        return
    with open(note, "r") as f:
        filename = f.readline()
    ref_image_path = ref_image[0:ref_image.rfind('/') + 1] + filename
    depth_path = ref_image_path.replace('/images/', '/depths/')
    depth_path = depth_path[0:depth_path.rfind('.') + 1] + 'exr'
    if not os.path.exists(depth_path):
        print(depth_path, 'not exist.')
        return
    from ..tools import exr
    depth_gt = exr.imread_first_channel(depth_path)
    if FLAGS.inverse_depth:
        depth_gt[depth_gt <= 0.0] = float("inf")
        depth_gt = 1.0 / (depth_gt)
    disp_max = np.max(depth_gt)
    depth_gt[depth_gt <= 0.0] = float("inf")
    disp_min = np.min(depth_gt)
    disp_interval = (disp_max - disp_min) / FLAGS.max_d
    for cam in cams:
        cam[1][3][0] = disp_min
        cam[1][3][1] = disp_interval
        cam[1][3][2] = FLAGS.max_d
        cam[1][3][3] = disp_max


def _view_paths(data):
    """The image paths of the FLAGS.view_num views of one pair.txt entry: a missing source is replaced by the reference view."""
    found = len(data) // 2
    return [data[2 * (view if view < found else 0)] for view in range(FLAGS.view_num)]


def _view_cams(data):
    """The cameras of those views as the files give them; a source without a plane count gets max_d."""
    found, cams = len(data) // 2, []
    for view in range(FLAGS.view_num):
        with open(data[2 * (view if view < found else 0) + 1]) as f:
            cam = load_cam(f, 1.0)
        if view < found and cam[1][3][2] == 0:
            cam[1][3][2] = FLAGS.max_d
        cams.append(cam)
    return cams


def _sweep_cams(ref_image, cams):
    """The closing steps on scaled and cropped cameras: inverse-depth range, ground-truth range, sample_scale."""
    if FLAGS.inverse_depth:
        for cam in cams:
            _inverse_depth_range(cam)
    _ground_truth_depth_range(ref_image, cams)
    return scale_mvs_camera(cams, scale=FLAGS.sample_scale)


def load_data(sample_list, data_index):
    """One pair.txt entry -> (scaled BGR images (1,N,h/4,w/4,3), centred images (1,N,h,w,3), cameras at
    sample_scale (1,N,2,4,4), a (1,h/4,w/4,1) placeholder, reference image index) (reference :97-203)."""
    data = sample_list[data_index]
    images, cams = [example._imread_bgr(v) for v in _view_paths(data)], _view_cams(data)
    resize_scale = 1
    if FLAGS.adaptive_scaling:
        h_scale = max(float(FLAGS.max_h) / im.shape[0] for im in images)
        w_scale = max(float(FLAGS.max_w) / im.shape[1] for im in images)
        if h_scale > 1 or w_scale > 1:
            print("max_h, max_w should < W and H!")
            print(images[-1].shape, 'h_scale', h_scale, 'w_scale', w_scale)
            sys.exit(-1)
        resize_scale = max(h_scale, w_scale)
    images, cams = scale_mvs_input(images, cams, scale=resize_scale)
    images, cams = crop_mvs_input(images, cams, base_image_size=32)
    centered = [center_image(im) for im in images]
    cams = _sweep_cams(data[0], cams)
    scaled = [scale_image(im, scale=FLAGS.sample_scale) for im in images]
    scaled_depth = scaled[-1][:, :, 0:1].copy()
    return (np.stack(scaled, 0)[None], np.stack(centered, 0)[None], np.stack(cams, 0)[None], scaled_depth[None],
            int(os.path.splitext(os.path.basename(data[0]))[0]))


def load_cams(data, shapes):
    """The host part of load_data for the scene driver (--scene_cache): the cameras of one pair.txt entry `data` whose views'
    images are (h, w) = `shapes` (after the missing-source substitution) -> (cams (1,N,2,4,4) at sample_scale, the adaptive
    scale).  The same steps on the same values as load_data: scale, crop offset, inverse-depth range, ground-truth range,
    sample_scale."""
    cams = _view_cams(data)
    resize_scale = scene.adaptive_scale(shapes) if FLAGS.adaptive_scaling else 1
    if resize_scale is None:
        print("max_h, max_w should < W and H!")
        print(shapes[-1], 'h_scale', max(float(FLAGS.max_h) / s[0] for s in shapes),
              'w_scale', max(float(FLAGS.max_w) / s[1] for s in shapes))
        sys.exit(-1)
    for v in range(FLAGS.view_num):
        cams[v] = scale_camera(cams[v], scale=resize_scale)
        y0, x0, _, _ = crop_window(*scaled_size(shapes[v][0], shapes[v][1], resize_scale), base_image_size=32)
        cams[v][1][0][2] -= x0
        cams[v][1][1][2] -= y0
    return np.stack(_sweep_cams(data[0], cams), 0)[None], resize_scale
