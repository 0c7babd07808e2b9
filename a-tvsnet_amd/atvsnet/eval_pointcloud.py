"""ETH3D batch driver: depth + probability maps for every reference image of a set of scenes.

Mirror of /root/reference/atvsnet/eval_pointcloud.py (gen_data_list :60-94, load_data :97-203, run_eval_pc
:206-397, main :400-424): the same on-disk inputs (<scene>/pair.txt, images/%08d.jpg, cams/%08d_cam.txt) and
outputs (<savepath>/<scene>/depths_atvsnet/%08d.pfm, %08d_prob.pfm, %08d.jpg, %08d.txt, %08d.png,
zz_runtime.txt).  The session.run sequence of the reference (base per source, AAM1, refinement per source,
AAM2 with probability maps) is pipeline.infer_multiview(out_prob_map=True), replayed from one HIP graph per
input shape.  Not available here and therefore not done: the optional ground-truth depth range from
depths/*.exr (:170-192, needs an EXR reader).
"""
from __future__ import print_function

import argparse
import os
import sys
import time

import numpy as np
import torch

from .. import variables
from ..flags import FLAGS
from ..tools.common import Notify
from . import clean_cloud
from . import clean_mesh
from . import depth_fusion
from . import eval_cloud
from . import eval_depth
from . import example, graphs, pipeline, range_guard
from . import scene
from .preprocess import (center_image, crop_mvs_input, crop_window, gen_pipeline_mvs_list, load_cam, scale_camera, scale_image,
                         scale_mvs_camera, scale_mvs_input, scaled_size, write_cam, write_pfm)

ETH3D_LOW_RES_TEST = ['lakeside', 'sand_box', 'storage_room', 'storage_room_2', 'tunnel']


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


class _Decoder(object):
    """Host uint8 BGR images by path: decoded on demand or by ONE background thread ahead of use (prefetch)."""

    def __init__(self):
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(1)
        self.pending = {}

    def prefetch(self, paths):
        for p in paths:
            if p not in self.pending:
                self.pending[p] = self.pool.submit(example._imread_bgr, p)

    def __call__(self, path):
        f = self.pending.pop(path, None)
        return f.result() if f is not None else example._imread_bgr(path)

    @staticmethod
    def shape(path):
        from PIL import Image
        with Image.open(path) as im:
            w, h = im.size
        return h, w

    def close(self):
        self.pool.shutdown(wait=True)
        self.pending.clear()


class _Writer(object):
    """A scene's file writing on one background thread behind a bounded queue (threaded=False: in the caller).  timed: times()
    gives TIMES' writer_busy, the seconds spent in the jobs themselves (the scene-cache route reports it)."""

    def __init__(self, threaded, depth=4, timed=False):
        import queue
        import threading
        self.thread, self.error, self.busy, self.timed = None, None, 0.0, timed
        if threaded:
            self.queue = queue.Queue(maxsize=depth)
            self.thread = threading.Thread(target=self._loop, name='atvs-writer', daemon=True)
            self.thread.start()

    def _loop(self):
        while True:
            job = self.queue.get()
            if job is None:
                return
            if self.error is None:
                try:
                    self._run(job)
                except BaseException as e:       # re-raised in the driver's thread
                    self.error = e

    def _run(self, job):
        t0 = time.time()
        try:
            job()
        finally:
            self.busy += time.time() - t0

    def __call__(self, job):
        if self.error is not None:
            raise self.error
        if self.thread is not None:
            self.queue.put(job)
        else:
            self._run(job)

    def times(self):
        return {'writer_busy': self.busy} if self.timed else {}

    def close(self):
        if self.thread is not None:
            self.queue.put(None)
            self.thread.join()
            self.thread = None
        if self.error is not None:
            raise self.error


class _Pipelines(object):
    """One set of captured HIP graphs per input shape (scenes of one data set share it), SLOTS depth maps queued:
    submit() issues a depth map asynchronously, fetch() returns the oldest one's results as numpy arrays.
    CO_RESIDENT = False: the GPU runs one depth map at a time (the reference's scene loop, eval_pointcloud.py:291-396, is
    serial too); the second slot only lets the host load / submit the next view and write the previous one's files
    meanwhile.  True runs both maps' kernels concurrently (+4.5 % maps/s) and stays off until the co-residency fault of
    DESIGN.md appendix B is root-caused or a >= 10,000-map full-size soak is clean; 'cu_split' (cli --maps_in_flight cu_split)
    runs them concurrently on disjoint halves of every XCD, where that fault cannot occur."""

    SLOTS = 2
    CO_RESIDENT = False

    def __init__(self, device, use_graph=True):
        self.device, self.use_graph, self.cache = device, use_graph, {}
        self.pending = []            # (pipeline, ticket) or (None, tensors) in submission order

    def submit(self, images_data, cams_data):
        images = torch.from_numpy(np.ascontiguousarray(images_data, dtype=np.float32))
        cams = torch.from_numpy(np.ascontiguousarray(cams_data, dtype=np.float32))
        split = self.use_graph and self.CO_RESIDENT == 'cu_split'
        key = tuple(images.shape)
        if not (split and key in self.cache):
            # (cu_split: the slot's own stream copies the HOST tensors -- an upload on the default stream would wait for the map in
            # flight on the other half of the chip, graphs.PipelinedInference.submit; the first map of a shape still needs device
            # tensors to capture the graphs from)
            images, cams = images.to(self.device), cams.to(self.device)
        if not self.use_graph:
            # eager: computed here, with the drivers' range guard (an fp16-range overflow reruns the map on the fp32 kernels)
            self.pending.append((None, range_guard.infer_checked(
                lambda: pipeline.infer_multiview(images, cams, FLAGS.max_d, out_prob_map=True), self.device)))
            return
        p = self.cache.get(key)
        if p is None:
            p = self.cache[key] = graphs.PipelinedInference(images, cams, FLAGS.max_d, slots=self.SLOTS,
                                                                co_resident=self.CO_RESIDENT, out_prob_map=True)
        self.pending.append((p, p.submit(images, cams)))

    def room(self):
        return len(self.pending) < self.SLOTS

    def fetch(self):
        p, t = self.pending.pop(0)
        # result(): the fp32 rerun of a map whose split-operand replay overflowed; host=True: copied by the slot's own stream
        out = t if p is None else p.result(t, host=True)
        return [range_guard.check_finite(o.cpu().numpy(), 'a network output') for o in out]


def _write_map(output_folder, out_index, outputs, image_raw, cams, plt):
    """finish()'s files of one depth map: PFMs, the 1/4 reference image, the camera text, the viridis PNG."""
    from PIL import Image
    depth, depth_up, prob, prob_up = outputs
    disp_up = np.squeeze(depth_up.copy())
    if FLAGS.inverse_depth:
        for m in (depth, depth_up):
            m[m <= 0] = float("inf")
        depth, depth_up = 1.0 / depth, 1.0 / depth_up
    stem = os.path.join(output_folder, '%08d' % out_index)
    write_pfm(stem + '.pfm', np.squeeze(depth).astype(np.float32))
    write_pfm(stem + '_prob.pfm', np.squeeze(prob).astype(np.float32))
    if getattr(FLAGS, 'write_upsampled', False):      # commented out in the reference (:378-379)
        write_pfm(stem + '_up.pfm', np.squeeze(depth_up).astype(np.float32))
        write_pfm(stem + '_prob_up.pfm', np.squeeze(prob_up).astype(np.float32))
    Image.fromarray(np.ascontiguousarray(image_raw[:, :, ::-1])).save(stem + '.jpg')
    write_cam(stem + '.txt', cams)
    plt.imsave(stem + '.png', disp_up, cmap='viridis')


class _PipelineSource(object):
    """The default route's maps: load_data's host arrays through _Pipelines; finish() hands out host arrays.  A map source is
    driven by _run_scene: begin_scene(mvs_list), then per map load(i), room(), submit(what load gave) and finish(stage) ->
    (out_index, the outputs on the host, the reference image, its (2,4,4) camera), end_scene() -> its own TIMES entries, close()."""

    def __init__(self, device, use_graph):
        self.run, self.queued = _Pipelines(device, use_graph), []          # queued: host data of the maps in flight, in order

    def begin_scene(self, mvs_list):
        self.mvs_list = mvs_list

    def end_scene(self):
        return {}

    def room(self):
        return self.run.room()

    def close(self):
        pass

    def load(self, i):
        return load_data(self.mvs_list, i)

    def submit(self, loaded):
        image_data_raw, images_data, cams_data, _depth, out_index = loaded
        self.run.submit(images_data, cams_data)
        self.queued.append((out_index, image_data_raw[0, 0], cams_data[0, 0]))

    def finish(self, stage):
        out_index, image_raw, cam = self.queued.pop(0)
        outputs = self.run.fetch()                   # host arrays, under check_finite's range guard
        if stage is not None:       # now: _write_map's inverse-depth step rewrites the host maps in place
            stage(out_index, outputs[0], outputs[2], image_raw, cam)
        return out_index, outputs, image_raw, cam


class _SceneSource(object):
    """--scene_cache's maps: every image prepared and run through the towers once per scene (scene.SceneInference), decoded one
    map ahead by _Decoder, the cameras from load_cams; finish() stages device tensors on the slot's stream."""

    def __init__(self, device):
        self.decoder, self.queued = _Decoder(), []          # queued: (ticket, cameras, out_index) of the maps in flight, in order
        self.run = scene.SceneInference(self.decoder, FLAGS.max_d, slots=_Pipelines.SLOTS, co_resident=_Pipelines.CO_RESIDENT or False,
                                        device=device, shape=self.decoder.shape)

    def begin_scene(self, mvs_list):
        self.mvs_list = mvs_list
        self.run.times['upload'], self.run.gpu_ms = 0.0, []

    def end_scene(self):
        return {'upload': self.run.times['upload'], 'gpu_ms': list(self.run.gpu_ms)}          # upload: part of `submit`

    def room(self):
        return self.run.room()

    def close(self):
        self.decoder.close()

    def load(self, i):
        views = _view_paths(self.mvs_list[i])
        if i + 1 < len(self.mvs_list):          # before this map's cameras are read: the decoding overlaps them
            self.decoder.prefetch([v for v in _view_paths(self.mvs_list[i + 1]) if ('image', v) not in self.run.cache])
        cams_data, _ = load_cams(self.mvs_list[i], [self.run.shape(v) for v in views])
        return views, cams_data, int(os.path.splitext(os.path.basename(self.mvs_list[i][0]))[0])

    def submit(self, loaded):
        views, cams_data, out_index = loaded
        self.queued.append((self.run.submit(views, cams_data), cams_data[0, 0], out_index))

    def finish(self, stage):
        ticket, cam, out_index = self.queued.pop(0)
        if stage is None:
            # result() has read the non-finite flag on the slot's stream: no second (default-stream) read here
            outputs = [range_guard.check_finite(o.numpy(), 'a network output', flag=False) for o in self.run.result(ticket, host=True)]
            return out_index, outputs, self.run.reference_image(ticket), cam
        # the slot's output buffers are overwritten by its next submission: staged from what result() returned (an overflowed
        # map's fp32 rerun), on the slot's stream, before submit() can reuse the slot; the host copies under that stream too
        dev_out = self.run.result(ticket)
        st = self.run.slot_stream(ticket)
        stage(out_index, dev_out[0], dev_out[2], self.run.reference_image(ticket, host=False), cam, stream=st)
        with torch.cuda.stream(st):
            outputs = [range_guard.check_finite(o.cpu().numpy(), 'a network output', flag=False) for o in dev_out]
            return out_index, outputs, self.run.reference_image(ticket), cam


# host time of the last scene run_eval_pc processed, seconds summed over its maps: prepare (load_data / load_cams), submit, wait
# (fetch / result), write (finish's files; with the writer thread: the hand-over); --scene_cache adds upload (the image uploads'
# share of submit) and gpu_ms (each map's GPU time, SceneInference.gpu_ms) -- tools_dev/scene_rate.py reports them
TIMES = {}


def _run_scene(source, mvs_list, savepath_current, writer, map_files=True, fuse=None, keep_cams=False, device=None):
    """The depth maps of one scene from `source` (a _PipelineSource, a _SceneSource), their files through `writer`, which is closed
    before zz_runtime.txt is written.  fuse: run_eval_pc's; every map is staged in the scene's SceneFusion, made at the first
    map, and with keep_cams its (2,4,4) camera is kept.  -> (that SceneFusion or None, {out_index: camera}, the wall clock)."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    output_folder = os.path.join(savepath_current, 'depths_atvsnet')
    os.makedirs(output_folder, exist_ok=True)
    TIMES.clear()                # this scene's maps only
    TIMES.update(prepare=0.0, submit=0.0, wait=0.0, write=0.0, maps=0)
    fusion, map_cams = [], {}

    def stage(out_index, depth, prob, image, cam, stream=None):
        if not fusion:               # made here: the maps' size
            rows, cols = image.shape[:2]
            fusion.append(depth_fusion.SceneFusion(len(mvs_list), rows, cols, device, **fuse))
        fusion[0].add(out_index, depth, prob, image, cam, stream=stream)
        if keep_cams:
            map_cams[out_index] = np.array(cam, np.float64)

    def finish():
        t0 = time.time()
        out_index, outputs, image_raw, cam = source.finish(stage if fuse is not None else None)
        t1 = time.time()
        if map_files:
            writer(lambda: _write_map(output_folder, out_index, outputs, image_raw, cam, plt))
        TIMES['wait'] += t1 - t0
        TIMES['write'] += time.time() - t1
        TIMES['maps'] += 1

    source.begin_scene(mvs_list)
    start_time = time.time()
    # the depth maps of a scene are independent: the next one is submitted before the previous one's results are
    # fetched and written, so file I/O overlaps the GPU (which still runs one map at a time: _Pipelines.CO_RESIDENT)
    for current_i in range(len(mvs_list)):
        t0 = time.time()
        loaded = source.load(current_i)
        t1 = time.time()
        if not source.room():
            finish()
        t2 = time.time()
        source.submit(loaded)
        TIMES['prepare'] += t1 - t0
        TIMES['submit'] += time.time() - t2
    while TIMES['maps'] < len(mvs_list):
        finish()
    writer.close()                       # this scene's files are on disk before its runtime is written
    TIMES.update(writer.times())
    TIMES.update(source.end_scene())
    scene_runtime = time.time() - start_time       # wall clock of the scene (the reference sums sess.run times)
    with open(os.path.join(savepath_current, 'zz_runtime.txt'), "w") as text_file:
        text_file.write('runtime ' + str(scene_runtime))
    return (fusion[0] if fusion else None), map_cams, scene_runtime


def _write_cloud(scene_fusion, folder):
    """final3d_model.ply -> its point count.  After every map's result: the slots are idle; the fusion runs on this thread's
    (ordinary) stream."""
    t0 = time.time()
    n_points = scene_fusion.write_ply(os.path.join(folder, 'final3d_model.ply'))
    TIMES['fuse'] = time.time() - t0
    return n_points


def _source_planes(register_args):
    """Whether the registration runs over the fused cloud's own normals (point-to-plane, not over the ground truth's)."""
    return register_args.get('register_icp') == 'plane' and register_args.get('register_normals') != 'target'


def _score_cloud(points, folder, device, gt_points, register_args, init_cameras, normals=None):
    """cloud_eval.json -> the score.  normals: the fused points' own, for a point-to-plane registration."""
    t0 = time.time()
    plane = {'recon_normals': normals} if _source_planes(register_args) else {}
    score = eval_cloud.evaluate(points, gt_points, device=device, **dict(register_args, **plane))
    if init_cameras is not None:
        score['init_cameras'] = init_cameras
    eval_cloud.write_json(os.path.join(folder, 'cloud_eval.json'), score)
    TIMES['cloud_eval'] = time.time() - t0
    return score


def _score_maps(scene_fusion, map_cams, score, folder, device, gt_points, score_maps):
    """depth_eval.json.  run() has ordered this stream after every staging; nd[..., 3] is the depth plane the fusion read."""
    t0 = time.time()
    order = scene_fusion.order()
    indices = [scene_fusion.index[k] for k in order]
    moved = score['registration']['matrix'] if 'registration' in score else None
    score_maps = dict(score_maps)
    files, tol = score_maps.pop('occlusion_mesh', None), score_maps.pop('occlusion_mesh_tol', None)
    occlude, extra = {}, {}
    if files:                                                            # the occluded maps, and what occluded them in the report
        occluder = eval_depth.load_meshes(files)
        tol = eval_depth.DEFAULT_OCCLUDER_TOL if tol is None else tol
        occlude = dict(occluders=[occluder], occluder_tol=tol)
        extra = dict(occlusion_mesh_tol=tol, occlusion_faces=len(occluder[1]))
    gt_maps = eval_depth.render_scan(gt_points, np.stack([map_cams[i] for i in indices]), scene_fusion.rows, scene_fusion.cols,
                                     transform=moved, device=device, **dict(score_maps, **occlude))
    pred = scene_fusion.nd[:len(indices), :, :, 3][torch.from_numpy(order).to(device)]
    eval_depth.write_json(os.path.join(folder, 'depth_eval.json'),
                          eval_depth.report(pred.cpu().numpy(), gt_maps.cpu().numpy(), indices=indices, transform=moved,
                                            **dict(score_maps, **extra)))
    TIMES['depth_eval'] = time.time() - t0


def _clean_cloud(points, colors, score, folder, device, gt_points, clean, normals=None):
    """final3d_model_clean.ply and cloud_clean.json, with a score cloud_eval_clean.json -> the cleaned point count.  normals: the
    fused points' own; those of the rows that stay are written into the cleaned PLY."""
    from ..tools.ply import write_ply
    t0 = time.time()
    clean_normals = None
    if normals is None:
        clean_points, clean_colors, clean_report = clean_cloud.clean(points, colors, device=device, **clean)
    else:
        clean_points, clean_colors, clean_normals, clean_report = clean_cloud.clean(points, colors, device=device, normals=normals, **clean)
    write_ply(os.path.join(folder, 'final3d_model_clean.ply'), clean_points, clean_colors, clean_normals)
    clean_cloud.write_json(os.path.join(folder, 'cloud_clean.json'), clean_report)
    TIMES['cloud_clean'] = time.time() - t0
    if score is not None:
        # the same transform: the matrix found for the whole cloud (it includes the initial one), not a second fit
        moved = {}
        if 'registration' in score:
            moved['init_transform'] = score['registration']['matrix']
        elif 'init_transform' in score:
            moved['init_transform'] = score['init_transform']
        clean_score = eval_cloud.evaluate(clean_points, gt_points, device=device, **moved)
        eval_cloud.write_json(os.path.join(folder, 'cloud_eval_clean.json'), clean_score)
    return len(clean_points)


def _write_mesh(scene_fusion, map_cams, folder, mesh):
    """final3d_mesh.ply and mesh.json -> the face count.  After the cloud: the fusion's result bounds the volume.  With clean= in
    `mesh` also final3d_mesh_clean.ply and mesh_clean.json, the mesh without its small components (SceneMesh's clean=)."""
    from . import mesh_fusion
    t0 = time.time()
    scene_mesh = mesh_fusion.SceneMesh(scene_fusion, map_cams, **mesh)
    n_faces = scene_mesh.write_ply(os.path.join(folder, 'final3d_mesh.ply'))
    if mesh.get('render'):
        scene_mesh.render(os.path.join(folder, 'depths_mesh'))
    mesh_fusion.write_json(os.path.join(folder, 'mesh.json'), scene_mesh.report())
    if mesh.get('clean'):
        scene_mesh.write_clean_ply(os.path.join(folder, 'final3d_mesh_clean.ply'))
        mesh_fusion.write_json(os.path.join(folder, 'mesh_clean.json'), scene_mesh.clean_report())
    TIMES['mesh'] = time.time() - t0
    return n_faces


def _end_scene(name, scene_fusion, map_cams, folder, device, gt_points, register_args, init_cameras, score_maps, clean,
               clean_keep_normals=False, mesh=None):
    """A fused scene's files, each group by its own step: the PLY, the mesh, the cloud's score, the maps' score, the cleaned cloud."""
    n_points = _write_cloud(scene_fusion, folder)
    if mesh is not None:
        print(Notify.INFO, '%s: %d mesh faces' % (name, _write_mesh(scene_fusion, map_cams, folder, mesh)), Notify.ENDC)
    points, colors, score, normals = None, None, None, None
    if gt_points is not None or clean:
        points, colors = scene_fusion.run()
        points = points.copy()
        points[~np.isfinite(points).all(axis=1)] = 0.0          # as tools/ply.write_ply stores them
        if _source_planes(register_args) or clean_keep_normals:
            normals = scene_fusion.normals().copy()
            normals[~np.isfinite(normals).all(axis=1)] = 0.0     # likewise
    if gt_points is not None:
        score = _score_cloud(points, folder, device, gt_points, register_args, init_cameras, normals)
    if score_maps is not None:
        _score_maps(scene_fusion, map_cams, score, folder, device, gt_points, score_maps)
    if clean:
        n_clean = _clean_cloud(points, colors, score, folder, device, gt_points, clean, normals if clean_keep_normals else None)
        print(Notify.INFO, '%s: %d points after cleaning' % (name, n_clean), Notify.ENDC)
    print(Notify.INFO, '%s: %d fused points' % (name, n_points), Notify.ENDC)


def _option_rules(use_graph=True, scene_cache=False, write_thread=True, fuse=None, map_files=True, gt_ply=None, register=None,
                  clean=None, score_maps=None, fuse_normals=None, clean_keep_normals=False, mesh=None):
    """What each of run_eval_pc's options needs -> every rule as (broken by these values, message).  The row of fuse_normals is
    listed for a caller that gives fuse_normals: without it there is nothing the row could refuse.  The rows of a point-to-plane
    registration, of clean_keep_normals and of mesh likewise, at the end."""
    mesh_row = [] if mesh is None else [
        (fuse is None, '--mesh_voxel, --mesh_trunc_voxels, --mesh_min_weight and --mesh_max_blocks need --fuse (mesh needs fuse): the '
                       'mesh is integrated from the maps the fusion stages and bounded by its cloud'),
        (mesh.get('voxel') is None, '--mesh_trunc_voxels, --mesh_min_weight and --mesh_max_blocks need --mesh_voxel (mesh needs voxel=)')]
    if mesh is not None and mesh.get('carve_weight') is not None:
        mesh_row.insert(1, (mesh.get('voxel') is None, '--mesh_carve needs --mesh_voxel (mesh carve_weight= needs voxel=): there is no '
                                                       'volume to carve'))
    if mesh is not None and mesh.get('clean') is not None:                 # in front of the row above: its message names what was given
        mesh_row.insert(1, (mesh.get('voxel') is None, '--mesh_clean_min_faces, --mesh_clean_min_ratio and --mesh_clean_keep_largest need '
                                                       '--mesh_voxel (mesh clean= needs voxel=): there is no mesh to clean'))
    normals_row = [] if fuse_normals is None else [
        (fuse is None, '--fuse_normals, --fuse_normal_threshold, --fuse_normal_step and --fuse_normal_depth_gate need --fuse '
                       '(fuse_normals needs fuse): there is no fusion whose normals they could set')]
    no_normals = not (fuse_normals or {}).get('normals') == 'depth'
    target = (register or {}).get('normal_side') == 'target'
    plane_row = [] if not (register or {}).get('icp') == 'plane' or target else [
        (no_normals, '--register_icp plane needs --fuse_normals depth (register icp=plane needs fuse_normals normals=depth): '
                     'point-to-plane registration runs over the fused cloud\'s own normals; or give --register_normals target '
                     '(register normal_side=target): the ground truth\'s planes, its normals estimated on the GPU')]
    target_row = [] if not any(k in (register or {}) for k in ('normal_side', 'normal_k', 'normal_radius')) else [
        (target and not register.get('icp') == 'plane', '--register_normals target needs --register_icp plane (register '
                                                        'normal_side=target needs icp=plane)'),
        (not target and ('normal_k' in register or 'normal_radius' in register),
         '--register_normal_k and --register_normal_radius need --register_normals target (normal_k and normal_radius need '
         'normal_side=target)')]
    global_row = [] if (register or {}).get('global') is None else [
        (bool(register.get('init_cameras')), '--register_global finds the initial matrix from the clouds alone: give it or '
                                             '--init_cameras (register global= or init_cameras=)')]
    keep_row = [] if not clean_keep_normals else [
        (not clean, '--clean_keep_normals needs --clean_voxel, --clean_sor or --clean_radius_filter (clean_keep_normals needs clean)'),
        (no_normals, '--clean_keep_normals needs --fuse_normals depth (clean_keep_normals needs fuse_normals normals=depth): there are '
                     'no normals to keep')]
    return normals_row + [
        (scene_cache and not use_graph, '--scene_cache replays captured graphs: it cannot be combined with --eager (use_graph=False)'),
        (not map_files and fuse is None, '--no_map_files needs --fuse (map_files=False needs fuse): the run would write nothing'),
        (bool(gt_ply) and fuse is None, '--gt_ply needs --fuse (gt_ply needs fuse): there is no point cloud to score'),
        (register is not None and not gt_ply, '--register needs --gt_ply (register needs gt_ply): there is nothing to align to'),
        (bool(clean) and fuse is None, '--clean_voxel, --clean_sor and --clean_radius_filter need --fuse (clean needs fuse): there is no '
                                       'point cloud to clean'),
        (score_maps is not None and not gt_ply, '--score_maps needs --gt_ply (score_maps needs gt_ply): there is no scan to render')
    ] + target_row + plane_row + global_row + keep_row + mesh_row


def _check_options(**options):
    """Raises ValueError with the message of the first of _option_rules that `options` break."""
    for broken, message in _option_rules(**options):
        if broken:
            raise ValueError(message)


def run_eval_pc(savepath, image_infos, use_graph=True, scene_cache=False, write_thread=True, fuse=None, map_files=True,
                gt_ply=None, register=None, clean=None, score_maps=None, fuse_normals=None, clean_keep_normals=False, mesh=None):
    """(reference :206-397) image_infos: [[[dense_path, image_folder, scene_name], format], ...]
    scene_cache: every image prepared and run through the towers once per scene (atvsnet/scene.py), the files written by one
    background thread (write_thread=False: in this thread, same bytes).
    fuse: None, or dict(prob_threshold=, disp_threshold=, num_consistent=): every map is also staged on the device as it is
    finished (depth_fusion.SceneFusion) and each scene ends with <savepath>/<scene>/final3d_model.ply, the point cloud
    depth_fusion.main makes from the written files.  map_files=False (with fuse only): no per-map files.
    fuse_normals (with fuse only): None, or a dict of SceneFusion's normal options (normals=, normal_threshold=, normal_step=,
    normal_depth_gate=): with normals='depth' the fusion estimates each map's normals from its depths, tests them and writes them
    into final3d_model.ply -- what depth_fusion.main --normals depth makes from the written files.  Scoring and cleaning read the
    points as before.
    gt_ply (with fuse only): ground-truth PLY paths; each scene's fused points, as the PLY stores them, are scored against them
    (eval_cloud.evaluate, default tolerances) into <savepath>/<scene>/cloud_eval.json -- what eval_cloud's CLI gives on that PLY.
    register (with gt_ply only): None, or dict(with_scale=, init_cameras=(recon_sparse, gt_sparse) or None): the cloud is aligned
    to the ground truth before it is scored (eval_cloud --register [--init_cameras]); cloud_eval.json carries `registration`.
    With icp='plane' in the dict (fuse_normals normals='depth' only) the registration is point-to-plane over the normals the
    fusion returns (eval_cloud --register_icp plane); with normal_side='target' too (and optionally normal_k, normal_radius) over
    the ground truth's planes instead, its normals estimated on the device: no fuse_normals needed (eval_cloud --register_normals).
    With global= in the dict ({} or register_cloud.global_init's keyword arguments) the start is found from the clouds alone
    (eval_cloud --register_global); init_cameras is then refused.
    clean_keep_normals (with clean and fuse_normals normals='depth' only): final3d_model_clean.ply carries the normals of the rows
    that stay (clean_cloud --keep_normals).
    clean (with fuse only): None, or dict(voxel=, sor=(k, ratio, radius), radius_filter=(radius, min_neighbours)), the arguments of
    clean_cloud.clean: each scene's fused points, as the PLY stores them, are cleaned into <savepath>/<scene>/
    final3d_model_clean.ply with the report in cloud_clean.json; with gt_ply the cleaned cloud is scored too, into
    cloud_eval_clean.json (with register: moved by the matrix found for the uncleaned cloud, not registered again).
    final3d_model.ply and cloud_eval.json are what they are without it.
    score_maps (with gt_ply only): None, or dict(splat=, occlusion_tol=, pixel_centre=), the arguments of eval_depth.render_scan:
    after the scene's fusion the ground truth is rendered into the scene's cameras (in SceneFusion.order()) and the staged,
    probability-filtered depth planes -- what enters the cloud -- are scored against it (eval_depth.score_maps) into
    <savepath>/<scene>/depth_eval.json.  With register the ground truth is moved by the inverse of the matrix already found (no
    second fit).  With occlusion_mesh= (a list of triangle-mesh PLY files in the ground truth's frame) and occlusion_mesh_tol= in
    the dict, a rendered pixel that lies behind those meshes is taken out first (eval_depth.render_scan's occluders).  Every other
    output is what it is without it.
    mesh (with fuse only): None, or dict(voxel=, trunc_voxels=, min_weight=, max_blocks=, clean=, carve_weight=), the arguments of mesh_fusion.SceneMesh
    (clean=dict(min_faces=, min_ratio=, keep_largest=) also writes final3d_mesh_clean.ply and mesh_clean.json, the mesh without the
    connected components that miss a criterion; the other files keep their bytes):
    after the scene's fusion the staged depth planes and images are integrated into a TSDF volume bounded by the fused cloud and
    meshed by marching tetrahedra into <savepath>/<scene>/final3d_mesh.ply, with the report in mesh.json; with render=True the
    mesh is also rendered into the scene's map cameras as <savepath>/<scene>/depths_mesh/%08d_mesh.pfm (SceneMesh.render).  Every
    other output is what it is without it."""
    assert FLAGS.view_num > 2, 'the ETH3D driver runs the multi-view (AANet) pipeline'
    _check_options(use_graph=use_graph, scene_cache=scene_cache, fuse=fuse, map_files=map_files, gt_ply=gt_ply, register=register,
                   clean=clean, score_maps=score_maps, fuse_normals=fuse_normals, clean_keep_normals=clean_keep_normals,
                   **({} if mesh is None else {'mesh': mesh}))
    if mesh is not None:
        from . import mesh_fusion
        mesh_fusion.check_options(**mesh)
    if fuse_normals is not None:
        depth_fusion.check_normal_options(**fuse_normals)
        fuse = dict(fuse, **fuse_normals)
    gt_points, register_args, init_cameras = None, {}, None
    if gt_ply:
        from ..tools.ply import read_ply_points
        gt_points = np.concatenate([read_ply_points(p) for p in gt_ply], 0)
    if register is not None:
        register_args = dict(register=True, with_scale=bool(register.get('with_scale')))
        if register.get('icp') == 'plane':
            register_args['register_icp'] = 'plane'
        if register.get('normal_side') == 'target':
            register_args['register_normals'] = 'target'
            for key in ('normal_k', 'normal_radius'):
                if register.get(key) is not None:
                    register_args['register_' + key] = register[key]
        if register.get('global') is not None:
            register_args['register_global'] = True
            if register['global']:
                register_args['global_options'] = dict(register['global'])
        if register.get('init_cameras'):
            from . import register_cloud
            init, matched, rms = register_cloud.init_from_cameras(*register['init_cameras'])
            register_args['init_transform'] = init
            init_cameras = {'recon_sparse': str(register['init_cameras'][0]), 'gt_sparse': str(register['init_cameras'][1]),
                            'matched_images': matched, 'rms': rms}
    example._load_weights()
    torch.cuda.set_device(FLAGS.gpu_id)          # every kernel launches on the current device's stream
    device = torch.device('cuda:%d' % FLAGS.gpu_id)
    source = _SceneSource(device) if scene_cache else _PipelineSource(device, use_graph)
    try:
        for image_info, _fmt in image_infos:
            mvs_list = gen_data_list(image_info[0])
            savepath_current = os.path.join(savepath, image_info[2])
            writer = _Writer(scene_cache and write_thread, timed=scene_cache)
            try:
                scene_fusion, map_cams, scene_runtime = _run_scene(source, mvs_list, savepath_current, writer, map_files, fuse,
                                                                   score_maps is not None or mesh is not None, device)
            finally:
                writer.close()
            if scene_fusion is not None:
                _end_scene(image_info[2], scene_fusion, map_cams, savepath_current, device, gt_points, register_args, init_cameras,
                           score_maps, clean, clean_keep_normals, mesh)
            print(Notify.INFO, '%s: %d depth maps, %.2f s' % (image_info[2], len(mvs_list), scene_runtime), Notify.ENDC)
    finally:
        source.close()


def _normal_options(flags):
    """run_eval_pc's fuse_normals from cli's --fuse_normal* options: those that were given, None when none was."""
    names = dict(fuse_normals='normals', fuse_normal_threshold='normal_threshold', fuse_normal_step='normal_step',
                 fuse_normal_depth_gate='normal_depth_gate')
    given = {key: getattr(flags, option) for option, key in names.items() if getattr(flags, option, None) is not None}
    return given or None


def _target_options(flags):
    """The entries of run_eval_pc's register dict from cli's --register_normal* options: those that were given."""
    names = dict(register_normals='normal_side', register_normal_k='normal_k', register_normal_radius='normal_radius')
    given = {key: getattr(flags, option) for option, key in names.items() if getattr(flags, option, None) is not None}
    if given.get('normal_side') == 'source':
        del given['normal_side']                                    # the default: nothing new is passed on
    return given


def _global_options(flags):
    """The entry `global` of run_eval_pc's register dict from cli's --register_global options: absent without --register_global,
    else register_cloud.global_init's keyword arguments that were given."""
    if not getattr(flags, 'register_global', False):
        return {}
    given = {key: getattr(flags, option) for option, key in eval_cloud.GLOBAL_FLAGS.items() if getattr(flags, option, None) not in (None, False)}
    if 'mutual' in given:
        given['mutual'] = False
    return {'global': given}


def _mesh_options(flags):
    """run_eval_pc's mesh from cli's --mesh_* options: those that were given, None when none was."""
    names = dict(mesh_voxel='voxel', mesh_trunc_voxels='trunc_voxels', mesh_min_weight='min_weight', mesh_max_blocks='max_blocks')
    given = {key: getattr(flags, option) for option, key in names.items() if getattr(flags, option, None) is not None}
    if getattr(flags, 'mesh_render', False):
        given['render'] = True
    if getattr(flags, 'mesh_carve', None) is not None:
        given['carve_weight'] = flags.mesh_carve
    clean = {key: getattr(flags, 'mesh_clean_' + key) for key in ('min_faces', 'min_ratio', 'keep_largest')
             if getattr(flags, 'mesh_clean_' + key, None) is not None}
    if clean:
        given['clean'] = clean
    return given or None


def _map_occlusion_options(flags):
    """score_maps' occlusion_mesh (a list of files) and occlusion_mesh_tol from cli's --map_occlusion_mesh options: those given."""
    files = getattr(flags, 'map_occlusion_mesh', None)
    if not files:
        return {}
    files = [p for p in files.split(',') if p] if isinstance(files, str) else list(files)
    tol = getattr(flags, 'map_occlusion_mesh_tol', None)
    return dict({'occlusion_mesh': files}, **({} if tol is None else {'occlusion_mesh_tol': tol}))


def _run_options(flags):
    """run_eval_pc's keyword arguments from a namespace of cli's options (FLAGS, cli's parsed arguments): one it lacks is off."""
    opt = lambda name, default=None: getattr(flags, name, default)          # noqa: E731
    mesh = _mesh_options(flags)
    return dict(
        {} if mesh is None else {'mesh': mesh},
        use_graph=not opt('eager'), scene_cache=opt('scene_cache', False), write_thread=not opt('sync_write'),
        fuse=dict(prob_threshold=flags.prob_threshold, disp_threshold=flags.disp_threshold, num_consistent=flags.num_consistent)
        if opt('fuse') else None,
        fuse_normals=_normal_options(flags),
        map_files=not opt('no_map_files'), gt_ply=opt('gt_ply') or None, clean=opt('clean') or None,
        register=dict(dict(icp='plane') if opt('register_icp') == 'plane' else {}, with_scale=opt('with_scale', False),
                      init_cameras=opt('init_cameras') or None, **dict(_target_options(flags), **_global_options(flags)))
        if opt('register') else None,
        clean_keep_normals=bool(opt('clean_keep_normals')),
        score_maps=dict(splat=opt('map_splat', eval_depth.DEFAULT_SPLAT),
                        occlusion_tol=opt('map_occlusion_tol', eval_depth.DEFAULT_OCCLUSION_TOL),
                        pixel_centre=opt('map_pixel_centre', eval_depth.DEFAULT_PIXEL_CENTRE),
                        **_map_occlusion_options(flags)) if opt('score_maps') else None)


def main(scene_list=None, base_path='eth3d/'):
    """(reference :400-424)"""
    scene_list = ETH3D_LOW_RES_TEST if scene_list is None else scene_list
    os.makedirs(FLAGS.savepath, exist_ok=True)
    FLAGS.max_h = int(FLAGS.max_h / 32) * 32
    FLAGS.max_w = int(FLAGS.max_w / 32) * 32
    image_infos = []
    for scene in scene_list:
        folder = os.path.join(FLAGS.data_root, base_path + scene)
        image_infos.append([[folder, os.path.join(folder, 'images'), scene], 'preprocessed'])
    run_eval_pc(FLAGS.savepath, image_infos, **_run_options(FLAGS))


def cli(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--data_root', type=str, default=FLAGS.data_root)
    parser.add_argument('--savepath', type=str, default=FLAGS.savepath)
    parser.add_argument('--pretrained_model_ckpt_path', type=str, default=FLAGS.pretrained_model_ckpt_path)
    parser.add_argument('--view_num', type=int, default=8)
    parser.add_argument('--max_d', type=int, default=128)
    parser.add_argument('--max_w', type=int, default=FLAGS.max_w)
    parser.add_argument('--max_h', type=int, default=FLAGS.max_h)
    parser.add_argument('--gpu_id', type=int, default=FLAGS.gpu_id)
    parser.add_argument('--scenes', type=str, default=None, help='comma-separated scene folders under data_root/eth3d/')
    parser.add_argument('--synthetic_weights', action='store_true')
    parser.add_argument('--write_upsampled', action='store_true')
    parser.add_argument('--eager', action='store_true')
    parser.add_argument('--maps_in_flight', choices=('serial', 'cu_split'), default='serial',
                        help='serial: one depth map on the GPU at a time (default); cu_split: the two queued depth maps run concurrently, '
                             'each on its own half of every XCD (example.cu_split_streams: no SIMD shared between them; same bits, '
                             'more depth maps per second, twice the latency of one)')
    parser.add_argument('--scene_cache', action='store_true',
                        help='prepare each image on the GPU and run the 2-D towers on it once per scene; maps are assembled from '
                             'the cached features (atvsnet/scene.py); files are written by a background thread')
    parser.add_argument('--sync_write', action='store_true', help='--scene_cache: write the files in the driver thread')
    parser.add_argument('--fuse', action='store_true',
                        help='stage every depth map on the GPU as it is finished and end each scene with <savepath>/<scene>/'
                             'final3d_model.ply, the point cloud depth_fusion makes from the written files (depth_fusion.SceneFusion)')
    parser.add_argument('--prob_threshold', type=float, default=0.8, help='--fuse: depth_fusion --prob_threshold')
    parser.add_argument('--disp_threshold', type=float, default=0.01, help='--fuse: depth_fusion --disp_threshold')
    parser.add_argument('--num_consistent', type=float, default=2, help='--fuse: depth_fusion --num_consistent')
    parser.add_argument('--no_map_files', action='store_true',
                        help='--fuse: do not write the per-map files of depths_atvsnet/ (zz_runtime.txt is still written)')
    parser.add_argument('--fuse_normals', choices=depth_fusion.NORMAL_SOURCES, default=None,
                        help='--fuse: depth_fusion --normals (depth: normals estimated from each depth map on the GPU, tested in the '
                             'fusion and written into final3d_model.ply; default fake)')
    parser.add_argument('--fuse_normal_threshold', type=float, default=None, metavar='DEG',
                        help='--fuse: depth_fusion --normal_threshold')
    parser.add_argument('--fuse_normal_step', type=int, default=None, metavar='S', help='--fuse: depth_fusion --normal_step')
    parser.add_argument('--fuse_normal_depth_gate', type=float, default=None, metavar='G',
                        help='--fuse: depth_fusion --normal_depth_gate')
    parser.add_argument('--gt_ply', type=str, default=None, metavar='FILE[,FILE...]',
                        help='--fuse: score each scene\'s fused cloud against these ground-truth PLY file(s) (eval_cloud: accuracy, '
                             'completeness, F-score; not the official ETH3D evaluator) into <savepath>/<scene>/cloud_eval.json')
    parser.add_argument('--register', action='store_true',
                        help='--gt_ply: align the fused cloud to the ground truth before scoring it (eval_cloud --register); '
                             'cloud_eval.json then carries the `registration` object')
    parser.add_argument('--with_scale', action='store_true', help='--register: fit the scale too')
    parser.add_argument('--init_cameras', default=None, nargs=2, metavar=('RECON_SPARSE', 'GT_SPARSE'),
                        help='--register: two COLMAP sparse model folders of the same images (the scene\'s own and one in the '
                             'ground truth\'s frame); their camera centres give the initial similarity')
    parser.add_argument('--register_icp', default=None, choices=('point', 'plane'),
                        help='--register: point-to-point ICP (the default) or point-to-plane over the fused cloud\'s normals '
                             '(eval_cloud --register_icp); plane needs --fuse_normals depth, or --register_normals target')
    parser.add_argument('--register_normals', default=None, choices=('source', 'target'),
                        help='--register_icp plane: the planes of the fused cloud (source, the default) or of the ground truth, whose '
                             'normals are estimated on the GPU (target: no --fuse_normals depth needed; eval_cloud --register_normals)')
    parser.add_argument('--register_normal_k', type=int, default=None, metavar='K',
                        help='--register_normals target: eval_cloud --register_normal_k')
    parser.add_argument('--register_normal_radius', type=float, default=None, metavar='R',
                        help='--register_normals target: eval_cloud --register_normal_radius')
    eval_cloud.add_global_arguments(parser)
    parser.add_argument('--score_maps', action='store_true',
                        help='--gt_ply: render the ground truth into the scene\'s cameras and score the depth maps that entered the '
                             'cloud against it (eval_depth: mae, rmse, ..., inlier ratios per map; a point splat, not ETH3D\'s '
                             'renderer) into <savepath>/<scene>/depth_eval.json; with --register the matrix found is used')
    parser.add_argument('--map_splat', type=int, default=eval_depth.DEFAULT_SPLAT,
                        help='--score_maps: half-width of the occlusion window in pixels, 0..4')
    parser.add_argument('--map_occlusion_tol', type=float, default=eval_depth.DEFAULT_OCCLUSION_TOL,
                        help='--score_maps: a pixel is kept when its depth is within (1 + this) of the nearest in its window')
    parser.add_argument('--map_pixel_centre', type=float, default=eval_depth.DEFAULT_PIXEL_CENTRE,
                        help='--score_maps: image coordinate of the centre of pixel (0,0): 0 (the fusion\'s) or 0.5 (the plane sweep\'s)')
    parser.add_argument('--map_occlusion_mesh', default=None, metavar='FILE[,FILE...]',
                        help='--score_maps: triangle-mesh PLY file(s) in the ground truth\'s frame; a rendered ground-truth pixel that '
                             'lies behind them is taken out (eval_depth --occlusion_mesh)')
    parser.add_argument('--map_occlusion_mesh_tol', type=float, default=None, metavar='E',
                        help='--map_occlusion_mesh: a pixel is kept when its depth is within (1 + this) of the mesh\'s (default %g)'
                             % eval_depth.DEFAULT_OCCLUDER_TOL)
    clean_cloud.add_options(parser, 'clean_')
    parser.add_argument('--clean_keep_normals', action='store_true',
                        help='--fuse_normals depth with a cleaning step: final3d_model_clean.ply carries the normals of the rows that '
                             'stay (clean_cloud --keep_normals)')
    parser.add_argument('--mesh_voxel', type=float, default=None, metavar='V',
                        help='--fuse: also mesh each scene (mesh_fusion.SceneMesh: TSDF fusion of the staged maps with voxels of this '
                             'edge, marching tetrahedra) into <savepath>/<scene>/final3d_mesh.ply and mesh.json')
    parser.add_argument('--mesh_trunc_voxels', type=float, default=None, metavar='T',
                        help='--mesh_voxel: the band either side of a depth, in voxels (default 4: a default, not a measurement)')
    parser.add_argument('--mesh_min_weight', type=float, default=None, metavar='W',
                        help='--mesh_voxel: views a voxel needs to be meshed (default 2, the fusion\'s num_consistent)')
    parser.add_argument('--mesh_max_blocks', type=int, default=None, metavar='N',
                        help='--mesh_voxel: blocks of 8^3 voxels the maps may mark (default 131072)')
    clean_mesh.add_options(parser, 'mesh_clean_')
    parser.add_argument('--mesh_carve', type=float, nargs='?', default=None, const=1.0, metavar='CW',
                        help='--mesh_voxel: free-space carving (mesh_fusion --carve): a view that sees past a voxel votes it outside '
                             'with this weight (given bare: 1.0, a default, not a measurement); mesh.json gains carve_weight, '
                             'free_voxels and max_free')
    parser.add_argument('--mesh_render', action='store_true',
                        help='--mesh_voxel: render the mesh into the scene\'s map cameras (ops.mesh_render) as '
                             '<savepath>/<scene>/depths_mesh/%%08d_mesh.pfm; mesh.json gains `render`')
    args = parser.parse_args(argv)
    # what only the command line can break; the rest is _option_rules
    if (args.with_scale or args.init_cameras) and not args.register:
        parser.error('--with_scale and --init_cameras need --register')
    if args.register_icp is not None and not args.register:
        parser.error('--register_icp needs --register')
    if (args.register_normals, args.register_normal_k, args.register_normal_radius) != (None, None, None) and not args.register:
        parser.error('--register_normals, --register_normal_k and --register_normal_radius need --register')
    if args.register_normal_k is not None and not 2 <= args.register_normal_k <= 32:
        parser.error('--register_normal_k must be in 2..32')
    if args.register_normal_radius is not None and not (args.register_normal_radius > 0.0 and np.isfinite(args.register_normal_radius)):
        parser.error('--register_normal_radius must be positive and finite')
    if args.register_global and not args.register:
        parser.error('--register_global needs --register')
    for name in eval_cloud.GLOBAL_FLAGS:
        if getattr(args, name) not in (None, False) and not args.register_global:
            parser.error('--%s needs --register_global' % name)
    if any(v is not None and not (v > 0.0 and np.isfinite(v)) for v in (args.global_voxel, args.global_tau)):
        parser.error('--global_voxel and --global_tau must be positive and finite')
    if args.global_hypotheses is not None and not 1 <= args.global_hypotheses <= 1 << 24:
        parser.error('--global_hypotheses must be in 1..2^24')
    if args.global_seed is not None and args.global_seed < 0:
        parser.error('--global_seed must be >= 0')
    if not args.score_maps and (args.map_splat != eval_depth.DEFAULT_SPLAT or args.map_occlusion_tol != eval_depth.DEFAULT_OCCLUSION_TOL
                                or args.map_pixel_centre != eval_depth.DEFAULT_PIXEL_CENTRE):
        parser.error('--map_splat, --map_occlusion_tol and --map_pixel_centre need --score_maps')
    if not args.score_maps and (args.map_occlusion_mesh is not None or args.map_occlusion_mesh_tol is not None):
        parser.error('--map_occlusion_mesh and --map_occlusion_mesh_tol need --score_maps')
    if args.map_occlusion_mesh_tol is not None and args.map_occlusion_mesh is None:
        parser.error('--map_occlusion_mesh_tol needs --map_occlusion_mesh')
    if args.map_occlusion_mesh_tol is not None and not (args.map_occlusion_mesh_tol >= 0.0 and np.isfinite(args.map_occlusion_mesh_tol)):
        parser.error('--map_occlusion_mesh_tol must be >= 0 and finite')
    if args.map_occlusion_mesh is not None and not [p for p in args.map_occlusion_mesh.split(',') if p]:
        parser.error('--map_occlusion_mesh names no file')
    if args.mesh_render and args.mesh_voxel is None:
        parser.error('--mesh_render needs --mesh_voxel')
    if args.mesh_carve is not None and args.mesh_voxel is None:
        parser.error('--mesh_carve needs --mesh_voxel')
    if clean_mesh.options(parser, args, 'mesh_clean_') and args.mesh_voxel is None:
        parser.error('--mesh_clean_min_faces, --mesh_clean_min_ratio and --mesh_clean_keep_largest need --mesh_voxel')
    if not 0 <= args.map_splat <= 4:
        parser.error('--map_splat must be in 0..4')
    if not (args.map_occlusion_tol >= 0.0 and np.isfinite(args.map_occlusion_tol)) or not np.isfinite(args.map_pixel_centre):
        parser.error('--map_occlusion_tol must be >= 0 and finite, --map_pixel_centre finite')
    args.gt_ply = [p for p in args.gt_ply.split(',') if p] if args.gt_ply else None
    args.clean = clean_cloud.options(parser, args, 'clean_') or None
    try:
        _check_options(**_run_options(args))
        depth_fusion.check_normal_options(**(_normal_options(args) or {}))
        if _mesh_options(args) is not None:
            from . import mesh_fusion
            mesh_fusion.check_options(**_mesh_options(args))
    except ValueError as e:
        parser.error(str(e))
    scenes = args.scenes.split(',') if args.scenes else None
    _Pipelines.CO_RESIDENT = 'cu_split' if args.maps_in_flight == 'cu_split' else False
    for k, v in vars(args).items():
        if k not in ('scenes', 'maps_in_flight'):
            setattr(FLAGS, k, v)
    print('Evaluate A-TVSNet pointcloud with %d views' % (FLAGS.view_num))
    main(scenes)


if __name__ == '__main__':
    cli()
