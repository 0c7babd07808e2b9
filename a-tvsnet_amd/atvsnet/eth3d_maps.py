"""The ETH3D driver's map loop (reference eval_pointcloud.py :291-396): _run_scene takes the depth maps of one scene from a map source
-- _PipelineSource (load_data's host arrays through _Pipelines' captured HIP graphs) or _SceneSource (--scene_cache: atvsnet/scene.py)
-- and hands each to _write_map through a _Writer; TIMES holds the host time of the last scene.  eval_pointcloud owns the rest."""
import os
import time

import numpy as np
import torch

from ..flags import FLAGS
from . import depth_fusion, example, graphs, pipeline, range_guard, scene
from .eth3d_inputs import _view_paths, load_cams, load_data
from .preprocess import write_cam, write_pfm


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
