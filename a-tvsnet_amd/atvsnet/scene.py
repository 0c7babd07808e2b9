"""Scene mode: every image of a scene prepared on the GPU and run through both 2-D towers ONCE; each depth map is assembled from
cached features (eval_pointcloud --scene_cache).

In an ETH3D pair.txt scene every image is the reference of one depth map and a source of about seven others.  The per-map path
(eth3d_inputs.load_data + GraphedInference) decodes, resizes and centres each image, and runs the towers on it, once per map it
appears in.  Here:

* the image is decoded once and uploaded as uint8; ops.prepare_view resizes it by the map's adaptive scale, crops and centres it,
  and forms the 1/4-scale image (bit for bit scale_image; the centring may differ from center_image in the last bits);
* one captured graph per (image shape, output shape, slot) runs preparation + both towers (pipeline.multiview_towers at N = 1:
  every tower has per-image statistics, so a row does not depend on the other images of a launch);
* the cache maps (image id, adaptive scale, crop window) -> (features, shallow features, 1/4 image), and image id -> the device
  uint8 image, bounded in bytes with LRU eviction;
* each map replays a features-mode graph (graphs.GraphedInference(features=True)) from PipelinedInference's slots.

Range rule: a map whose replay or whose newly computed tower features raised the non-finite flag is
recomputed entirely on the fp32 kernels from the uint8 images (what ops.configure(split16=False) computes for it), and the cache
entries its submission made are dropped.  Entries belong to the weights they were computed with: a change of the variable store
clears the cache and the captured graphs.
"""
from __future__ import print_function

import collections
import gc
import math
import time
import weakref

import numpy as np
import torch

from .. import ops, variables
from ..flags import FLAGS
from . import graphs, pipeline, range_guard
from .preprocess import crop_window, scaled_size


def pad_views(views, view_num):
    """A pair.txt entry's views (reference first) -> exactly view_num of them: missing sources are the reference (load_data)."""
    views = list(views)[:view_num]
    return views + [views[0]] * (view_num - len(views))


def adaptive_scale(shapes, max_h=None, max_w=None):
    """load_data's resize_scale of a map whose views have `shapes` [(h, w), ...] (FLAGS.adaptive_scaling); None if an image is
    smaller than max_h x max_w (load_data exits then)."""
    if not FLAGS.adaptive_scaling:
        return 1
    max_h = FLAGS.max_h if max_h is None else max_h
    max_w = FLAGS.max_w if max_w is None else max_w
    h_scale = max(float(max_h) / s[0] for s in shapes)
    w_scale = max(float(max_w) / s[1] for s in shapes)
    if h_scale > 1 or w_scale > 1:
        return None
    return max(h_scale, w_scale)


def view_key(image_id, scale, crop):
    """Cache key of one prepared view."""
    return (image_id, float(scale), tuple(int(v) for v in crop))


def tensor_bytes(*ts):
    return sum(int(t.numel()) * t.element_size() for t in ts)


class ViewCache(object):
    """key -> value with a byte bound and least-recently-used eviction; cleared when the weights change (`generation`).
    The most recent entry is always kept, even alone above the bound."""

    def __init__(self, max_bytes):
        self.max_bytes = int(max_bytes)
        self.items = collections.OrderedDict()          # key -> (value, bytes)
        self.bytes = 0
        self.generation = None
        self.evictions = 0

    def check_generation(self, generation):
        """Clear if the weights changed since the entries were made; True if it cleared."""
        if generation == self.generation:
            return False
        self.clear()
        self.generation = generation
        return True

    def get(self, key):
        item = self.items.get(key)
        if item is None:
            return None
        self.items.move_to_end(key)
        return item[0]

    def put(self, key, value, nbytes):
        self.drop(key)
        self.items[key] = (value, int(nbytes))
        self.bytes += int(nbytes)
        while self.bytes > self.max_bytes and len(self.items) > 1:
            _, (_, b) = self.items.popitem(last=False)
            self.bytes -= b
            self.evictions += 1

    def drop(self, key):
        item = self.items.pop(key, None)
        if item is not None:
            self.bytes -= item[1]

    def clear(self):
        self.items.clear()
        self.bytes = 0

    def __contains__(self, key):
        return key in self.items

    def __len__(self):
        return len(self.items)


class _Entry(object):
    """Device tensors made on `stream`, complete at `event`."""
    __slots__ = ('tensors', 'stream', 'event')

    def __init__(self, tensors, stream):
        self.tensors, self.stream = tensors, stream
        self.event = torch.cuda.Event()
        self.event.record(stream)

    def use(self, stream):
        """Make the tensors usable on `stream` (an event wait between two side streams: no default-stream operation)."""
        if stream != self.stream:
            stream.wait_event(self.event)
            for t in self.tensors:
                t.record_stream(stream)
        return self.tensors


class _TowerGraph(object):
    """ops.prepare_view + pipeline.multiview_towers of one image, captured for one (source shape, output shape); the taps are
    static inputs, so one graph serves every scale / crop with those shapes."""

    def __init__(self, plan, scale, crop, sample_scale, device):
        self.image = torch.zeros(plan.src_shape, dtype=torch.uint8, device=device)
        self.ws = (torch.empty(plan.shape, dtype=torch.float32, device=device),
                   torch.empty(plan.quarter_shape, dtype=torch.uint8, device=device)) + ops.prepare_workspace(plan, device)
        self.args = (scale, crop, sample_scale)
        torch.cuda.current_stream(device).wait_event(plan.ready)
        self.taps = [t.clone() for t in plan.taps]
        self.graph, self.out, self._weights = graphs.capture(self._run, device)

    def _run(self):
        scale, crop, sample_scale = self.args
        centred, quarter = ops.prepare_view(self.image, scale, crop, sample_scale, out=self.ws, taps=self.taps)
        feats, shallow = pipeline.multiview_towers(centred.view((1, 1) + tuple(centred.shape)))
        return feats, shallow, quarter

    def __call__(self, image, plan):
        self.image.copy_(image)
        for d, t in zip(self.taps, plan.taps):
            d.copy_(t)
        self.graph.replay()
        return self.out


class _Slot(object):
    """What a slot of a pipeline holds: the map's views, adaptive scale and crops, the cache keys its submission made (`new`),
    the reference's 1/4-scale image (`quarter`) and the (start, end) timing events."""
    __slots__ = ('views', 'scale', 'crops', 'new', 'quarter', 'events')


class SceneInference(object):
    """Depth maps of one or more scenes from cached per-image features.

        scene = SceneInference(loader, max_d, slots=2, co_resident=False)
        scale, crops = scene.layout(views)               # views: image ids, reference first, padded to view_num
        t = scene.submit(views, cams)                    # cams (1,N,2,4,4) at FLAGS.sample_scale, host or device
        depth, depth_up, prob, prob_up = scene.result(t, host=True)
        quarter = scene.reference_image(t)               # the reference's 1/4-scale uint8 BGR image (host)

    loader(image_id) -> (h,w,3) uint8 BGR numpy; shape(image_id) -> (h, w) (defaults to the loader's image).  Slot semantics
    are PipelinedInference's (slots, co_resident False | 'cu_split', result(host=True)).  In cu_split mode nothing runs on the
    default stream between submissions once every (views, crop size) has been captured: image and tap uploads (from pinned
    memory), tower replays and feature copies run on the slot's stream.
    Instrumentation: times['upload'] (host seconds spent issuing image uploads), gpu_ms (per fetched map: its GPU time on the
    slot's stream, from after the slot's ordering waits to the end of its replay)."""

    def __init__(self, loader, max_d=None, slots=2, co_resident=False, max_bytes=4 << 30, device=None, shape=None,
                 sample_scale=None, view_num=None):
        if co_resident not in (False, 'cu_split'):
            raise ValueError("SceneInference: co_resident is False or 'cu_split'")
        self.loader, self._shape_fn = loader, shape
        self.max_d = FLAGS.max_d if max_d is None else max_d
        self.view_num = FLAGS.view_num if view_num is None else view_num
        self.sample_scale = FLAGS.sample_scale if sample_scale is None else sample_scale
        self.slots, self.co_resident = slots, co_resident
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.cache = ViewCache(max_bytes)
        self.shapes = {}
        self.tower_runs = 0
        self.times, self.gpu_ms = {'upload': 0.0}, []
        self.streams = graphs.cu_split_streams(self.device, slots) if co_resident == 'cu_split' else None
        self._reset()

    def _reset(self):
        self.towers, self.pipelines = {}, {}
        self.slot = {}                                     # (id(pipeline), slot) -> _Slot
        self.last = None                                   # (pipeline, slot) of the latest submission

    def _check_weights(self):
        if self.cache.check_generation(variables.default_store().generation) and self.cache.generation is not None:
            self._reset()                                  # graphs hold the weights they were captured with

    def shape(self, image_id):
        s = self.shapes.get(image_id)
        if s is None:
            s = tuple(self._shape_fn(image_id)) if self._shape_fn is not None else tuple(self.loader(image_id).shape[:2])
            self.shapes[image_id] = s
        return s

    def layout(self, views):
        """(adaptive scale, [crop window per view]) of a map; ValueError if an image is smaller than max_h x max_w."""
        shapes = [self.shape(v) for v in views]
        scale = adaptive_scale(shapes)
        if scale is None:
            raise ValueError('max_h, max_w should < W and H! (views %s)' % (shapes,))
        return scale, [crop_window(*scaled_size(h, w, scale)) for h, w in shapes]

    def room(self):
        return sum(p.in_flight() for p in self.pipelines.values()) < self.slots

    # -- device images and cache entries ------------------------------------------------------------------------------------
    def _device_image(self, image_id, stream):
        key = ('image', image_id)
        e = self.cache.get(key)
        if e is None:
            host = torch.from_numpy(np.ascontiguousarray(self.loader(image_id), dtype=np.uint8))
            t0 = time.time()
            with torch.cuda.stream(stream):
                # from pinned memory: the copy is queued on the slot's stream and the host does not wait for the map in flight
                img = host.pin_memory().to(self.device, non_blocking=True)
                e = _Entry((img,), stream)
            self.times['upload'] += time.time() - t0
            self.shapes[image_id] = tuple(img.shape[:2])
            self.cache.put(key, e, tensor_bytes(img))
        return e.use(stream)[0]

    def _tower_graph(self, plan, scale, crop, slot):
        key = (plan.src_shape, plan.shape, plan.quarter_shape, slot)
        g = self.towers.get(key)
        if g is None:
            gc.collect()
            g = self.towers[key] = _TowerGraph(plan, scale, crop, self.sample_scale, self.device)
        return g

    def _pipeline(self, n, H, W, cams):
        key = (n, H, W)
        p = self.pipelines.get(key)
        if p is None:
            gc.collect()                                    # no unreachable graph of an earlier run may be freed during the capture
            h, w = int(math.ceil(H / 4.0)), int(math.ceil(W / 4.0))
            feats = (torch.zeros((n, h, w, 32), device=self.device), torch.zeros((n, h, w, 16), device=self.device))
            # weak references only: a cycle scene -> pipeline -> graph -> scene would leave the captured graphs to the cyclic garbage
            # collector, which may then destroy one in the middle of a later capture (not permitted while a stream is capturing)
            me = weakref.ref(self)
            p = graphs.PipelinedInference(feats, cams.to(self.device, torch.float32), self.max_d, slots=self.slots,
                                          co_resident=self.co_resident, out_prob_map=True, features=True,
                                          streams=self.streams,   # every shape's slot k on the same CU share
                                          fp32_fn=lambda s: me()._fp32_map(pw(), s))
            pw = weakref.ref(p)                             # what fp32_fn finds when a map is rerun
            self.pipelines[key] = p
        return p

    # -- submission ---------------------------------------------------------------------------------------------------------
    def submit(self, views, cams):
        """Issue the depth map of `views` (image ids, reference first; fewer than view_num: padded with the reference) with
        cameras `cams` (1,N,2,4,4); returns the ticket."""
        self._check_weights()
        views = pad_views(views, self.view_num)
        scale, crops = self.layout(views)
        sizes = set((c[2], c[3]) for c in crops)
        if len(sizes) != 1:
            raise ValueError('SceneInference: the views of a map crop to different sizes %s' % sorted(sizes))
        cams = cams if isinstance(cams, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cams, dtype=np.float32))
        p = self._pipeline(len(views), crops[0][2], crops[0][3], cams)
        slot, stream = p.next_slot()
        with torch.cuda.stream(stream):                     # a new (size, scale, crop) uploads its taps on the slot's stream
            plans = [ops.view_plan(self.shape(v)[0], self.shape(v)[1], scale, c, self.sample_scale, self.device)
                     for v, c in zip(views, crops)]
        for v, c, plan in zip(views, crops, plans):         # first use of a shape: capture now, not inside the slot's stream
            if view_key(v, scale, c) not in self.cache:
                self._tower_graph(plan, scale, c, slot)
        last = self.last
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def fill(s):
            st = torch.cuda.current_stream(self.device)
            if not self.co_resident and last is not None and last[0] is not p and last[0].busy[last[1]]:
                st.wait_event(last[0].events[last[1]])      # one depth map on the GPU at a time, across shapes too
            start.record(st)
            if host_cams is not None:                       # pinned: queued on the slot's stream, the host does not wait
                p.graphs[s].cams.copy_(host_cams, non_blocking=True)
            feats, shallow = p.graphs[s].images
            rec = self.slot[(id(p), s)] = _Slot()
            rec.views, rec.scale, rec.crops, rec.new, rec.quarter = views, scale, crops, [], None
            for i, (v, c, plan) in enumerate(zip(views, crops, plans)):
                key = view_key(v, scale, c)
                e = self.cache.get(key)
                if e is None:
                    img = self._device_image(v, st)
                    st.wait_event(plan.ready)
                    f, sh, q = self._tower_graph(plan, scale, c, s)(img, plan)
                    e = _Entry((f.clone(), sh.clone(), q.clone()), st)
                    self.cache.put(key, e, tensor_bytes(*e.tensors))
                    rec.new.append(key)
                    self.tower_runs += 1
                f, sh, q = e.use(st)
                feats[i].copy_(f[0])
                shallow[i].copy_(sh[0])
                if i == 0:
                    rec.quarter = q

        host_cams = None if cams.is_cuda else cams.to(torch.float32).contiguous().pin_memory()
        s = p.submit(None, cams if cams.is_cuda else None, fill=fill)
        end.record(p.streams[s])
        self.slot[(id(p), s)].events = (start, end)
        self.last = (p, s)
        return (p, s)

    def result(self, ticket, host=False):
        """The (depth, depth_up, prob, prob_up) of `ticket` (PipelinedInference.result: an overflowed map comes back computed on
        the fp32 kernels); the cache entries of every map found suspect are dropped.  The non-finite flag is device-wide: when it
        is found up, every map in flight in ANY of the scene's pipelines (one per crop size) becomes suspect."""
        p, s = ticket
        if not p.busy[s]:
            raise RuntimeError('SceneInference: nothing in flight on slot %d' % s)
        p.events[s].synchronize()
        queues = list(self.pipelines.values())
        if p not in queues:
            queues.append(p)                                 # reset away (new weights) with this map still in flight
        with torch.cuda.stream(p.streams[s]):                # the flag read: on the slot's (idle) stream
            range_guard.mark_suspects(self.device, queues)
        for q in queues:
            for t in q.suspect:
                self._drop_new(q, t)                         # made while the flag was up: never reused
        out = p.result(s, host=host)
        rec = self.slot[(id(p), s)]
        (start, end), rec.events = rec.events, None
        end.synchronize()
        self.gpu_ms.append(start.elapsed_time(end))
        return out

    def reference_image(self, ticket, host=True):
        """The reference view's sample_scale uint8 BGR image of `ticket`'s map (host numpy; after result()).  host=False: the
        device tensor, valid until the slot's next submission -- use it on slot_stream(ticket)."""
        p, s = ticket
        if not host:
            return self.slot[(id(p), s)].quarter
        with torch.cuda.stream(p.streams[s]):
            return self.slot[(id(p), s)].quarter.cpu().numpy()

    def slot_stream(self, ticket):
        """The stream `ticket`'s map runs on: work enqueued there after result() precedes the slot's next submission."""
        p, s = ticket
        return p.streams[s]

    def _drop_new(self, p, s):
        """Forget the cache entries that the submission now in slot s of p made (once: the list is consumed)."""
        rec = self.slot.get((id(p), s))
        while rec is not None and rec.new:
            self.cache.drop(rec.new.pop())

    def _fp32_map(self, p, s):
        """The map now in slot s, computed entirely on the fp32 kernels from the uint8 images (towers included)."""
        rec = self.slot[(id(p), s)]
        views, scale, crops = rec.views, rec.scale, rec.crops
        self._drop_new(p, s)                                 # made while the flag was up
        st = torch.cuda.current_stream(self.device)
        with ops.configure(split16=False):
            imgs = torch.stack([ops.prepare_view(self._device_image(v, st), scale, c, self.sample_scale)[0]
                                for v, c in zip(views, crops)], 0)[None]
            out = pipeline.infer_multiview(imgs, p.graphs[s].cams, self.max_d, out_prob_map=True)
        if ops.nonfinite_seen(self.device):
            raise range_guard.fp32_nonfinite('a batch norm saw non-finite moments')
        return out
