"""Capture and queuing: the depth-map pipelines of atvsnet/pipeline.py captured in HIP graphs (GraphedInference) and queued
over slots, one graph and one stream each (PipelinedInference; cu_split_streams gives every slot its own compute units)."""
import ctypes
import functools

import torch

from .. import ops, variables
from ..flags import FLAGS
from ..tools.common import Notify
from .pipeline import BATCHED, infer_multiview, infer_multiview_from_features, infer_twoview
from .range_guard import _log_fp32_fallback, fp32_nonfinite, mark_suspects


def warm_up(fn, device):
    """fn() once on a fresh side stream, joined back, the device idle afterwards: weight packing / uploads and function
    attributes happen here, not inside a capture."""
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)


def pinned_weights():
    """A graph holds raw pointers to the weights it was captured with: whoever owns one keeps these copies alive even if the
    variable store is reloaded afterwards (the graph then goes on computing with the captured weights)."""
    return (ops.cache_snapshot(), variables.default_store().device_snapshot())


def capture(fn, device, pool=None):
    """fn() captured in a HIP graph after a warm_up: -> (graph, fn's outputs in the graph's static memory, pinned_weights())."""
    warm_up(fn, device)
    graph = torch.cuda.CUDAGraph()
    # thread_local: other threads (e.g. the RCCL watchdog of a multi-GPU run) may issue HIP calls meanwhile
    with torch.cuda.graph(graph, pool=pool, capture_error_mode='thread_local'):
        out = fn()
    return graph, out, pinned_weights()


class GraphedInference(object):
    """The whole depth-map pipeline captured once in a HIP graph and replayed per depth map.

    Eager execution issues ~2000 kernel launches per depth map from Python (~20 us each), which is
    close to the GPU time of the step; a captured graph (all shapes are static for a given
    (views, H, W, D)) replays them -- including the per-view stream fork/join -- with one host call.
    Inputs live in static device buffers: pass new images / cams to __call__ to overwrite them.
    """

    def __init__(self, images, cams, max_d=None, view_streams=True, out_prob_map=False, batched=None, features=False, fp32_fn=None):
        """features=True: `images` is (features (N,h,w,32), shallow features (N,h,w,16)) of the N views and the graph is the
        pipeline after the towers (infer_multiview_from_features; the scene driver, atvsnet/scene.py).  fp32_fn: what
        fp32_rerun returns instead of replaying an fp32 capture of this graph (scene mode recomputes the towers too)."""
        self.max_d = FLAGS.max_d if max_d is None else max_d
        self.split16 = bool(ops.cfg.split16)    # the kernels this graph was captured with (a replay ignores later switches)
        self._fp32 = None                       # the same pipeline captured on the fp32 matrix cores, built on first need
        self.fp32_fn = fp32_fn
        self.out_prob_map = out_prob_map
        self.batched = BATCHED if batched is None else batched
        self.features = bool(features)
        self.images = tuple(t.clone() for t in images) if self.features else images.clone()
        self.cams = cams.clone()
        self.twoview = not self.features and images.shape[1] == 2
        self.view_streams = view_streams
        self.graph, self.out, self._weights = capture(self._run, cams.device)

    def _run(self):
        if self.features:
            return infer_multiview_from_features(self.images[0], self.images[1], self.cams, self.max_d, out_prob_map=self.out_prob_map)
        if self.twoview:
            return infer_twoview(self.images, self.cams, self.max_d, batched=self.batched)
        return infer_multiview(self.images, self.cams, self.max_d, view_streams=self.view_streams,
                               out_prob_map=self.out_prob_map, batched=self.batched)

    def __call__(self, images=None, cams=None):
        if images is not None:
            if self.features:
                for d, t in zip(self.images, images):
                    d.copy_(t)
            else:
                self.images.copy_(images)
        if cams is not None:
            self.cams.copy_(cams)
        self.graph.replay()
        return self.out

    def checked(self, images=None, cams=None):
        """__call__, then wait for the depth map; if a batch norm of this replay saw non-finite moments (an fp16-range overflow
        of the split-operand kernels) THAT map is recomputed on the fp32 matrix cores (`fp32_rerun`) and the fp32 result is
        returned -- the reference is fp32 end to end (cnn_wrapper/network.py:165-167, 570-601), a drop-in must not need a
        user action to have fp32's range.  FloatingPointError only if the fp32 kernels see non-finite values too."""
        out = self(images, cams)
        if ops.nonfinite_seen(self.cams.device):
            out = self.fp32_rerun()
        return out

    def fp32_rerun(self):
        """The depth map of the inputs now in this graph's static buffers on the fp32-MFMA kernels: a second captured graph
        (built once, in this process -- never a re-exec of a process that has touched the GPU), replayed synchronously.
        Raises FloatingPointError if this graph already IS the fp32 form or the fp32 kernels see non-finite moments too."""
        dev = self.cams.device
        if not self.split16:
            raise fp32_nonfinite('a batch norm saw non-finite moments', too=False)
        _log_fp32_fallback()
        if self.fp32_fn is not None:
            return self.fp32_fn()
        if self._fp32 is None:
            with ops.configure(split16=False):
                self._fp32 = GraphedInference(self.images, self.cams, self.max_d, view_streams=self.view_streams,
                                              out_prob_map=self.out_prob_map, batched=self.batched, features=self.features)
            ops.nonfinite_seen(dev)            # the capture's warm-up ran on the inputs too: start from a clear flag
        out = self._fp32(self.images, self.cams)
        if ops.nonfinite_seen(dev):
            raise fp32_nonfinite('a batch norm saw non-finite moments')
        return out


_hip_runtime = None


def cu_split_streams(device, parts):
    """`parts` HIP streams whose kernels run on DISJOINT sets of compute units: part k of every XCD (hipExtStreamCreateWithCUMask;
    mask bit i = CU i / 8 of XCD i % 8 on MI355X, so part k owns the CUs with (i / 8) % parts == k -- an equal share of every
    XCD, of its L2 and of the memory channels behind it).  Kernels of different streams then never share a CU, hence never a
    SIMD: the one condition of the co-residency fault cannot arise between them.
    (Masks that leave an XCD without a CU -- "even / odd bits" -- are not honoured by the runtime: the stream then runs on the whole
    chip.  tests/test_gpu_pipeline.py checks that a stream of this function really is confined.)  The streams live as long as the
    process (a handful per process; nothing to free in a driver run)."""
    global _hip_runtime
    props = torch.cuda.get_device_properties(device)
    ncu, nxcd = int(props.multi_processor_count), 8
    if parts < 1 or ncu % nxcd or (ncu // nxcd) < parts:
        raise ValueError('cu_split_streams: %d parts of %d compute units' % (parts, ncu))
    if _hip_runtime is None:
        # the HIP runtime torch has ALREADY loaded (a stream of a second copy of the runtime would mean nothing to torch): its path from
        # this process's mappings, the soname as a fallback (dlopen returns the loaded instance for a matching soname)
        path = 'libamdhip64.so'
        try:
            with open('/proc/self/maps') as f:
                for ln in f:
                    if 'libamdhip64.so' in ln:
                        path = ln.split()[-1]
                        break
        except OSError:
            pass
        _hip_runtime = ctypes.CDLL(path)
    out = []
    with torch.cuda.device(device):
        for k in range(parts):
            words = (ctypes.c_uint32 * ((ncu + 31) // 32))()
            for i in range(ncu):
                if (i // nxcd) % parts == k:
                    words[i // 32] |= (1 << (i % 32))
            st = ctypes.c_void_p()
            rc = _hip_runtime.hipExtStreamCreateWithCUMask(ctypes.byref(st), len(words), words)
            if rc != 0 or not st.value:
                raise RuntimeError('hipExtStreamCreateWithCUMask failed (%d)' % rc)
            out.append(torch.cuda.ExternalStream(st.value, device=device))
    return out


class PipelinedInference(object):
    """`slots` depth maps queued: one captured graph (static buffers) and one HIP stream per slot.

    The depth maps of a scene are independent (one per reference view, reference eval_pointcloud.py:399-424).
    `co_resident=False` (default): a slot's graph starts when the previously submitted one has finished -- the GPU runs
    ONE depth map at a time, bit for bit the single-map path, and what the queue buys is that the host prepares and submits
    the next map (and writes the previous one's files) meanwhile.
    `co_resident=True`: the slots' graphs run concurrently on their streams; the second map's kernels fill the phases in
    which one pipeline leaves the GPU under-filled (+4.5 % depth maps/s at config 3).  Opt-in only: wavefronts of different
    kernels then share SIMDs, and on this pool's MI355X kernels with compiler-formed packed fp32 arithmetic on dwordx2-loaded
    operands have produced wrong lane quarters beside another kernel's 16x16x32 MFMA wavefronts (narrowed
    to that instruction form, cause not established; the kernels that still contain packed fp32 are pinned by
    tests/test_packed_fp32_census.py, and conv2d_b / conv1x1_b / bottleneck_b / deconv_up_b run two workgroups per CU, so
    nothing reserves their SIMDs).  bench.py measures it under `pipelined` and fails the run if a slot's output differs from
    the single-map output.
    `co_resident='cu_split'` (round 6): the slots' graphs run concurrently, each on its OWN share of every XCD's compute units
    (cu_split_streams): no SIMD ever holds wavefronts of two kernels, so the fault above cannot occur, and every slot still
    produces the single-map bits.  Two slots: +1.5 ... 4 % depth maps/s at config 3 (each map has half the chip; what is gained
    is the overlap of one map's launch tails and latency-bound kernels with the other's work), +19 % for two-view maps
    (configs[1]: 184 -> 218 maps/s); the latency of ONE map roughly doubles.  bench.py reports it under `pipelined_cu_split`.

        t = p.submit(images, cams)      # asynchronous: copies the inputs, replays the slot's graph on its stream
        out = p.result(t)               # waits for that depth map; the tensors are valid until the slot is re-used
    """

    def __init__(self, images, cams, max_d=None, slots=2, co_resident=False, streams=None, fp32_fn=None, **kw):
        """streams: the slots' streams, instead of new ones (the scene driver gives slot k of every shape the same CU share).
        fp32_fn(slot): what a slot's graph returns as its fp32 rerun (GraphedInference's fp32_fn, bound per slot)."""
        if slots < 1:
            raise ValueError('PipelinedInference: slots >= 1')
        self.device = cams.device
        self.cu_split, self.co_resident = self._mode(co_resident)
        self.last = None                 # slot of the most recent submission (its event orders the next one behind it)
        self.graphs = [GraphedInference(images, cams, max_d, fp32_fn=fp32_fn and functools.partial(fp32_fn, s), **kw)
                       for s in range(slots)]
        self.streams = self._new_streams(slots, self.cu_split) if streams is None else streams
        self.events = [torch.cuda.Event() for _ in range(slots)]
        self.busy = [False] * slots
        self.suspect = set()             # slots in flight when the non-finite flag was found set: their maps are recomputed in fp32
        self.next = 0
        self._warned = False

    @staticmethod
    def _mode(co_resident):
        """co_resident -> (cu_split, co_resident as a bool)."""
        if co_resident not in (False, True, 'cu_split'):
            raise ValueError("PipelinedInference: co_resident is False, True or 'cu_split'")
        return co_resident == 'cu_split', bool(co_resident)

    def _new_streams(self, slots, split):
        return cu_split_streams(self.device, slots) if split else [torch.cuda.Stream(self.device) for _ in range(slots)]

    @property
    def slots(self):
        return len(self.graphs)

    def next_slot(self):
        """(slot, its stream) of the next submission."""
        return self.next, self.streams[self.next]

    def in_flight(self):
        """How many slots hold an unfetched result."""
        return self.busy.count(True)

    def set_mode(self, co_resident):
        """Switch the way the slots share the GPU (False | True | 'cu_split') with nothing in flight: the captured graphs stay,
        the slots' streams are replaced."""
        if any(self.busy):
            raise RuntimeError('PipelinedInference.set_mode: results still in flight')
        split, co_resident = self._mode(co_resident)
        torch.cuda.synchronize(self.device)
        if split != self.cu_split:
            self.streams = self._new_streams(self.slots, split)
        self.cu_split, self.co_resident, self.last = split, co_resident, None

    def submit(self, images=None, cams=None, fill=None):
        """Issue one depth map on the next slot (its previous result must have been fetched); returns the ticket.
        images: a tensor, or the (features, shallow features) pair of a features-mode graph.  fill(slot): called on the slot's
        stream before the replay, after the slot's ordering waits (the scene driver computes and copies the views' features there)."""
        s = self.next
        if self.busy[s]:
            raise RuntimeError('PipelinedInference: slot %d still holds an unfetched result' % s)
        self.next = (s + 1) % len(self.graphs)
        st = self.streams[s]
        # inputs prepared on the caller's stream are ordered in front of the slot's work.  cu_split: the CU-masked streams are BLOCKING
        # streams in the legacy sense -- any operation on the default stream (an event record, a copy) waits for every map in flight
        # and holds the next one back, which serialises the slots (34 instead of 62 maps/s at configs[2]); so HOST tensors (or None)
        # are copied by the slot's own stream with no default-stream operation at all, and only device inputs pay for the ordering
        inputs = (list(images) if isinstance(images, (tuple, list)) else [images]) + [cams]
        if not self.cu_split or any(t is not None and t.is_cuda for t in inputs):
            cur = torch.cuda.current_stream(self.device)
            if self.cu_split and cur == torch.cuda.default_stream(self.device) and not self._warned:
                self._warned = True
                print(Notify.WARNING, "PipelinedInference(co_resident='cu_split'): device inputs prepared on the default stream order "
                      'every submission behind ALL maps in flight (the slots then run one after the other, each on its share of the '
                      'chip); pass host tensors or prepare the inputs on a side stream', Notify.ENDC)
            st.wait_stream(cur)
        if not self.co_resident and self.last is not None and self.last != s:
            st.wait_event(self.events[self.last])                   # one depth map on the GPU at a time
        for t in inputs:
            # the copy into the slot's static buffers runs on the slot's stream, possibly long after this call returns:
            # tell the caching allocator, or the caller's next allocation could re-use the block while it is still read
            if t is not None and t.is_cuda:
                t.record_stream(st)
        with torch.cuda.stream(st):
            if fill is not None:
                fill(s)
            self.graphs[s](images, cams)
            self.events[s].record(st)
        self.busy[s] = True
        self.last = s
        return s

    def result(self, ticket, host=False):
        """The depth map (tuple of outputs with out_prob_map) of `ticket`; host=True: as CPU tensors, copied by the slot's own stream
        (cu_split: the way to fetch results without an operation on the default stream, see submit)."""
        if not self.busy[ticket]:
            raise RuntimeError('PipelinedInference: nothing in flight on slot %d' % ticket)
        self.events[ticket].synchronize()
        with torch.cuda.stream(self.streams[ticket]):          # the flag read and the copies below: on the slot's (idle) stream
            self.busy[ticket] = False
            if mark_suspects(self.device, [self]):
                self.suspect.add(ticket)
            if ticket in self.suspect:
                self.suspect.discard(ticket)
                out = self.graphs[ticket].fp32_rerun()         # synchronous, from the slot's static input buffers
            else:
                out = self.graphs[ticket].out
            if host:
                out = tuple(o.cpu() for o in out) if isinstance(out, (tuple, list)) else out.cpu()
        return out

    def run(self, count):
        """Benchmark helper: `count` depth maps of the captured inputs, round-robin over the slots; returns when all are
        done (results are overwritten)."""
        for s, st in enumerate(self.streams):
            st.wait_stream(torch.cuda.current_stream(self.device))
        for i in range(count):
            s = i % len(self.graphs)
            if not self.co_resident and self.last is not None and self.last != s:
                self.streams[s].wait_event(self.events[self.last])
            with torch.cuda.stream(self.streams[s]):
                self.graphs[s].graph.replay()
                self.events[s].record(self.streams[s])
            self.last = s
        # wait on the HOST for every slot's last event -- not `current_stream.wait_stream(slot stream)`: the CU-masked streams are
        # blocking streams in the legacy sense, and an operation on the default stream while their queues are full cost 13 % of the
        # run's throughput (round 6, tools_dev/cu_mask_probe.py: 61.4 -> 53.9 maps/s; plain side streams are unaffected)
        for s in range(min(count, len(self.graphs))):
            self.events[s].synchronize()
