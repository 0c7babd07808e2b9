"""The depth map as a function of device tensors: the two-view and multi-view pipelines of the reference's run loops
(reference example.py:140-181, 239-267) on one MI355X, without leaving the device.  What captures and queues them is
atvsnet/graphs.py, what guards their fp16 range atvsnet/range_guard.py; atvsnet/example.py re-exports the public names."""
import torch

from ..flags import FLAGS
from .model import (TVSNet, TVSNet_base_siamese, TVSNet_feature_extraction, TVSNet_refine, base_stage_batch,
                    cost_volume_aggregation, cost_volume_aggregation_refine, extract_feature_shallow, feature_extraction_batch,
                    output_conv, output_conv_refine, prob2depth, prob2depth_upsample, refinement_batch, shallow_feature_batch)
from .. import ops
from ..cnn_wrapper.atvsnet import ResNetDS2SPP_shallow_f16


def depth_range(cams):
    """depth_start = cams[0,0,1,3,0], depth_interval = cams[0,0,1,3,1] as 1-element device tensors
    (reference example.py:66-69)."""
    return cams[0, 0, 1, 3, 0:1].contiguous(), cams[0, 0, 1, 3, 1:2].contiguous()


# Every network of a depth map is evaluated ONCE over all its independent calls (views, siamese directions) stacked on
# the batch axis, with per-call batch statistics (model.*_batch): ~8x fewer, 8x larger launches than the reference's
# call-per-view order, same values.  batched=False keeps the call-per-view order (per-view HIP streams).
BATCHED = True


def infer_twoview(images, cams, max_d=None, batched=None):
    """The graph of run_test_twoview (reference example.py:239-240, 267): images (1,2,H,W,3) float32
    BGR 0..255, cams (1,2,2,4,4), both on the device -> inverse-depth map (1,H,W,1) on the device."""
    max_d = FLAGS.max_d if max_d is None else max_d
    depth_start, depth_interval = depth_range(cams)
    if BATCHED if batched is None else batched:
        # model.TVSNet (reference model.py:346-377) with both towers, both siamese directions in one pass each
        feats = feature_extraction_batch(images)
        hom = {}
        _, prob_b2, depth_b2, dview = base_stage_batch(feats, cams, max_d, depth_start, depth_interval, fwd=[1], rev=[1], hom=hom,
                                                       filtered=False)
        shallow = shallow_feature_batch(images)
        _, prob_residual = refinement_batch(depth_b2, dview, prob_b2, cams, max_d, depth_start, depth_interval, [1], shallow,
                                            hom=hom, cost=False)
        refined_prob_volume = ops.add_n([prob_b2, prob_residual])
        _, depth_refined = prob2depth_upsample(refined_prob_volume, max_d, depth_start, depth_interval, out_prob_map=False)
        return depth_refined
    refined_prob_volume = TVSNet(images, cams, max_d, depth_start, depth_interval, view_i=1, ref_i=0)
    _, depth_refined = prob2depth_upsample(refined_prob_volume, max_d, depth_start, depth_interval, out_prob_map=False)
    return depth_refined


# A-B on MI355X (tools_dev/ab.py): 49.3 ms without, 52.5 ms with (five concurrent towers delay the reference
# tower every stream then waits for)
OVERLAP_REF_TOWER = False
# Upper bound on concurrently issued views (views are dealt round-robin to the streams).  A-B at config 3 (4 sources):
# 1 stream 55.3 ms, 2 streams 45.7, 3 streams 47.4, 4 streams 43.5; one stream per (source, direction) = 8 streams
# 50.1 ms -- more concurrency than one stream per source makes the GPU-filling kernels of different streams collide.
MAX_VIEW_STREAMS = 16


class _ViewStreams(object):
    """One HIP stream per source view (plus the caller's stream).

    The per-view base and refinement stages are independent (reference example.py:144-149,163-172), and
    many of their kernels (1/4- and 1/8-resolution layers, 2-D towers) cannot fill 256 CUs on their own:
    issuing the views on separate streams lets the GPU overlap them.  Every tensor a view stream produces
    is handed to the main stream with an event wait + record_stream (caching-allocator safety)."""

    def __init__(self, n, device, enabled):
        self.device = device
        self.enabled = bool(enabled) and device.type == 'cuda' and n > 1
        self.streams = [torch.cuda.Stream(device) for _ in range(min(n, MAX_VIEW_STREAMS))] if self.enabled else []

    @property
    def main(self):
        """The caller's stream NOW (a pipeline captured as several graphs re-enters with a new capture stream)."""
        return torch.cuda.current_stream(self.device) if self.device.type == 'cuda' else None

    def run(self, i, fn, after=None):
        """fn() on stream i, after everything queued so far on the main stream (or after the event `after`
        recorded earlier on it); returns fn's result."""
        if not self.enabled:
            return fn()
        st = self.streams[i % len(self.streams)]
        if after is not None:
            st.wait_event(after)
        else:
            st.wait_stream(self.main)
        with torch.cuda.stream(st):
            return fn()

    def mark(self):
        """An event on the main stream at this point of the issue order (None when streams are off)."""
        return self.main.record_event() if self.enabled else None

    def join(self, tensors):
        """Main stream waits for every view stream; `tensors` (nested lists ok) become usable on it."""
        if not self.enabled:
            return
        main = self.main
        for st in self.streams:
            main.wait_stream(st)
        if torch.cuda.is_current_stream_capturing():        # a capturing graph owns its pool's lifetimes
            return

        def rec(t):
            if isinstance(t, (list, tuple)):
                for u in t:
                    rec(u)
            elif isinstance(t, torch.Tensor):
                t.record_stream(main)
        rec(tensors)



def multiview_towers(images):
    """Both 2-D towers of every view: (1,N,H,W,3) -> (features (N,H/4,W/4,32), shallow features (N,H/4,W/4,16)); per-image
    statistics, so each row depends on its own image only (the scene cache, atvsnet/scene.py, computes them once per image)."""
    return feature_extraction_batch(images), shallow_feature_batch(images)


def infer_multiview_from_features(feats, shallow, cams, max_d, stages=None, out_prob_map=False):
    """The batched multi-view pipeline after the towers: feats (N,h,w,32) and shallow (N,h,w,16) of the N views (tensors, or
    callables computing them when first needed), cams (1,N,2,4,4)."""
    max_d = FLAGS.max_d if max_d is None else max_d
    n = cams.shape[1]
    src = list(range(1, n))
    depth_start, depth_interval = depth_range(cams)
    feats = feats() if callable(feats) else feats
    hom = {}                       # the plane sweeps of the camera pairs: computed once per depth map
    # only the forward filtered volumes and the reverse depths are read: the head runs over the reverse samples alone
    filtered, _, _, depth_view = base_stage_batch(feats, cams, max_d, depth_start, depth_interval, fwd=src, rev=src, hom=hom,
                                                  fwd_prob=False)
    del feats
    # AAM1
    cost_volume_agg = cost_volume_aggregation(filtered, reuse=False, keepchannel=True)
    prob_volume_agg = output_conv(cost_volume_agg, reuse=False)
    depth_agg_init = prob2depth(prob_volume_agg, max_d, depth_start, depth_interval, out_prob_map=False)
    del filtered
    # refinement of every source against the aggregated estimate
    shallow = shallow() if callable(shallow) else shallow
    # refined_cost = filtered_cost + residual (model.py:438) of every source: formed by the pass that forms the residuals, which
    # are read by nothing else (no probability head, the residual itself not written)
    _, _, refined = refinement_batch(depth_agg_init, depth_view, prob_volume_agg, cams, max_d, depth_start, depth_interval, src,
                                     shallow, hom=hom, residual_base=cost_volume_agg, cost=False, prob=False)
    # AAM2
    refined_cost_volume_agg = cost_volume_aggregation_refine(refined, reuse=False, keepchannel=True)
    refined_prob_volume_agg = output_conv_refine(refined_cost_volume_agg, reuse=False)
    final = prob2depth_upsample(refined_prob_volume_agg, max_d, depth_start, depth_interval, out_prob_map=out_prob_map)
    if stages is not None:
        stages.update(depth_views=[depth_view[v] for v in src], cost_volume_agg=cost_volume_agg,
                      prob_volume_agg=prob_volume_agg, depth_agg_init=depth_agg_init,
                      refined_cost_volume_agg=refined_cost_volume_agg, refined_prob_volume_agg=refined_prob_volume_agg)
    return final if out_prob_map else final[1]


def infer_multiview(images, cams, max_d=None, stages=None, view_streams=True, out_prob_map=False, batched=None):
    """The run loop of run_test_multiview (reference example.py:140-181), on the device:
    base (per source) -> AAM1 -> refinement (per source) -> AAM2 -> x4 upsample + soft-argmin.
    batched (default BATCHED): one pass of each network over all its per-view calls; otherwise call per view, and
    view_streams: issue the independent per-view stages on separate HIP streams.
    out_prob_map: return (depth, depth_up, prob_map, prob_map_up) as the ETH3D driver's last stage does
    (reference eval_pointcloud.py:268-272) instead of depth_up alone."""
    max_d = FLAGS.max_d if max_d is None else max_d
    n = images.shape[1]
    assert n > 2
    if BATCHED if batched is None else batched:
        # every per-view network evaluated once over all views (model.*_batch); the towers are issued where the body first needs
        # their output (feature tower first, shallow tower after AAM1)
        return infer_multiview_from_features(lambda: feature_extraction_batch(images), lambda: shallow_feature_batch(images), cams,
                                             max_d, stages, out_prob_map)
    depth_start, depth_interval = depth_range(cams)
    vs = _ViewStreams(n - 1, images.device, view_streams)
    start = vs.mark() if OVERLAP_REF_TOWER else None     # the source towers need not wait for the reference tower ...
    ref_feature = TVSNet_feature_extraction(images, 0)
    ref_ready = vs.mark() if OVERLAP_REF_TOWER else None  # ... only their cost volumes do
    base = [vs.run(v - 1, lambda v=v: TVSNet_base_siamese(images, cams, max_d, depth_start, depth_interval, view_i=v,
                                                          ref_i=0, ref_feature=ref_feature, ref_ready=ref_ready),
                   after=start)
            for v in range(1, n)]
    vs.join(base)
    filtered_cost_volumes = [b[2] for b in base]    # prob volumes are fed but unused by the reference (quirk C12)
    depth_views = [b[3] for b in base]
    del base
    # AAM1
    cost_volume_agg = cost_volume_aggregation(filtered_cost_volumes, reuse=False, keepchannel=True)
    prob_volume_agg = output_conv(cost_volume_agg, reuse=False)
    depth_agg_init = prob2depth(prob_volume_agg, max_d, depth_start, depth_interval, out_prob_map=False)
    del filtered_cost_volumes
    # refinement against the aggregated estimate
    ref_shallow = ResNetDS2SPP_shallow_f16({'data': images[:, 0]}, is_training=True).get_output()

    def refine(view_i):
        shallow = extract_feature_shallow(images, 0, view_i, ref_feature=ref_shallow)
        return TVSNet_refine(depth_agg_init, depth_views[view_i - 1], prob_volume_agg, cost_volume_agg, images, cams,
                             max_d, depth_start, depth_interval, view_i=view_i, ref_i=0, shallow_features=shallow)[1]
    refined_cost_volumes = [vs.run(v - 1, lambda v=v: refine(v)) for v in range(1, n)]
    vs.join(refined_cost_volumes)
    # AAM2
    refined_cost_volume_agg = cost_volume_aggregation_refine(refined_cost_volumes, reuse=False, keepchannel=True)
    refined_prob_volume_agg = output_conv_refine(refined_cost_volume_agg, reuse=False)
    final = prob2depth_upsample(refined_prob_volume_agg, max_d, depth_start, depth_interval, out_prob_map=out_prob_map)
    depth_agg_refined = final[1]
    if stages is not None:
        stages.update(depth_views=depth_views, cost_volume_agg=cost_volume_agg, prob_volume_agg=prob_volume_agg,
                      depth_agg_init=depth_agg_init, refined_cost_volume_agg=refined_cost_volume_agg,
                      refined_prob_volume_agg=refined_prob_volume_agg)
    return final if out_prob_map else depth_agg_refined

