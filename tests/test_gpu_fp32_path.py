"""-m gpu: the fp32 recompute path (ops.configure(split16=False): every convolution on the fp32 matrix cores, the AANet modules
as score convolution + ops.aanet_combine) as whole pipelines -- what atvsnet/range_guard.py returns for a map whose residual
stream left the fp16 range of the split-operand kernels, i.e. what a real checkpoint may get for every map.

tests/test_gpu_split_precision.py holds the fp32 launch forms element by element at the smallest shapes that reach them; here:
the metric's configuration at full size (where tests/golden/conv_dispatch.json's 640x512 cases pick conv_tiled and the grids and
byte offsets are product-sized), the guard's three multi-view drivers against the eager fp32 map, and the five-source AANet
inside a pipeline -- each against the float32 oracle at BASELINE.json's bar."""
import pytest
import torch

import atvsnet_amd  # noqa: F401
from oracle import model as OM

import test_conv_dispatch as CD
import test_gpu_fullsize as FS
import test_gpu_range as R

pytestmark = pytest.mark.gpu
BAR = FS.BAR                      # 1e-3 rel-L1, BASELINE.json


def test_cfg3_multiview_fullsize_on_the_fp32_kernels(cuda, weights):
    """BASELINE configs[2] (5 views 640x512, D=192) under split16=False against tests/golden/fullsize_cfg3.npz with
    test_cfg3_multiview_fullsize's assertions: the final map, AAM1's depth, the middle plane of AAM1's output (two launches on
    this path); a graph captured under the same switch replays the eager bits."""
    from atvsnet_amd import ops
    from atvsnet_amd.atvsnet import example as ex
    gold = FS._gold('cfg3')
    imgs, cams, D = FS._inputs('cfg3', cuda)
    with ops.configure(split16=False, clear_pack_cache=True):
        ops.nonfinite_seen(cuda)
        G = {}
        got = ex.infer_multiview(imgs, cams, D, G, view_streams=False)
        FS._check_depth('cfg3 fp32', got, gold, cams, D)
        e = FS.rel_l1(G['depth_agg_init'].cpu()[0, ..., 0], torch.from_numpy(gold['depth_agg_init']))
        print('cfg3 fp32 depth_agg_init rel-L1 %.3e' % e)
        assert e <= BAR
        w = torch.from_numpy(gold['cost_agg_mid'])
        diff = (G['cost_volume_agg'].cpu()[0, D // 2] - w).abs()
        print('cfg3 fp32 cost_volume_agg plane %d: max abs diff %.3e of max %.3e'
              % (D // 2, float(diff.max()), float(w.abs().max())))
        assert float(diff.max()) <= 1e-3 * float(w.abs().max())
        del G
        gr = ex.GraphedInference(imgs, cams, D)
        assert not gr.split16
        assert torch.equal(gr(), got)
        assert not ops.nonfinite_seen(cuda)
    ops.clear_pack_cache()


def test_the_multiview_drivers_return_the_fp32_map_when_the_split_kernels_overflow(cuda, weights):
    """test_gpu_range's overflowing tower on the multi-view pipeline (three views 128x160, D=32): the split path raises the
    flag, the split16=False map is inside the bar against the oracle evaluated with the same weights, and the eager guard,
    GraphedInference.checked() (its first call, which captures the fallback graph, and the replay of that graph) and
    PipelinedInference.result() each return that map bit for bit."""
    from atvsnet_amd import ops, synthetic
    from atvsnet_amd.atvsnet import example as ex
    imgs, cams = synthetic.make_inputs(3, 128, 160, 32)
    imgs_t, cams_t = torch.from_numpy(imgs), torch.from_numpy(cams)
    di, dc = imgs_t.to(cuda), cams_t.to(cuda)
    with R._overflowing_tower(weights) as scaled:
        want = OM.run_multiview(imgs_t, cams_t, scaled, 32)
        assert bool(torch.isfinite(want).all())
        ops.nonfinite_seen(cuda)
        ex.infer_multiview(di, dc, 32)
        assert ops.nonfinite_seen(cuda), 'the scaled weights no longer overflow the split-operand towers'
        with ops.configure(split16=False):
            fp32 = ex.infer_multiview(di, dc, 32).cpu()
        assert not ops.nonfinite_seen(cuda) and bool(torch.isfinite(fp32).all())
        err = FS.rel_l1(fp32, want)
        print('fp32 multi-view map vs the oracle on the overflowing weights: rel-L1 %.2e' % err)
        assert err <= BAR
        # (1) the eager drivers' guard
        got = ex.infer_checked(lambda: ex.infer_multiview(di, dc, 32), cuda).cpu()
        assert torch.equal(got, fp32)
        assert ops.cfg.split16 == ops.Config._DEFAULTS['split16']                # the switch is restored
        # (2) a captured graph: the fallback graph is captured by the first call and replayed by the second
        g = ex.GraphedInference(di, dc, 32)
        assert not g.twoview
        ops.nonfinite_seen(cuda)
        assert torch.equal(g.checked().cpu(), fp32)
        assert g._fp32 is not None and not g._fp32.split16 and not g._fp32.twoview
        fallback = g._fp32
        assert torch.equal(g.checked(di, dc).cpu(), fp32)
        assert g._fp32 is fallback
        # (3) the queue
        p = ex.PipelinedInference(di, dc, 32, slots=2)
        ops.nonfinite_seen(cuda)
        t0 = p.submit(di, dc)
        t1 = p.submit(di, dc)
        assert torch.equal(p.result(t0).cpu(), fp32)
        assert torch.equal(p.result(t1).cpu(), fp32)
    ops.nonfinite_seen(cuda)


def test_five_source_aanet_unfused_inside_the_fp32_pipeline(cuda, weights):
    """Six views (five sources) 128x160, D=32 under split16=False against the oracle: both AANet modules run as the score
    convolution of every view and ONE ops.aanet_combine over five views (csrc/aanet.hip), never as aanet_b.hip's single launch."""
    from atvsnet_amd import ops, synthetic
    from atvsnet_amd.atvsnet import example as ex
    imgs, cams = synthetic.make_inputs(6, 128, 160, 32)
    imgs_t, cams_t = torch.from_numpy(imgs), torch.from_numpy(cams)
    want = OM.run_multiview(imgs_t, cams_t, weights, 32)
    events, views = [], []
    combine = ops.aanet_combine

    def counted(srs, xs, out=None):
        views.append(len(xs))
        return combine(srs, xs, out=out)
    with ops.configure(split16=False, clear_pack_cache=True):
        ops.nonfinite_seen(cuda)
        with CD._counting(events, 'aanet_fused'), CD._replaced(combine, counted):
            got = ex.infer_multiview(imgs_t.to(cuda), cams_t.to(cuda), 32, view_streams=False).cpu()
        assert not ops.nonfinite_seen(cuda)
    ops.clear_pack_cache()
    assert views == [5, 5] and events == []
    err = FS.rel_l1(got, want)
    print('fp32 five-source map vs the oracle: rel-L1 %.2e' % err)
    assert err <= BAR
