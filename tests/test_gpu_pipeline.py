"""-m gpu: whole networks and the example.py pipelines on the MI355X vs the CPU oracle,
same seeded inputs and weights (config 1 of BASELINE.json: 160x128 image, D=32).

Bar (BASELINE.json north_star): rel-L1 of the final depth map <= 1e-3.  The fp32 path is
expected to sit orders of magnitude below it; intermediate volumes are checked at 1e-3 of
their max (31 BN-normalised layers amplify summation-order noise by < 100x).
"""
import pytest
import torch

from oracle import model as OM
from oracle import nets

pytestmark = pytest.mark.gpu


def rel_l1(got, want):
    return float(((got - want).abs() / want.abs().clamp(min=1e-12)).mean())


def _inputs(views, H=128, W=160, D=32):
    from atvsnet_amd import synthetic
    imgs, cams = synthetic.make_inputs(views, H, W, D)
    return torch.from_numpy(imgs), torch.from_numpy(cams)


def test_feature_tower(cuda, weights):
    from atvsnet_amd.cnn_wrapper.atvsnet import ResNetDS2SPP, ResNetDS2SPP_shallow_f16
    imgs, _ = _inputs(2)
    L = {}
    want = nets.resnet_ds2_spp(imgs[:, 0], weights, L)
    net = ResNetDS2SPP({'data': imgs[:, 0].to(cuda)}, is_training=True)
    for name in ('conv1_x', 'conv3_x', 'branch_0', 'branch_1', 'branch_2', 'branch_3', 'fusion0', 'fusion1'):
        g, w = net.get_output_by_name(name).cpu(), L[name]
        assert g.shape == w.shape, name
        assert float((g - w).abs().max()) <= 2e-4 * float(w.abs().max()) + 1e-6, name
    assert float((net.get_output().cpu() - want).abs().max()) <= 2e-4 * float(want.abs().max())
    want16 = nets.resnet_ds2_spp_shallow_f16(imgs[:, 1], weights)
    got16 = ResNetDS2SPP_shallow_f16({'data': imgs[:, 1].to(cuda)}, is_training=True).get_output().cpu()
    assert got16.shape == want16.shape
    assert float((got16 - want16).abs().max()) <= 2e-4 * float(want16.abs().max())


def test_stacked_unet(cuda, weights):
    from atvsnet_amd.cnn_wrapper.atvsnet import StackedUNet_prob
    g = torch.Generator().manual_seed(3)
    data = torch.randn(1, 32, 32, 40, 64, generator=g)
    L = {}
    want_p, want_f = nets.stacked_unet_prob(data, weights, L)
    net = StackedUNet_prob({'data': data.to(cuda)}, is_training=True)
    for name, w in L.items():
        if name == 'data':
            continue
        gt = net.get_output_by_name(name).cpu()
        assert gt.shape == w.shape, name
        assert float((gt - w).abs().max()) <= 1e-3 * float(w.abs().max()) + 1e-6, name
    assert float((net.get_output().cpu() - want_p).abs().max()) <= 1e-3 * float(want_p.abs().max())


def test_twoview_end_to_end(cuda, weights):
    from atvsnet_amd.atvsnet import example as ex
    imgs, cams = _inputs(2)
    S = {}
    want = OM.run_twoview(imgs, cams, weights, 32, S)
    got = ex.infer_twoview(imgs.to(cuda), cams.to(cuda), 32).cpu()
    assert got.shape == want.shape == (1, 128, 160, 1)
    err = rel_l1(got, want)
    err_depth = rel_l1(OM.invert_depth(got, True), OM.invert_depth(want, True))
    print('two-view rel-L1 inverse depth %.3e, depth %.3e' % (err, err_depth))
    assert err <= 1e-3 and err_depth <= 1e-3
    assert float(want.std()) > 0.02            # not a degenerate (flat) answer


def test_against_committed_oracle_fixture(cuda, weights):
    """The same pipelines against tests/golden/oracle_cfg1.npz (made by tests/golden/make_oracle_golden.py)."""
    import os
    import numpy as np
    from atvsnet_amd.atvsnet import example as ex
    gold = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'oracle_cfg1.npz'))
    imgs, cams = _inputs(2)
    got = ex.infer_twoview(imgs.to(cuda), cams.to(cuda), 32).cpu()[0, ..., 0]
    assert rel_l1(got, torch.from_numpy(gold['twoview_depth'])) <= 1e-3
    imgs, cams = _inputs(3)
    G = {}
    got = ex.infer_multiview(imgs.to(cuda), cams.to(cuda), 32, G).cpu()[0, ..., 0]
    assert rel_l1(got, torch.from_numpy(gold['multiview3_depth'])) <= 1e-3
    assert rel_l1(G['depth_agg_init'].cpu()[0, ..., 0], torch.from_numpy(gold['multiview3_depth_agg_init'])) <= 1e-3


def test_multiview_end_to_end(cuda, weights):
    from atvsnet_amd.atvsnet import example as ex
    imgs, cams = _inputs(4)
    S, G = {}, {}
    want = OM.run_multiview(imgs, cams, weights, 32, S)
    got = ex.infer_multiview(imgs.to(cuda), cams.to(cuda), 32, G).cpu()
    for k in ('depth_agg_init', 'cost_volume_agg', 'prob_volume_agg', 'refined_cost_volume_agg',
              'refined_prob_volume_agg'):
        g, w = G[k].cpu(), S[k]
        assert g.shape == w.shape, k
        assert float((g - w).abs().max()) <= 2e-3 * float(w.abs().max()), k
    assert len(G['depth_views']) == len(S['depth_views']) == 3
    for v, (g, w) in enumerate(zip(G['depth_views'], S['depth_views']), 1):      # the reverse direction's depth of every source
        assert g.shape == w.shape, v
        assert float((g.cpu() - w).abs().max()) <= 2e-3 * float(w.abs().max()), v
    err = rel_l1(got, want)
    print('multi-view (N=4) rel-L1 inverse depth %.3e' % err)
    assert err <= 1e-3
    assert rel_l1(OM.invert_depth(got, False), OM.invert_depth(want, False)) <= 1e-3


def test_stacked_attention_input_matches_list(cuda, weights):
    """cost_volume_aggregation accepts the reference's (B,D,H,W,C,N) layout as well as a list."""
    from atvsnet_amd.atvsnet import model
    g = torch.Generator().manual_seed(9)
    X = torch.randn(1, 8, 8, 12, 8, 3, generator=g)
    want = OM.cost_volume_aggregation(X, weights)
    a = model.cost_volume_aggregation(X.to(cuda), keepchannel=True).cpu()
    b = model.cost_volume_aggregation([X[..., n].contiguous().to(cuda) for n in range(3)], keepchannel=True).cpu()
    assert torch.equal(a, b)
    assert float((a - want).abs().max()) < 1e-5
    p = model.cost_volume_aggregation(X.to(cuda), keepchannel=False).cpu()
    want_p = nets.output_conv(want, weights, 'attention_prob_vol')
    assert float((p - want_p).abs().max()) < 1e-4 * float(want_p.abs().max()) + 1e-5


def test_graph_replay_equals_eager(cuda, weights):
    """The pipeline captured in a HIP graph (per-view streams included) gives the eager result, also
    after the static input buffers are overwritten with another scene."""
    from atvsnet_amd.atvsnet import example as ex
    imgs, cams = _inputs(4)
    imgs, cams = imgs.to(cuda), cams.to(cuda)
    eager = ex.infer_multiview(imgs, cams, 32).clone()
    g = ex.GraphedInference(imgs, cams, 32)
    assert torch.equal(g(), eager)
    imgs2 = imgs.flip(1).contiguous()
    cams2 = cams.flip(1).contiguous()
    eager2 = ex.infer_multiview(imgs2, cams2, 32).clone()
    assert not torch.equal(eager2, eager)
    assert torch.equal(g(imgs2, cams2), eager2)
    assert torch.equal(g(imgs, cams), eager)


def test_midsize_pipelines(cuda, weights):
    """320x256 images, D=64 (feature grid 64x80): exercises full tiles, the x-pair form, N-split and the
    fused transposed convolution at sizes between config 1 and the benchmark configuration."""
    from atvsnet_amd.atvsnet import example as ex
    imgs, cams = _inputs(3, 256, 320, 64)
    want2 = OM.run_twoview(imgs[:, :2], cams[:, :2], weights, 64)
    got2 = ex.infer_twoview(imgs[:, :2].contiguous().to(cuda), cams[:, :2].contiguous().to(cuda), 64).cpu()
    e2 = rel_l1(got2, want2)
    want3 = OM.run_multiview(imgs, cams, weights, 64)
    got3 = ex.infer_multiview(imgs.to(cuda), cams.to(cuda), 64).cpu()
    e3 = rel_l1(got3, want3)
    print('mid-size rel-L1: two-view %.3e, 3-view %.3e' % (e2, e3))
    assert e2 <= 1e-3 and e3 <= 1e-3


def test_midsize_against_float64_networks(cuda, weights):
    """tests/golden/truth64_mid.npz (tests/golden/make_truth64_golden.py): the same two-view case with the
    oracle's networks in float64.  With these weights float32 rounding alone moves the final depth by
    ~1e-3 (31 batch-normalised layers + a peaked soft-argmin amplify it); the HIP path must be no further
    from the float64 value than the float32 oracle is (x1.5 slack), and within 1e-3 of the float32 oracle."""
    import os
    import numpy as np
    from atvsnet_amd.atvsnet import example as ex
    gold = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'truth64_mid.npz'))
    imgs, cams = _inputs(2, 256, 320, 64)
    got = ex.infer_twoview(imgs.to(cuda), cams.to(cuda), 64).cpu()[0, ..., 0]
    e64 = rel_l1(got, torch.from_numpy(gold['depth64']))
    e32 = rel_l1(got, torch.from_numpy(gold['depth32']))
    print('HIP vs float64 networks %.3e (float32 oracle: %.3e); HIP vs float32 oracle %.3e'
          % (e64, float(gold['oracle32_rel_l1']), e32))
    assert e64 <= 1.5 * float(gold['oracle32_rel_l1'])
    assert e32 <= 1e-3


def test_graft_entry_build_then_smoke_in_one_process(cuda):
    """build() loads the HIP library before anything touched the GPU; smoke() then runs the pipeline.  (The library
    must bind to the HIP runtime torch carries -- loaded before torch it once bound to /opt/rocm's and every launch
    on a torch stream failed.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', 'import __graft_entry__ as g; g.build(); g.smoke()'], cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode('utf-8', 'replace')
    assert r.returncode == 0 and 'smoke ok' in out, out[-2000:]


@pytest.mark.parametrize('co_resident', [False, True, 'cu_split'])
def test_pipelined_inference_two_in_flight(cuda, weights, co_resident):
    """example.PipelinedInference: two depth maps queued (independent reference views of a scene, reference
    eval_pointcloud.py:399-424) give, per depth map, exactly what one pipeline gives -- with the GPU running one map at
    a time (the default), with both maps' kernels on the GPU at once (co_resident=True, opt-in) and with each map on its own
    share of every XCD's compute units (co_resident='cu_split': no SIMD shared between the maps)."""
    from atvsnet_amd.atvsnet import example as ex
    from atvsnet_amd import synthetic
    imgs, cams = _inputs(3)
    imgs, cams = imgs.to(cuda), cams.to(cuda)
    imgs2 = torch.from_numpy(synthetic.make_inputs(3, 128, 160, 32, seed=7)[0]).to(cuda)
    want1 = ex.infer_multiview(imgs, cams, 32).clone()
    want2 = ex.infer_multiview(imgs2, cams, 32).clone()
    assert not torch.equal(want1, want2)
    p = ex.PipelinedInference(imgs, cams, 32, slots=2, co_resident=co_resident)
    assert ex.PipelinedInference.__init__.__defaults__[2] is False          # co-residency is opt-in
    t1 = p.submit(imgs, cams)
    t2 = p.submit(imgs2, cams)
    with pytest.raises(RuntimeError):
        p.submit(imgs, cams)                        # both slots hold unfetched results
    got1 = p.result(t1).clone()
    t3 = p.submit(imgs2, cams)                      # slot of t1 again, other inputs
    got2 = p.result(t2).clone()
    got3 = p.result(t3).clone()
    assert torch.equal(got1, want1) and torch.equal(got2, want2) and torch.equal(got3, want2)
    with pytest.raises(RuntimeError):
        p.result(t1)
    p.run(5)                                        # the benchmark loop: captured inputs of each slot, all complete on return
    torch.cuda.synchronize()
    assert torch.isfinite(p.graphs[0].out).all() and torch.isfinite(p.graphs[1].out).all()


def test_small_kernels_beside_other_wavefronts(cuda):
    """Two depth maps in flight put wavefronts of DIFFERENT kernels on one SIMD.  An unrolled form of the plane-sweep warp
    (packed arithmetic, four passes in flight) produced wrong first components of its 16-byte stores only then -- beside a
    wavefront of the stride-2 encoder kernel -- and passed every single-stream test.  Here the small kernels of the pipeline
    run on one stream while register-light convolution kernels run on another; every output must equal its single-stream
    value."""
    import numpy as np
    from atvsnet_amd import ops, synthetic
    rng = np.random.default_rng(0)
    wt = lambda *s: (rng.standard_normal(s) * 0.1).astype(np.float32)      # noqa: E731
    D, h, w, C, G = 32, 32, 40, 32, 4
    src = torch.randn(h, w, C, device=cuda)
    cams = torch.from_numpy(synthetic.make_inputs(2, 128, 160, D)[1]).to(cuda)[0]
    cams4 = cams.clone()
    cams4[:, 1, :2, :3] /= 4.0
    Hm = ops.get_homographies(cams4[0], cams4[1], cams[0, 1, 3, 0:1].contiguous(), cams[0, 1, 3, 1:2].contiguous(), D)
    vol = torch.empty(C // 8, ops.planar_stride(D, h, w), device=cuda)
    x8 = torch.randn(G, D, h, w, 8, device=cuda)
    wh = torch.randn(3, 3, 3, 8, 1, device=cuda) * 0.1
    par = torch.stack([torch.randn(G, 8) * 0.1, torch.rand(G, 8) + 0.5, torch.randn(G, 8) * 0.1], 1).to(cuda).contiguous()
    victims = {
        'warp': lambda: ops.planar_view(ops.warp_planes(src, Hm, out=vol, planar=True), D, h, w),
        'warp channel-last': lambda: ops.warp_planes(src, Hm),
        '8to1': lambda: ops.conv3d_8to1(x8, wh, groups=G),
        'bn_add': lambda: ops.bn_add([ops.PendingBN(x8, par, True), ops.PendingBN(x8, par, False)]),
    }
    x16 = torch.randn(G, 16, 16, 20, 16, device=cuda)
    x32 = torch.randn(G, 8, 8, 16, 32, device=cuda)
    x2d = torch.randn(3, 32, 40, 128, device=cuda)
    w1632, w3232, w2d, w1 = wt(3, 3, 3, 16, 32), wt(3, 3, 3, 32, 32), wt(3, 3, 128, 128), wt(1, 1, 128, 128)
    aggressors = {
        'stride-2 encoder': lambda: ops.conv(x16, 'race_s2b', w1632, stride=2, want_stats=True, groups=G)[0],
        '32 -> 32': lambda: ops.conv(x32, 'race_c3b', w3232, want_stats=True, groups=G)[0],
        'tower 3x3': lambda: ops.conv2d_lds(x2d, 'race_c2b', w2d, 2, want_stats=True)[0],
        'tower 1x1': lambda: ops.conv1x1(x2d, 'race_c1b', w1, want_stats=True)[0],
    }
    ref = {k: f().clone() for k, f in victims.items()}
    for f in aggressors.values():
        f()
    torch.cuda.synchronize()

    def capture(f, n):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = [f() for _ in range(n)]
        return g, outs

    vg = {k: capture(f, 4) for k, f in victims.items()}
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for an, fa in aggressors.items():
        ga, _ = capture(fa, 16)
        for vn, (gv, outs) in vg.items():
            for rep in range(4):
                torch.cuda.synchronize()
                with torch.cuda.stream(sa):
                    ga.replay()
                with torch.cuda.stream(sb):
                    gv.replay()
                torch.cuda.synchronize()
                for o in outs:
                    assert torch.equal(o, ref[vn]), '%s beside %s' % (vn, an)


def test_two_depth_maps_in_flight_fullsize(cuda, weights):
    """BASELINE configs[2] with two depth maps in flight (example.PipelinedInference), 30 pairs: every map equals its
    one-at-a-time value bit for bit.  At this size the kernels of the two maps share SIMDs in many combinations; before the
    small kernels were built without compiler-formed packed fp32 instructions 4-15 % of the maps came out wrong here (the
    homographies of 16 depth planes = the last lane quarter of one wavefront)."""
    from atvsnet_amd.atvsnet import example as ex
    from atvsnet_amd import synthetic

    def inputs(seed):
        i, c = synthetic.make_inputs(5, 512, 640, 192, seed=seed)
        return torch.from_numpy(i).to(cuda), torch.from_numpy(c).to(cuda)

    imgs, cams = inputs(0)
    imgs2, _ = inputs(7)
    p = ex.PipelinedInference(imgs, cams, 192, slots=2, co_resident=True)
    w1 = p.result(p.submit(imgs, cams)).clone()
    torch.cuda.synchronize()
    w2 = p.result(p.submit(imgs2, cams)).clone()
    torch.cuda.synchronize()
    assert not torch.equal(w1, w2)
    for rep in range(30):
        t1 = p.submit(imgs, cams)
        t2 = p.submit(imgs2, cams)
        g1 = p.result(t1).clone()
        g2 = p.result(t2).clone()
        assert torch.equal(g1, w1) and torch.equal(g2, w2), rep


def test_cu_split_streams_confine_their_kernels(cuda, weights):
    """example.cu_split_streams: the runtime silently IGNORES a CU mask it does not like (one that leaves an XCD without a compute
    unit runs on the whole chip) -- and a stream that is not confined gives no protection against the co-residency fault.  So: the
    same captured depth map replayed on one of the two half-chip streams must be clearly slower than on a plain stream (measured:
    1.25 x here, 1.6 x at configs[2]), on one of four quarter-chip streams slower again, with every bit unchanged; and two / four maps in flight on the parts
    give the single-map bits."""
    import time
    from atvsnet_amd.atvsnet import example as ex
    from atvsnet_amd import synthetic
    i, c = synthetic.make_inputs(3, 256, 320, 96)
    imgs, cams = torch.from_numpy(i).to(cuda), torch.from_numpy(c).to(cuda)
    g = ex.GraphedInference(imgs, cams, 96)
    want = g().clone()
    torch.cuda.synchronize()                 # the replays below run on other streams: the copy must have read the buffer first

    def timed(stream, n=10):
        with torch.cuda.stream(stream):
            g.graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            for _ in range(n):
                g.graph.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n
    plain = timed(torch.cuda.Stream(cuda))
    halves, quarters = ex.cu_split_streams(cuda, 2), ex.cu_split_streams(cuda, 4)
    th = [timed(st) for st in halves]
    assert torch.equal(g.out, want)
    tq = timed(quarters[3])
    assert torch.equal(g.out, want)
    print('one map: plain stream %.2f ms, half-chip streams %.2f / %.2f ms, a quarter-chip stream %.2f ms' % (1e3 * plain, 1e3 * th[0], 1e3 * th[1], 1e3 * tq))
    assert min(th) >= 1.15 * plain, (plain, th)           # half the compute units: measured 1.25 x at this size (1.6 x at configs[2])
    assert tq >= 1.15 * max(th), (th, tq)                 # a quarter: measured 1.5 x the halves
    with pytest.raises(ValueError):
        ex.cu_split_streams(cuda, 0)
    for parts in (2, 4):
        p = ex.PipelinedInference(imgs, cams, 96, slots=parts, co_resident='cu_split')
        assert p.cu_split and p.co_resident
        himgs, hcams = imgs.cpu(), cams.cpu()
        for rep in range(3):
            # host tensors in, host tensors out: the slots' own streams do the copies (no operation on the default stream, which would
            # order every submission behind all maps in flight); device tensors work too, serialised
            ts = [p.submit(himgs, hcams) if rep else p.submit(imgs, cams) for _ in range(parts)]
            for t in ts:
                got = p.result(t, host=bool(rep))
                assert got.is_cuda != bool(rep) and torch.equal(got.to(cuda), want)
        p.set_mode(False)
        assert not p.cu_split and torch.equal(p.result(p.submit(imgs, cams)), want)
