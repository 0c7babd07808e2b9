"""-m gpu: the 8 -> 1 heads that form their input -- a U-Net's last skip add relu?(bn(a)) + relu?(bn(b)) -- while they stage it
(atvs_conv3d_8to1_bn2), atvs_bn_add_plus without the sum, and the pipelines with the dead heads left out: every result is the
bits of the passes they replace (bn_add, then the plain head)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _term(G, shape, seed, cuda, mean=0.0, std=1.0, grouped=True):
    """A raw volume (G,)+shape+(8,) around `mean` and its batch-norm parameters (mean, rstd, beta) per sample."""
    raw = (_rand((G,) + shape + (8,), seed) * std + mean).to(cuda)
    m = raw.reshape(G, -1, 8).mean(1)
    v = raw.reshape(G, -1, 8).var(1, unbiased=False)
    beta = _rand((G, 8), seed + 1).to(cuda) * 0.5
    params = torch.stack([m, torch.rsqrt(v + 1e-3), beta], 1).contiguous()          # (G,3,8)
    if not grouped:
        params = params[0].contiguous()
    return raw, params


@pytest.mark.parametrize('G,shape', [(1, (5, 13, 21)), (3, (7, 18, 35)), (2, (4, 16, 16)), (4, (9, 33, 17))])
@pytest.mark.parametrize('relu_mask', [0, 1, 2, 3])
def test_head_sums_on_load_bit_for_bit(cuda, G, shape, relu_mask):
    """Ragged D / H / W, one or several samples with their own parameters, every ReLU mask."""
    from atvsnet_amd import ops
    a, pa = _term(G, shape, 11 + G, cuda)
    b, pb = _term(G, shape, 23 + G, cuda)
    w = (_rand((3, 3, 3, 8, 1), 5) * 0.2).to(cuda).contiguous()
    items = lambda: [ops.PendingBN(a, pa, relu_mask & 1), ops.PendingBN(b, pb, relu_mask & 2)]   # noqa: E731
    want = ops.conv3d_8to1(ops.bn_add(items()), w, groups=G)
    got = ops.conv3d_8to1(ops.PendingSum(items()), w, groups=G)
    assert torch.equal(got, want)
    assert got.abs().max() > 0
    # a slice of the samples forms only those samples
    if G > 1:
        part = ops.conv3d_8to1(ops.PendingSum(items()).samples(1, G), w, groups=G - 1)
        assert torch.equal(part, want[1:])
    # cfg.sum_on_load off: the sum is materialised (bn_add) and the plain head runs
    with ops.configure(sum_on_load=False):
        assert torch.equal(ops.conv3d_8to1(ops.PendingSum(items()), w, groups=G), want)


@pytest.mark.parametrize('relu_mask', [1, 3])
def test_head_sums_on_load_many_tiles_per_workgroup(cuda, relu_mask):
    """More tiles (5 x 9 x 9 per sample, 1215 in all) than the 512 persistent workgroups: every workgroup walks several tiles and
    crosses from one sample to the next, reloading that sample's parameters."""
    from atvsnet_amd import ops
    G, shape = 3, (17, 130, 129)
    a, pa = _term(G, shape, 41, cuda, mean=2.0, std=3.0)
    b, pb = _term(G, shape, 42, cuda, mean=-1.0, std=0.5)
    w = (_rand((3, 3, 3, 8, 1), 7) * 0.2).to(cuda).contiguous()
    items = lambda: [ops.PendingBN(a, pa, relu_mask & 1), ops.PendingBN(b, pb, relu_mask & 2)]   # noqa: E731
    want = ops.conv3d_8to1(ops.bn_add(items()), w, groups=G)
    got = ops.conv3d_8to1(ops.PendingSum(items()), w, groups=G)
    assert torch.equal(got, want)
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])


def test_head_sums_on_load_large_mean_and_ungrouped_params(cuda):
    """|mean| / std large (cancellation in the normalisation); one sample with (3,8) parameters."""
    from atvsnet_amd import ops
    a, pa = _term(1, (6, 20, 24), 3, cuda, mean=3.0e3, std=20.0, grouped=False)
    b, pb = _term(1, (6, 20, 24), 4, cuda, mean=-1.5e4, std=0.5, grouped=False)
    w = (_rand((3, 3, 3, 8, 1), 6) * 0.2).to(cuda).contiguous()
    items = lambda: [ops.PendingBN(a, pa, True), ops.PendingBN(b, pb, False)]   # noqa: E731
    want = ops.conv3d_8to1(ops.bn_add(items()), w, groups=1)
    got = ops.conv3d_8to1(ops.PendingSum(items()), w, groups=1)
    assert torch.equal(got, want)


def test_bn_add_plus_without_the_sum(cuda):
    """keep_sum=False: y2 = base + sum keeps its bits and the sum is not returned."""
    from atvsnet_amd import ops
    G, shape = 3, (5, 12, 20)
    a, pa = _term(G, shape, 31, cuda)
    b, pb = _term(G, shape, 32, cuda)
    base = _rand(shape + (8,), 33).to(cuda)
    items = lambda: [ops.PendingBN(a, pa, True), ops.PendingBN(b, pb, True)]   # noqa: E731
    y, y2 = ops.bn_add(items(), plus=base)
    n, n2 = ops.bn_add(items(), plus=base, keep_sum=False)
    assert n is None and torch.equal(n2, y2)
    assert torch.equal(y, ops.bn_add(items()))


def _inputs(cuda, views, H, W, D):
    from atvsnet_amd import synthetic
    imgs, cams = synthetic.make_inputs(views, H, W, D)
    return torch.from_numpy(imgs).to(cuda), torch.from_numpy(cams).to(cuda)


def test_multiview_sum_on_load_on_off_equal_fullsize(cuda, weights):
    """BASELINE configs[2] (5 views 640x512, D=192), captured in a HIP graph: the heads that sum on load and the y-less
    bn_add_plus against the materialised passes; the stage outputs of the eager pipeline too."""
    from atvsnet_amd import ops
    from atvsnet_amd.atvsnet import example as ex
    imgs, cams = _inputs(cuda, 5, 512, 640, 192)
    st_on, st_off = {}, {}
    on = ex.GraphedInference(imgs, cams, 192)().clone()
    eager_on = ex.infer_multiview(imgs, cams, 192, stages=st_on).clone()
    with ops.configure(head_sum=False):
        off = ex.GraphedInference(imgs, cams, 192)().clone()
        eager_off = ex.infer_multiview(imgs, cams, 192, stages=st_off).clone()
    assert torch.equal(on, off) and torch.equal(eager_on, eager_off) and torch.equal(on, eager_on)
    assert set(st_on) == set(st_off)
    for k in st_on:
        a, b = st_on[k], st_off[k]
        if isinstance(a, list):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), k
        else:
            assert torch.equal(a, b), k


def test_twoview_sum_on_load_on_off_equal_fullsize(cuda, weights):
    """BASELINE configs[1] (two views 640x512, D=192): both heads sum on load."""
    from atvsnet_amd import ops
    from atvsnet_amd.atvsnet import example as ex
    imgs, cams = _inputs(cuda, 2, 512, 640, 192)
    on = ex.infer_twoview(imgs, cams, 192).clone()
    with ops.configure(head_sum=False):
        off = ex.infer_twoview(imgs, cams, 192).clone()
    assert torch.equal(on, off)


def test_base_stage_outputs_with_and_without_dead_heads(cuda, weights):
    """base_stage_batch(filtered=False / fwd_prob=False) returns exactly the entries the full call returns."""
    from atvsnet_amd.atvsnet import model
    from atvsnet_amd.atvsnet.example import depth_range
    imgs, cams = _inputs(cuda, 3, 128, 160, 32)
    feats = model.feature_extraction_batch(imgs)
    ds, di = depth_range(cams)
    full = model.base_stage_batch(feats, cams, 32, ds, di, fwd=[1, 2], rev=[1, 2])
    rev_only = model.base_stage_batch(feats, cams, 32, ds, di, fwd=[1, 2], rev=[1, 2], fwd_prob=False)
    no_filt = model.base_stage_batch(feats, cams, 32, ds, di, fwd=[1, 2], rev=[1, 2], filtered=False)
    assert rev_only[1] is None and rev_only[2] is None and no_filt[0] is None
    assert torch.equal(rev_only[0], full[0])
    assert torch.equal(no_filt[1], full[1]) and torch.equal(no_filt[2], full[2])
    for v in (1, 2):
        assert torch.equal(rev_only[3][v], full[3][v]) and torch.equal(no_filt[3][v], full[3][v])
