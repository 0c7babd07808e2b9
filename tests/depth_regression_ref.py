"""A float64 reference of the depth regression and confidence kernels (csrc/softargmin.hip), shared by
tests/test_depth_regression_ref_host.py (CPU) and tests/test_gpu_depth_regression.py (-m gpu).

What is an INPUT of the operation is formed in float32 exactly as the kernels and the oracle form it, so that it is no part of the
error: the depth hypotheses (`depths`), the bilinearly interpolated cost (`upsampled`: the same float32 operations in the same
order as the kernels', built with -ffp-contract=off) and the plane indices of the confidence (`planes`: float32 division, floor
and ceil).  What follows is float64: the soft-max over the depth axis, the expectation, the four gathered terms.

    want = sum_d p_d v_d,     cond = sum_d p_d |v_d|,     p = softmax(-cost) in float64

cond is what the rounding of the weighted sum scales with; a depth is held to |got - want| <= REL * cond, a soft-max confidence
to PROB_ABS absolute (a sum of at most four probabilities, at most 2 where an integral coordinate counts its plane twice).
"""
import torch

from oracle import model as OM

REL = 2e-6          # the project's soft-argmin tolerance, here against float64 and per element
PROB_ABS = 2e-6     # the project's tolerance of the soft-max confidence (tests/test_gpu_probmap.py), likewise

REGIMES = ('flat', 'typical', 'peaked', 'decreasing')
_SCALE = {'flat': 0.5, 'typical': 6.0, 'peaked': 30.0, 'decreasing': 6.0}


def _f32(x):
    return torch.as_tensor(x, dtype=torch.float32).reshape(())


def depths(start, interval, D):
    """The float32 hypotheses v_d as linspace_step() of the kernels and oracle.tf_ops.linspace form them."""
    start, interval = _f32(start), _f32(interval)
    if D == 1:
        return start.reshape(1).clone()
    end = start + (torch.tensor(float(D), dtype=torch.float32) - 1.0) * interval
    step = (end - start) / torch.tensor(float(D - 1), dtype=torch.float32)
    return start + step * torch.arange(D, dtype=torch.float32)


def upsampled(cost, up):
    """cost (D,h,w) float32 -> (D, h*up, w*up): the oracle's align_corners bilinear interpolation, in float32."""
    assert cost.dtype == torch.float32 and cost.dim() == 3
    return OM.upsample_prob_vol(cost[None], up)[0]


def softargmin64(vol, v):
    """vol (D,H,W), v (D,) -> (want, cond), both (H,W) float64."""
    D = vol.shape[0]
    p = torch.softmax(-vol.double(), 0)
    vv = v.double().reshape(D, 1, 1)
    return (p * vv).sum(0), (p * vv.abs()).sum(0)


def planes(depth, start, interval, D):
    """(l0, l1, r0, r1), int64 of depth's shape: the planes the kernel must choose.  dc = (depth - start) / interval in float32;
    l0 = clip(floor(dc)), l1 = clip(l0 - 1), r0 = clip(ceil(dc)), r1 = clip(r0 + 1), each clipped to [0, D-1].  A dc that is not
    finite is not taken through a cast; its planes are stated:
        NaN, -inf -> (0, 0, 0, min(1, D-1))             (the conversion gives 0 / the most negative integer, clipped to 0)
        +inf      -> (D-1, max(D-2, 0), D-1, D-1)       (the conversion saturates, clipped to D-1)"""
    dc = (depth.float() - _f32(start)) / _f32(interval)
    fin = torch.isfinite(dc)
    safe = torch.where(fin, dc, torch.zeros_like(dc))
    l0 = torch.clamp(torch.floor(safe).to(torch.int64), 0, D - 1)
    r0 = torch.clamp(torch.ceil(safe).to(torch.int64), 0, D - 1)
    high = dc == float('inf')
    low = ~fin & ~high
    l0 = torch.where(low, torch.zeros_like(l0), torch.where(high, torch.full_like(l0, D - 1), l0))
    r0 = torch.where(low, torch.zeros_like(r0), torch.where(high, torch.full_like(r0, D - 1), r0))
    l1 = torch.clamp(l0 - 1, 0, D - 1)
    r1 = torch.clamp(r0 + 1, 0, D - 1)
    return l0, l1, r0, r1


def _gather(P, idx):
    D = P.shape[0]
    return torch.gather(P.reshape(D, -1), 0, idx.reshape(1, -1)).reshape(idx.shape)


def probmap64(vol, depth, start, interval, softmax):
    """vol (D,H,W) float32 (already at depth's resolution), depth (H,W) -> (H,W) float64: the four terms gathered from the float64
    soft-max of -vol (softmax) or from vol itself, and summed."""
    D = vol.shape[0]
    P = torch.softmax(-vol.double(), 0) if softmax else vol.double()
    return sum(_gather(P, i) for i in planes(depth, start, interval, D))


def probmap32_plain(vol, depth, start, interval):
    """The plain form as the kernel states it: a gather and ((P[l0] + P[l1]) + P[r0]) + P[r1] in float32."""
    l0, l1, r0, r1 = planes(depth, start, interval, vol.shape[0])
    return ((_gather(vol, l0) + _gather(vol, l1)) + _gather(vol, r0)) + _gather(vol, r1)


# ------------------------------------------------------------------------------------------------------------------ the cases

def costs(regime, shape, seed):
    """A seeded cost volume: flat 0.5 * randn (every plane carries weight), typical 6 * randn, peaked 30 * randn (a handful
    of planes carry everything); decreasing = typical, run on a sweep of negative interval.
    The flat regime's normal is cut at +-2 sigma: its purpose is that every plane carries at least 1 / (8 D), and the plain
    0.5 * randn misses that at these sample counts (0.10 / D at 63 x 3 x 130, where the largest of 25 k samples is beyond 4 sigma).
    With |cost| <= 1 the smallest weight is at least 1 / (1 + (D - 1) e^2) >= 1 / (8 D) for every D, through the interpolation
    too (a convex combination stays in the range)."""
    g = torch.Generator().manual_seed(int(seed))
    z = torch.randn(tuple(shape), generator=g)
    if regime == 'flat':
        z = z.clamp(-2.0, 2.0)
    return _SCALE[regime] * z


def sweep(regime, D):
    """(depth_start, depth_interval) as 1-element float32 tensors: a different positive sweep per regime, one of them dyadic (the
    plane coordinate of a hypothesis is then exactly integral), and a decreasing one."""
    ds, di = {'flat': (0.5, 2.0 ** -6), 'typical': (0.4, 0.05), 'peaked': (0.05, 0.31 / D),
              'decreasing': (0.36, -0.31 / D)}[regime]
    return torch.tensor([ds]), torch.tensor([di])


def one_hot(D, h, w, k):
    """cost +100 everywhere, -100 at plane k (h,w int64) of each pixel: exp(-200) is 0 in float32, the answer is v_k itself."""
    cost = torch.full((D, h * w), 100.0)
    cost.scatter_(0, k.reshape(1, -1), -100.0)
    return cost.reshape(D, h, w)


def boundary_planes(D):
    """Plane indices where a kernel changes hands: the ends, the four wavefronts' ranges D*wv/4, the 64-plane chunks."""
    ks = {0, D - 1, D // 2}
    for wv in range(1, 4):
        ks.update((D * wv // 4 - 1, D * wv // 4))
    for c in range(64, D + 1, 64):
        ks.update((c - 1, c, c + 1))
    return sorted(k for k in ks if 0 <= k < D)


def depth_map(H, W, start, interval, D, seed):
    """(H,W) float32 depths for the confidence: uniformly inside and two intervals beyond the sweep, then (first pixels) exactly
    on hypotheses 0, 3 and D-1, one float32 ulp to either side of each, NaN, +inf, -inf."""
    v = depths(start, interval, D)
    step = abs(float(_f32(interval)))
    lo = min(float(v[0]), float(v[-1])) - 2 * step
    g = torch.Generator().manual_seed(int(seed))
    d = (lo + step * (D + 3) * torch.rand(H * W, generator=g)).float()
    on = torch.stack([v[0], v[min(3, D - 1)], v[D - 1]])
    big = torch.tensor(float('inf'))
    special = torch.cat([on, torch.nextafter(on, big), torch.nextafter(on, -big),
                         torch.tensor([float('nan'), float('inf'), -float('inf')])])
    assert H * W >= special.numel(), 'the depth map is too small for the special values'
    d[:special.numel()] = special
    return d.reshape(H, W)
