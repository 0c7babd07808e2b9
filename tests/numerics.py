"""Per-element precision bars for the convolution kernels, shared by tests/test_numerics_bar.py (CPU) and
tests/test_gpu_split_precision.py (-m gpu).

A kernel output element is held to its float64 value by

    |got - ref64| <= rel * cond + floor,      cond = the same operation on |x|, |w|, |bias|, |residual|

with floor = Bar.floor * 2^-36 * sum|w| (a scalar, or a per-element tensor where a row needs one: the AANet module, the fp32
rounding of a residual add).

`cond` (sum_i |x_i| |w_i| for one convolution) is what an accumulation error scales with, so the bar does not loosen where an
output cancels to ~0 and does not tighten where it is large: a defect on ONE tile, halo row, sample or Cin chunk fails it as
surely as a defect everywhere.  The floor covers the split's absolute precision below 2^-14, where both fp16 pieces are
subnormal (2^-36 per operand).

The ratios below and the ones assert_elementwise returns are (err - floor) / cond, net of the floor (0 for an element within
it); the floor is significant only in the below-2^-14 regime and on residual adds.

Measured on one MI355X by tests/test_gpu_split_precision.py, largest err / cond over every row and regime except near_max:
split-operand kernels 3.7e-7 (conv1x1_b, log-uniform), fp32 matrix-core / FMA kernels 7.9e-7 (conv2d_lds 128 -> 128 with
dilation 2, log-uniform; 5.1e-7, conv_c16, before the fp32 twins of the split rows were added).  With a
few entries near 6e4 one product dominates cond and every later fp32 add of the accumulator rounds at its ulp, so err / cond
grows with the number of adds: 1.3e-6 split (conv2d_b), 3.3e-6 fp32 (conv2d_lds, dilation 2; conv_tiled 2.8e-6); that regime is
held to NEAR_MAX * rel.
The CPU emulation of the split with float64 accumulation (tests/test_numerics_bar.py) gives at most 2.0e-7 for the correct
split and 3.1e-5 (3x3, Cin 128) for the mildest defect it checks, one tap's low pieces dropped.  SPLIT.rel is 8.1x the
split maximum of the convolution rows and 1/10 of that defect; FP32_MFMA.rel 8.8x the fp32 maximum it was set from (5.1e-7) and
5.7x today's; near_max keeps 18x / 10.9x.
Exception: the AANet module under its linearised bound (aanet_cond) measures 6.4e-7 with log-uniform views, 4.7x under
SPLIT.rel; its cond leaves out the fp32 rounding of the scores and the softmax, which a wider SPLIT.rel may not absorb
without losing the 8x above the one-tap defect.

The fp32 forms of the overflow recompute (the rows under cfg=FP32, ops.configure(split16=False)), largest err / cond per family
over the regimes except near_max | near_max: conv1x1 (plain, on load, G = 3, with a residual) 4.2e-7 | 5.1e-7; conv2d_lds (dilated,
ragged) 7.9e-7 | 3.3e-6; c16 (8 / 16 / 48 -> 16 / 32, D = 1) 5.1e-7 | 2.3e-6; gather (stride 2, the tiny map, the strided conv2)
4.9e-7 | 1.6e-6; tiled 3.8e-7 | 2.8e-6; deconv_up (16 -> 8, 32 -> 16 with G = 3) 3.8e-7 | 1.0e-6; the 64 -> 32 transposed
convolution 4.4e-7 | 1.1e-6 as eight gather launches and 5.8e-7 | 1.3e-6 on conv_tiled (statistics folded by 4); the x-pair kernel
conv_xw under its Winograd cond 7.9e-8 | 4.8e-7, with a plane bias 5.9e-8 | 4.8e-7, with its sibling (plain, a batch norm or a
two-term sum formed on load) 4.2e-7 | 1.0e-6; the three-launch residual unit 6.1e-9 | 3.2e-8 (its cond is the propagated bound
of three convolutions, as the fused unit's: 2.4e-8); offset regime at most 9.3e-9 (conv1x1).  The largest of the convolution
families is conv2d_lds 128 -> 128 with dilation 2 (Cin chunks of a 1152-term sum): FP32_MFMA.rel keeps 5.7x over it, near_max 10.9x.
The fp32 AANet module (conv_c16 scores + aanet_combine, nv = 1, 2, 5, 8, 16, and the three aanet_partial stages at 2 + 3 and
4 + 4 views) measures 3.3e-7 | 2.8e-5 under aanet_cond.  The near_max figure, 0.78 of NEAR_MAX * FP32_MFMA.rel, is the fp32
rounding of U_n = (R_n - S_n) + S_sum, which that cond leaves out: one view's 6e4 entry puts S_sum at up to 2.6e4 for EVERY
view, so every score is rounded at the ulp of S_sum (2^-10) while the other views' own cond R_n + cond S_n is ~ 12 (aanet_b.hip,
3.0e-7 there, takes the softmax of R_n - S_n alone from five views on: the shared sum cancels).  It is the reference's own
arithmetic (fp32 R - S + S_sum): 2.82e-5 at five views and 2.79e-5 at eight, from the single launch and from the partial stages
alike, 2.26e-5 at sixteen on the generic kernel -- and tests/test_numerics_bar.py gets the same three figures on the CPU from
float64 scores with that one add rounded to fp32 (3.8e-9 without S_sum), so the kernels add nothing to it.

A lazy input (a pending batch norm formed on load) enters `cond` as |its float64 normalised value|, which hides the rounding of
the transform itself: about u |mean * rstd|, not u |value|.  The rows with such an input therefore also run the `offset` regime
of tests/bn_ref.py (channel means of 50 to 2e4 standard deviations) against `cond_on_load`, at the row's rel + 2^-22; measured
there: at most 9.3e-9 (conv1x1).
"""
import collections

import torch

Bar = collections.namedtuple('Bar', 'rel floor')        # floor in units of 2^-36 * sum|w| (per output channel, largest)

SPLIT = Bar(3.0e-6, 4.0)          # x = h0 + h1/2048 in fp16, three products on v_mfma_f32_16x16x32_f16, fp32 accumulation
FP32_MFMA = Bar(4.5e-6, 4.0)      # fp32 operands: fp32 matrix cores, or fp32 FMA (stems, 8->1 heads)
NEAR_MAX = 8.0                    # rel factor of the near-6e4 regime (one dominant product)


# ----------------------------------------------------------------------------------------------------------- float64 references

def term64(t):
    """A convolution input in float64 on the CPU: a finished tensor, or relu?((raw - mean) * rstd + beta) of a PendingBN."""
    from atvsnet_amd import ops
    if not isinstance(t, ops.PendingBN):
        return t.cpu().double()
    raw, par = t.raw.cpu().double(), t.params.cpu().double()
    G, C = raw.shape[0], raw.shape[-1]
    if par.dim() == 2:
        par = par.unsqueeze(0).expand(G, -1, -1)
    bc = (G,) + (1,) * (raw.dim() - 2) + (C,)
    v = (raw - par[:, 0].reshape(bc)) * par[:, 1].reshape(bc) + par[:, 2].reshape(bc)
    return torch.clamp(v, min=0) if t.relu else v


def _d(t):
    return term64(t) if _is_pending(t) else t.detach().cpu().double()


def ref64(op, *args, **kw):
    """op (an oracle.tf_ops function, or any function of tensors built from them) in float64.  Tensor arguments (CPU or device,
    or PendingBN) become CPU float64; keyword tensors too."""
    a = [_d(v) if (torch.is_tensor(v) or _is_pending(v)) else v for v in args]
    k = {n: (_d(v) if (torch.is_tensor(v) or _is_pending(v)) else v) for n, v in kw.items()}
    return op(*a, **k)


def cond(op, *args, **kw):
    """The same op in float64 on the absolute values of its tensor operands: sum |x_i| |w_i| (+ |bias| + |residual|) per output
    element for a convolution; for a composition of convolutions, ReLUs and adds, the propagated bound of the same kind.  A lazy
    input enters as |its float64 normalised value|."""
    a = [_d(v).abs() if (torch.is_tensor(v) or _is_pending(v)) else v for v in args]
    k = {n: (_d(v).abs() if (torch.is_tensor(v) or _is_pending(v)) else v) for n, v in kw.items()}
    return op(*a, **k)


def cond_on_load(op, *args, **kw):
    """cond where the rounding of the on-load transform counts (tests/bn_ref.py): the same op on bn_cond = |x s| + |m s| + |b| of
    each lazy operand, which bounds both its normalised value and, times 2u, the transform's error; |x| of any other tensor."""
    import bn_ref

    def a(v):
        if _is_pending(v):
            return bn_ref.bn_cond(v.raw, v.params)
        return _d(v).abs() if torch.is_tensor(v) else v
    return op(*[a(v) for v in args], **{n: a(v) for n, v in kw.items()})


def _is_pending(v):
    from atvsnet_amd import ops
    return isinstance(v, ops.PendingBN)


def floor_of(w, bar):
    """The absolute floor of a bar for a TF kernel w [k.., Cin, Cout] (numpy or tensor): bar.floor * 2^-36 * max_co sum|w|."""
    w = torch.as_tensor(w).double()
    return bar.floor * 2.0 ** -36 * float(w.abs().reshape(-1, w.shape[-1]).sum(0).max())


def assert_elementwise(got, want64, cond64, rel, abs_floor, what=''):
    """|got - want64| <= rel * cond64 + abs_floor at every element (abs_floor: a number or a tensor of want64's shape); returns
    the largest (|got - want64| - abs_floor) / cond64 (the err / cond the bar compares, net of the floor: 0 where an element is
    within it).  On failure names the worst element."""
    got = got.detach().cpu().double()
    want64, cond64 = want64.double(), cond64.double()
    if tuple(got.shape) != tuple(want64.shape) or tuple(cond64.shape) != tuple(want64.shape):
        raise AssertionError('%s: shapes got %s, ref %s, cond %s' % (what, tuple(got.shape), tuple(want64.shape),
                                                                   tuple(cond64.shape)))
    err = (got - want64).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float('inf')))
    ratio = (err - abs_floor).clamp(min=0) / cond64.clamp(min=1e-300)
    ratio = torch.where((err <= abs_floor), torch.zeros_like(ratio), ratio)
    worst = int(torch.argmax(ratio.reshape(-1)))
    r = float(ratio.reshape(-1)[worst])
    if not r <= rel:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), got.shape))
        fl = float(abs_floor[idx]) if torch.is_tensor(abs_floor) else float(abs_floor)
        raise AssertionError('%s: element %s got %.9e, float64 %.9e, cond %.3e: err/cond %.3e > %.1e (floor %.2e)'
                             % (what, idx, float(got[idx]), float(want64[idx]), float(cond64[idx]), r, rel, fl))
    return r


# ---------------------------------------------------------------------------------------------------------- AANet module

def aanet64(X, ws, wu, conv=None):
    """The AANet module (oracle/nets.py attention_aggregation) in float64 for views X (nv, D, H, W, C) -> (D, H, W, C).
    conv(x, w): the score convolution (default: the oracle's in float64); the split emulation passes its own."""
    from oracle import tf_ops as T
    X = X.double()
    conv = conv or (lambda x, w: T.conv(x, w.double(), 1, 'SAME'))
    S, R = conv(X, ws).clamp(min=0), conv(X, wu).clamp(min=0)
    U = R - S + S.sum(0, keepdim=True)
    p = torch.softmax(U, 0)
    return (p * X).sum(0)


def aanet_cond(X, ws, wu):
    """(cond, spread) of the AANet module's output.  Errors dR_n, dS_n of the score convolutions move the scores by
    dU_n = dR_n - dS_n + sum_m dS_m; the shared sum shifts every score alike and cancels in the softmax
    (sum_n p_n (X_n - y) = 0), so the output moves by sum_n p_n (X_n - y) (dR_n - dS_n):
    cond = sum_n p_n |X_n - y| (cond R_n + cond S_n) + sum_n p_n |X_n|  (the last term: the weighted sum's own rounding), and
    spread = sum_n p_n |X_n - y|, which scales the absolute floor of the score convolutions."""
    from oracle import tf_ops as T
    X = X.double()
    S = T.conv(X, ws.double(), 1, 'SAME').clamp(min=0)
    R = T.conv(X, wu.double(), 1, 'SAME').clamp(min=0)
    p = torch.softmax(R - S + S.sum(0, keepdim=True), 0)
    y = (p * X).sum(0)
    cS, cR = T.conv(X.abs(), ws.double().abs(), 1, 'SAME'), T.conv(X.abs(), wu.double().abs(), 1, 'SAME')
    spread = (p * (X - y).abs()).sum(0)
    return (p * (X - y).abs() * (cR + cS)).sum(0) + (p * X.abs()).sum(0), spread


# -------------------------------------------------------------------------------------------------------------- the split

def emulate_split(t):
    """(h0, h1) of DESIGN.md 8 on the CPU, as float32 tensors holding fp16 values: h0 = f16(x), h1 = f16((x - h0) * 2048), so
    that x ~ h0 + h1 / 2048 (22 significant bits; 2^-36 absolute below 2^-14)."""
    x = t.float()
    h0 = x.half().float()
    h1 = ((x - h0) * 2048.0).half().float()
    return h0, h1


# -------------------------------------------------------------------------------------------------------------- poisoning

def nan_bordered(t, border=None):
    """A contiguous device copy of t placed inside a larger allocation that is NaN before and after it.  The border (default: the
    tensor's own size + 4096 floats, rounded to 1024) is wider than any halo plus one Cin chunk a kernel could overrun by, so a
    read outside t meets a NaN."""
    t = t.contiguous()
    n = t.numel()
    if border is None:
        border = ((n + 4096 + 1023) // 1024) * 1024
    buf = torch.full((n + 2 * border,), float('nan'), dtype=t.dtype, device=t.device)
    view = buf[border:border + n].view(t.shape)
    view.copy_(t)
    return view


_POISON_SMALL = 48          # blocks of 512 KiB (the caching allocator's small-block pool)
_POISON_LARGE = (64 << 20, 16 << 20, 4 << 20, 2 << 20)


def poison_allocator(device):
    """Fill and free NaN blocks of the caching allocator's small and large pools, so that the torch.empty calls that follow
    (outputs, float64 statistics partials) hand back NaN bits instead of whatever finite values happened to be there."""
    blocks = [torch.full((bytes_ // 4,), float('nan'), device=device) for bytes_ in _POISON_LARGE]
    blocks += [torch.full((131072,), float('nan'), device=device) for _ in range(_POISON_SMALL)]
    blocks += [torch.full((n,), float('nan'), device=device) for n in (64, 256, 1024, 4096, 16384, 65536)]
    torch.cuda.synchronize(device)
    del blocks


def nan_output(shape, device):
    """An output buffer filled with NaN: the channels a kernel must not write keep these exact bits."""
    return torch.full(tuple(shape), float('nan'), device=device)


def assert_bits_kept(buf, lo, hi):
    """The channels outside [lo, hi) of a NaN-filled output buffer are still the NaN bits nan_output wrote."""
    b = buf.detach().cpu().view(torch.int32)
    want = torch.full((), float('nan')).view(torch.int32)
    outside = torch.cat([b[..., :lo].reshape(-1), b[..., hi:].reshape(-1)])
    bad = int((outside != want).sum())
    assert bad == 0, '%d values outside channels [%d, %d) were written' % (bad, lo, hi)
