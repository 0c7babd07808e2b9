"""View preparation of the scene driver: uint8 BGR image on the device -> network input + 1/4-scale image (csrc/prepare.hip).

The tap indices and 11-bit weights are formed on the host by preprocess.resize_taps_u8 (scale_image's own code), once per (source
size, scale, crop window), and only for the rows / columns inside the window; the kernel evaluates scale_image's integer formula on
them, so the resize is bit for bit the numpy one.  `resize_u8_host` is that formula in numpy on the same taps (the CPU tests pin it
against scale_image).  Centring: exact integer sums, mu and sd in double (center_image forms them with float32 sums; the two may
differ in the last bits of the output, DESIGN.md "Scene mode").
"""


import numpy as np
import torch

from .base import _call, _p, _stream

_plans = {}


def _axis_taps(n_src, scale, start, count):
    """(4, count) int32: left, right, left weight, right weight of output samples start .. start+count-1 of an axis of n_src
    samples resized by `scale` (scale_image's step 1/scale)."""
    from ..atvsnet.preprocess import resize_taps_u8
    n_dst = int(np.rint(n_src * scale))
    if not (0 <= start and count >= 1 and start + count <= n_dst):
        raise ValueError('prepare: window %d+%d outside the %d resized samples' % (start, count, n_dst))
    taps = np.stack(resize_taps_u8(n_dst, n_src, 1.0 / scale), 0)[:, start:start + count]
    if taps[:2].min() < 0 or taps[:2].max() >= n_src:
        raise ValueError('prepare: tap outside the source axis')       # resize_taps_u8 clamps: never expected
    return np.ascontiguousarray(taps, dtype=np.int32)


def prepare_taps(h, w, scale, crop, sample_scale=0.25):
    """Host taps of one view: ((ytap, xtap) of the scaled + cropped image, (ytap, xtap) of its sample_scale image).
    crop = (y0, x0, rows, cols) in the scaled image (preprocess.crop_window)."""
    y0, x0, nh, nw = (int(v) for v in crop)
    main = (_axis_taps(h, scale, y0, nh), _axis_taps(w, scale, x0, nw))
    qh, qw = int(np.rint(nh * sample_scale)), int(np.rint(nw * sample_scale))
    quarter = (_axis_taps(nh, sample_scale, 0, qh), _axis_taps(nw, sample_scale, 0, qw)) if min(qh, qw) >= 1 else None
    return main, quarter


def resize_u8_host(src, ytap, xtap):
    """The kernel's integer formula evaluated in numpy on host taps: src (h,w,3) uint8 -> (len(ytap[0]), len(xtap[0]), 3)."""
    p = np.asarray(src).astype(np.int64)
    y0, y1, by0, by1 = (t.astype(np.int64) for t in ytap)
    x0, x1, ax0, ax1 = (t.astype(np.int64) for t in xtap)
    horiz = p[:, x0] * ax0[None, :, None] + p[:, x1] * ax1[None, :, None]
    top, bot = horiz[y0] >> 4, horiz[y1] >> 4
    acc = ((by0[:, None, None] * top) >> 16) + ((by1[:, None, None] * bot) >> 16)
    return np.clip((acc + 2) >> 2, 0, 255).astype(np.uint8)


class ViewPlan(object):
    """Device taps of one (source size, scale, crop window, sample scale) and the output shapes.  The taps are uploaded from pinned
    memory on the current stream; `ready` is recorded there (a user on another stream waits for it: prepare_view does)."""

    def __init__(self, h, w, scale, crop, sample_scale, device):
        (my, mx), quarter = prepare_taps(h, w, scale, crop, sample_scale)
        if quarter is None:                     # a window of under 2 rows / columns has no sample_scale image
            quarter = tuple(np.zeros((4, 0), np.int32) for _ in range(2))
        qy, qx = quarter
        self.src_shape = (h, w, 3)
        self.shape = (my.shape[1], mx.shape[1], 3)
        self.quarter_shape = (qy.shape[1], qx.shape[1], 3)
        self.taps = [torch.from_numpy(t).pin_memory().to(device, non_blocking=True) for t in (my, mx, qy, qx)]
        self.ready = torch.cuda.Event()
        self.ready.record(torch.cuda.current_stream(device))


def view_plan(h, w, scale, crop, sample_scale=0.25, device=None):
    """The cached ViewPlan (build it before a graph capture: forming one uploads the taps, on the current stream)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    key = (int(h), int(w), float(scale), tuple(int(v) for v in crop), float(sample_scale), str(device))
    p = _plans.get(key)
    if p is None:
        p = _plans[key] = ViewPlan(int(h), int(w), float(scale), crop, float(sample_scale), device)
    return p


def prepare_workspace(plan, device):
    """(cropped uint8 (H,W,3), sums (6,) int64) scratch of prepare_view."""
    return (torch.empty(plan.shape, dtype=torch.uint8, device=device), torch.empty(6, dtype=torch.int64, device=device))


def prepare_view(image, scale, crop, sample_scale=0.25, out=None, taps=None):
    """image (h,w,3) uint8 BGR on the device -> (centred (H,W,3) float32, sample_scale image (H/4,W/4,3) uint8):
    scale_image(image, scale) cropped to `crop` = (y0, x0, H, W), center_image of it, scale_image(cropped, sample_scale).
    out: (centred, quarter, cropped, sums) buffers to write (captured graphs); taps: device tap tensors replacing the plan's
    (static buffers of a captured graph, same shapes).  meta tensors: shapes only."""
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or not image.is_contiguous():
        raise ValueError('prepare_view: a contiguous (h,w,3) uint8 image, got %s %s' % (image.dtype, tuple(image.shape)))
    h, w = int(image.shape[0]), int(image.shape[1])
    dev = image.device
    if dev.type == 'meta':
        y0, x0, nh, nw = (int(v) for v in crop)
        q = (int(np.rint(nh * sample_scale)), int(np.rint(nw * sample_scale)), 3)
        return (torch.empty((nh, nw, 3), dtype=torch.float32, device=dev), torch.empty(q, dtype=torch.uint8, device=dev))
    if dev.type != 'cuda':
        raise RuntimeError('prepare_view runs on the MI355X only: got a %s tensor and there is no CPU fallback' % dev.type)
    plan = view_plan(h, w, scale, crop, sample_scale, dev)
    if out is None:
        out = (torch.empty(plan.shape, dtype=torch.float32, device=dev), torch.empty(plan.quarter_shape, dtype=torch.uint8, device=dev)) \
            + prepare_workspace(plan, dev)
    centred, quarter, cropped, sums = out
    if (tuple(centred.shape) != plan.shape or tuple(quarter.shape) != plan.quarter_shape or tuple(cropped.shape) != plan.shape
            or centred.dtype != torch.float32 or quarter.dtype != torch.uint8 or cropped.dtype != torch.uint8
            or sums.dtype != torch.int64 or sums.numel() < 6):
        raise ValueError('prepare_view: output buffers do not match the plan')
    if taps is None and not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream(dev).wait_event(plan.ready)      # the plan may have been formed on another stream
    my, mx, qy, qx = plan.taps if taps is None else taps
    for a, b in zip((my, mx, qy, qx), plan.taps):
        if a.shape != b.shape or a.dtype != torch.int32:
            raise ValueError('prepare_view: tap buffers do not match the plan')
    H, W = plan.shape[:2]
    _call('atvs_prepare_resize_u8', _p(image), h, w, _p(cropped), H, W, _p(my), _p(mx), _p(sums), _stream())
    _call('atvs_prepare_center', _p(cropped), H * W, _p(sums), _p(centred), _stream())
    if quarter.numel():
        _call('atvs_prepare_resize_u8', _p(cropped), H, W, _p(quarter), int(quarter.shape[0]), int(quarter.shape[1]), _p(qy),
              _p(qx), None, _stream())
    return centred, quarter
