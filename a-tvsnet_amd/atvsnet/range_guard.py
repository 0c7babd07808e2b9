"""The fp16-range guard: the sticky non-finite flag of the batch norms (ops.nonfinite_seen), the messages that name its cause,
the fp32 rerun of the host drivers and the rule for the maps in flight when the flag is found up."""
import numpy as np
import torch

from .. import ops
from ..tools.common import Notify

_NONFINITE_HINT = 'the inputs or the weights are not finite (the fp32 kernels have the reference\'s range)'
_RANGE_HINT = ('an activation or weight left the fp16 range of the split-operand kernels (or the inputs were not finite); rerun with '
               'ATVS_SPLIT16=0 for the fp32 kernels')
_fallback_logged = [False]


def fp32_nonfinite(what, too=True):
    """The error of a depth map that is not finite on the fp32 kernels either (`too`: after the split-operand kernels failed)."""
    return FloatingPointError('%s on the fp32 kernels%s: ' % (what, ' too' if too else '') + _NONFINITE_HINT)


def _log_fp32_fallback():
    if not _fallback_logged[0]:
        _fallback_logged[0] = True
        print(Notify.INFO, 'an activation left the fp16 range of the split-operand kernels: this depth map is recomputed on the '
              'fp32 matrix cores (ATVS_SPLIT16=0 selects them from the start)', Notify.ENDC)


def infer_checked(fn, device=None):
    """fn() -> device tensor(s), with the range guard of the host drivers: if a batch norm saw non-finite moments (the sticky
    device flag) or an output is not finite, fn() runs again under ops.configure(split16=False) -- every convolution on the
    fp32 matrix cores, the reference's arithmetic range (cnn_wrapper/network.py:165-167) -- and THAT result is returned.
    FloatingPointError only if the fp32 kernels fail as well (non-finite inputs / weights).  Synchronises."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else device

    def finite(out):
        ts = out if isinstance(out, (list, tuple)) else [out]
        return all(bool(torch.isfinite(t).all()) for t in ts if isinstance(t, torch.Tensor))
    ops.nonfinite_seen(device)                 # start from a clear flag: only THIS map's batch norms count
    out = fn()
    if not ops.nonfinite_seen(device) and finite(out):
        return out
    if not ops.cfg.split16:
        raise fp32_nonfinite('non-finite values', too=False)
    _log_fp32_fallback()
    del out
    with ops.configure(split16=False):
        out = fn()
        bad = ops.nonfinite_seen(device) or not finite(out)
    if bad:
        raise fp32_nonfinite('non-finite values')
    return out


def mark_suspects(device, queues, read_flag=ops.nonfinite_seen):
    """An fp16-range overflow of the split-operand kernels is never returned.  The sticky flag is device-wide and does not say
    WHICH of the maps in flight set it: when it is found up, every busy slot of every queue (anything with `.busy` and
    `.suspect`) becomes suspect, to be recomputed on the fp32 kernels when it is fetched.  The device is synchronised and the
    flag read again first, so that what those maps still raise is cleared with it.  True if the flag was up."""
    if not read_flag(device):
        return False
    torch.cuda.synchronize(device)
    read_flag(device)
    for q in queues:
        q.suspect.update(t for t, b in enumerate(q.busy) if b)
    return True


def check_device(device=None):
    """Raise if a batch norm on `device` saw a non-finite moment since the last check (the sticky flag atvs_bn_finalize sets,
    ops.nonfinite_seen): catches an fp16-range overflow of the split-operand kernels even where a later ReLU swallowed the NaN
    before it could reach the depth map.  Synchronises with the device; GraphedInference.checked() / PipelinedInference.result()
    and the host drivers call it on every result they hand out."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    if ops.nonfinite_seen(device):
        raise FloatingPointError('a batch norm saw non-finite moments: ' + _RANGE_HINT)


def check_finite(arr, what='depth map', flag=True):
    """The split-operand convolutions carry activations as two fp16 pieces: a value beyond +-65504 turns
    into inf/NaN there instead of a silently wrong depth.  The host drivers call this on every result they copy back so that
    the failure names its cause (ATVS_SPLIT16=0 selects the fp32 matrix-core kernels, which have fp32's range)."""
    if flag and torch.cuda.is_available() and torch.cuda.is_initialized():     # flag=False: the caller has read the flag itself
        check_device()
    if not np.isfinite(arr).all():
        raise FloatingPointError('%s holds %d non-finite values: ' % (what, int((~np.isfinite(arr)).sum())) + _RANGE_HINT)
    return arr
