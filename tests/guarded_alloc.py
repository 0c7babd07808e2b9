"""Guard bands and dirty scratch for the ops that take caller-owned buffers (tests/test_gpu_buffer_contract.py, -m gpu;
tests/test_guarded_alloc_host.py proves on the CPU that every check here can fail).

`guarded(device, fill)` patches torch.empty / empty_like / zeros / zeros_like / full for the block.  An allocation on `device`
becomes a slice of one uint8 buffer

    guard | payload, rounded up to 256 bytes | guard          guard = max(64 KiB, the payload's size), rounded up to 256 bytes

taken from the original torch.empty; the tensor handed out is the payload, 256-byte aligned, in the dtype and shape asked for.
`empty` payloads hold the byte `fill` (0x00 and 0xFF make two runs that differ in every bit an op reads without having written
it); `zeros` and `full` payloads hold what was asked for.  The guards and the round-up tail hold PATTERN, a function of the byte's
position alone, so a kernel that writes the fill value outside its payload is still seen.  `check()` names every allocation whose
guard or tail changed, and every `place`d input whose bits changed.  All buffers live until the block ends: nothing is recycled
into another allocation in between.

`recording_lib()` puts a proxy in front of the loaded library that notes the name of each entry point called.
`run_contract(...)` is the three-run comparison (plain, fill 0x00, fill 0xFF) both test files share.

Three additions serve the network side (tests/network_contract_rows.py, tests/test_gpu_network_contract.py):

Slice masks.  Many network ops write a channel range of a caller's wider buffer.  `place(t, writable=<bool mask | (lo, hi) of the
last axis>)` remembers the bits of every element the op may NOT write; `check()` reports such an element that changed with its flat
index.  The buffer must hold a position-dependent pattern (the rows' `ramp`): a kernel that copies a neighbour's value over a
neighbour then still changes it.

Arranged weights.  ops/packing.py packs on the host and uploads with `.to(device)`, which no patch of torch.empty sees.
`weights_under(place, **switches)` is `ops.configure(clear_pack_cache=True, **switches)` in which every `_Packed.wp` / `.tab` that a
packer assigns becomes `place(...)` of it, so the launch reads its weights from a guarded allocation whose next byte is the
pattern: a read-ahead beyond "one zero chunk behind the last" meets pattern bytes, which differ from what the plain run's
allocator holds there, and a store meets the guard.  The caches are cleared on entry and on exit and asserted empty afterwards.

Pooled device words.  ops.nonfinite_flag, _fin_counter, _side_stream and prepare_workspace make a device buffer on first use and
KEEP it.  Made inside a guarded block it would be a payload of that block: a 0xFF-filled flag word that the next test reads as
"a non-finite moment was seen", and memory that is released with the block while the pool still points into it.  So
`run_contract(warm=...)` touches the pools before the first run, and `pools=` (-> [(name, tensor)]) is asserted inside every block,
before the guards are dropped, to hold no tensor whose address lies in one of the block's buffers (`guarded.owns`).
"""
import collections
import contextlib
import linecache
import os
import sys

import torch

GUARD = 64 << 10
ALIGN = 256
_PATCHED = ('empty', 'empty_like', 'zeros', 'zeros_like', 'full')
_ORIGINAL = {name: getattr(torch, name) for name in _PATCHED}
_HERE = os.path.abspath(__file__)
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

Allocation = collections.namedtuple('Allocation', 'site line code nbytes kind shape dtype')      # code: 'function: source line'


def _round_up(n, to=ALIGN):
    return (n + to - 1) // to * to


def pattern(start, stop, device):
    """Bytes start..stop-1 of the guard pattern: a function of the position in the buffer alone, never constant over a run."""
    i = torch.arange(start, stop, dtype=torch.int64, device=device)
    return ((i * 167 + (i >> 8) * 13 + 0x5A) & 0xFF).to(torch.uint8)


def _site():
    """(file, line number, function, source line) of the nearest frame outside this helper (and outside the one-line allocation
    helper ops.base._new): the product line that allocated."""
    f = sys._getframe(1)
    while f is not None:
        name = os.path.abspath(f.f_code.co_filename)
        if name != _HERE and not (f.f_code.co_name == '_new' and name.endswith(os.path.join('ops', 'base.py'))):
            return name, f.f_lineno, f.f_code.co_name, linecache.getline(name, f.f_lineno).strip()
        f = f.f_back
    return '?', 0, '?', ''


def bits(t):
    """t on the CPU as integers of its element size: NaN payloads and the sign of a zero count."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    if t.dtype.is_floating_point or t.dtype.is_complex:
        return t.view(_INT_OF_SIZE[t.element_size()])
    return t


class _Buffer(object):
    __slots__ = ('raw', 'start', 'nbytes', 'guard', 'payload', 'record', 'kept', 'mask')


class guarded(object):
    def __init__(self, device, fill):
        self.device = torch.device(device)
        self.fill = int(fill) & 0xFF
        self.allocations = []
        self._buffers = []
        self._active = False

    # ------------------------------------------------------------------------------------------------------------ patching
    def __enter__(self):
        if any(getattr(torch, n) is not _ORIGINAL[n] for n in _PATCHED):
            raise RuntimeError('guarded blocks do not nest')
        torch.empty = self._empty
        torch.empty_like = self._empty_like
        torch.zeros = self._zeros
        torch.zeros_like = self._zeros_like
        torch.full = self._full
        self._active = True
        return self

    def __exit__(self, *exc):
        for n in _PATCHED:
            setattr(torch, n, _ORIGINAL[n])
        self._active = False
        self._buffers = []
        return False

    def _mine(self, device):
        if device is None:
            device = torch.get_default_device() if hasattr(torch, 'get_default_device') else torch.device('cpu')
        d = torch.device(device)
        if d.type != self.device.type:
            return False
        if d.type != 'cuda':
            return True
        cur = torch.cuda.current_device()
        return (cur if d.index is None else d.index) == (cur if self.device.index is None else self.device.index)

    @staticmethod
    def _shape(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        return tuple(int(s) for s in size)

    def _plain(self, kw):
        """True when the request is an ordinary dense allocation this guard can stand in for."""
        return (kw.get('out') is None and kw.get('layout', torch.strided) == torch.strided and not kw.get('pin_memory', False)
                and kw.get('memory_format', torch.contiguous_format) in (torch.contiguous_format, torch.preserve_format)
                and not kw.get('requires_grad', False) and kw.get('names') is None)

    def _empty(self, *size, **kw):
        if not self._mine(kw.get('device')) or not self._plain(kw):
            return _ORIGINAL['empty'](*size, **kw)
        return self._allocate(self._shape(size), kw.get('dtype') or torch.get_default_dtype(), 'empty')

    def _zeros(self, *size, **kw):
        if not self._mine(kw.get('device')) or not self._plain(kw):
            return _ORIGINAL['zeros'](*size, **kw)
        return self._allocate(self._shape(size), kw.get('dtype') or torch.get_default_dtype(), 'zeros').zero_()

    def _full(self, size, fill_value, **kw):
        if not self._mine(kw.get('device')) or not self._plain(kw):
            return _ORIGINAL['full'](size, fill_value, **kw)
        dtype = kw.get('dtype')
        if dtype is None:
            dtype = _ORIGINAL['full']((), fill_value).dtype
        return self._allocate(self._shape((size,)), dtype, 'full').fill_(fill_value)

    def _empty_like(self, t, **kw):
        if not self._mine(kw.get('device', t.device)) or not self._plain(kw) or not t.is_contiguous():
            return _ORIGINAL['empty_like'](t, **kw)
        return self._allocate(tuple(t.shape), kw.get('dtype') or t.dtype, 'empty_like')

    def _zeros_like(self, t, **kw):
        if not self._mine(kw.get('device', t.device)) or not self._plain(kw) or not t.is_contiguous():
            return _ORIGINAL['zeros_like'](t, **kw)
        return self._allocate(tuple(t.shape), kw.get('dtype') or t.dtype, 'zeros_like').zero_()

    # ---------------------------------------------------------------------------------------------------------- allocating
    def _allocate(self, shape, dtype, kind, site=None):
        item = _ORIGINAL['empty']((), dtype=dtype).element_size()
        count = 1
        for s in shape:
            count *= s
        nbytes = count * item
        b = _Buffer()
        b.nbytes, b.guard = nbytes, _round_up(max(GUARD, nbytes))
        total = 2 * b.guard + _round_up(nbytes)
        b.raw = _ORIGINAL['empty'](total + ALIGN, dtype=torch.uint8, device=self.device)
        b.start = b.guard + (-b.raw.data_ptr()) % ALIGN          # the payload begins on a 256-byte address
        lo, hi = b.start - b.guard, b.start + _round_up(nbytes) + b.guard
        b.raw[lo:b.start] = pattern(lo, b.start, self.device)
        b.raw[b.start + nbytes:hi] = pattern(b.start + nbytes, hi, self.device)
        b.raw[b.start:b.start + nbytes] = self.fill
        b.payload = b.raw[b.start:b.start + nbytes].view(dtype).reshape(shape)
        assert b.payload.is_contiguous() and b.payload.data_ptr() % ALIGN == 0
        name, line, function, text = site or _site()
        b.record = Allocation(name, line, function + ': ' + text, nbytes, kind, shape, dtype)
        b.kept = b.mask = None
        self.allocations.append(b.record)
        self._buffers.append(b)
        return b.payload

    def place(self, t, writable=False):
        """A copy of `t` inside a guarded allocation of this block's device.  Its bits are remembered: check() reports a placed
        input that changed, unless `writable` is True (an operand the op rewrites in place: only its guards are held).
        writable = a bool tensor of t's shape (True: the op may write the element), or (lo, hi): the op may write [..., lo:hi] of
        the last axis and nothing else -- check() reports every other element that changed."""
        if not self._active:
            raise RuntimeError('place() outside the guarded block')
        src = t.detach().contiguous()
        out = self._allocate(tuple(src.shape), src.dtype, 'input', _site())
        out.copy_(src)
        b = self._buffers[-1]
        if writable is not True:
            b.kept = _ORIGINAL['empty'](tuple(src.shape), dtype=src.dtype, device=self.device).copy_(src)
        if writable is not True and writable is not False:
            b.mask = writable_mask(writable, tuple(src.shape)).to(self.device)
        return out

    def owns(self, t):
        """Does the tensor's first byte lie inside one of this block's buffers (guards included)?"""
        a = t.data_ptr()
        return any(b.raw.data_ptr() <= a < b.raw.data_ptr() + b.raw.numel() for b in self._buffers)

    # ------------------------------------------------------------------------------------------------------------ checking
    def check(self):
        """Synchronises; raises ONE AssertionError that lists every guard or tail byte that changed (allocation site, shape and
        dtype, side, first and last offending byte offset relative to the payload's start) and every placed input that changed."""
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        if not self._buffers:
            return
        flags = []
        for b in self._buffers:
            lo, hi = b.start - b.guard, b.start + _round_up(b.nbytes) + b.guard
            flags.append((b.raw[lo:b.start] != pattern(lo, b.start, self.device)).any())
            flags.append((b.raw[b.start + b.nbytes:hi] != pattern(b.start + b.nbytes, hi, self.device)).any())
            same = torch.tensor(True, device=self.device) if b.kept is None else _same_bits_device(b.payload, b.kept, b.mask)
            flags.append(~same)
        flags = torch.stack(flags).cpu().reshape(-1, 3).tolist()
        found = []
        for b, (before, after, changed) in zip(self._buffers, flags):
            r = b.record
            what = '%s:%d (%s) %s %s %s, %d bytes' % (r.site, r.line, r.code, r.kind, tuple(r.shape), r.dtype, r.nbytes)
            lo, hi = b.start - b.guard, b.start + _round_up(b.nbytes) + b.guard
            if before:
                bad = torch.nonzero(b.raw[lo:b.start] != pattern(lo, b.start, self.device)).reshape(-1).cpu()
                found.append('%s: %d bytes BEFORE the payload changed, offsets %d .. %d' % (
                    what, len(bad), int(bad[0]) - b.guard, int(bad[-1]) - b.guard))
            if after:
                bad = torch.nonzero(b.raw[b.start + b.nbytes:hi] != pattern(b.start + b.nbytes, hi, self.device)).reshape(-1).cpu()
                first, last = int(bad[0]) + b.nbytes, int(bad[-1]) + b.nbytes
                where = 'in the round-up tail' if last < _round_up(b.nbytes) else 'past the 256-byte round-up'
                found.append('%s: %d bytes AFTER the payload changed (%s), offsets %d .. %d' % (what, len(bad), where, first, last))
            if changed:
                ne = bits(b.payload).reshape(-1) != bits(b.kept).reshape(-1)
                if b.mask is not None:
                    ne &= ~b.mask.reshape(-1).cpu()
                diff = torch.nonzero(ne).reshape(-1)
                found.append('%s: %s, %d elements, first %d' % (what, 'the placed INPUT changed' if b.mask is None else
                                                               'elements OUTSIDE the writable slice changed', len(diff), int(diff[0])))
        if found:
            raise AssertionError('%d buffer violations:\n  %s' % (len(found), '\n  '.join(found)))

    def address(self, index):
        """The address of the payload of allocation `index` (of `allocations`), also where it has no byte."""
        b = self._buffers[index]
        return b.raw.data_ptr() + b.start

    def summary(self, kinds=('empty', 'empty_like', 'zeros', 'zeros_like', 'full')):
        mine = [a for a in self.allocations if a.kind in kinds]
        return len(mine), sum(a.nbytes for a in mine)


def _same_bits_device(a, b, mask=None):
    """Do a and b hold the same bits -- with `mask` (True: writable), wherever the mask is False?"""
    if a.numel() == 0:
        return torch.tensor(True, device=a.device)
    item = a.element_size()
    same = a.contiguous().reshape(-1).view(torch.uint8) == b.contiguous().reshape(-1).view(torch.uint8)
    if mask is not None:
        same = same.reshape(-1, item) | mask.reshape(-1, 1)
    return same.all()


def writable_mask(spec, shape):
    """A bool tensor of `shape`, True where the op may write: spec is such a tensor, or (lo, hi) of the last axis."""
    if isinstance(spec, torch.Tensor):
        if spec.dtype != torch.bool or tuple(spec.shape) != tuple(shape):
            raise ValueError('a writable mask is a bool tensor of the placed tensor\'s shape %s, got %s %s' % (shape, spec.dtype, tuple(spec.shape)))
        return spec.contiguous()
    lo, hi = spec
    if not 0 <= lo <= hi <= shape[-1]:
        raise ValueError('writable range %s of a last axis of %d' % ((lo, hi), shape[-1]))
    m = _ORIGINAL['zeros'](shape, dtype=torch.bool)           # (the original: a mask is no allocation of the op under test)
    m[..., lo:hi] = True
    return m


# ----------------------------------------------------------------------------------------------------------------- the library
class _Recorder(object):
    def __init__(self, lib, calls):
        object.__setattr__(self, '_lib', lib)
        object.__setattr__(self, '_calls', calls)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('atvs_'):
            return fn
        calls = self._calls

        def recorded(*args):
            calls.append(name)
            return fn(*args)
        return recorded


@contextlib.contextmanager
def recording_lib(lib_module=None):
    """`with recording_lib() as calls:` -- the names of the library's entry points called inside the block, in order.  Patched onto
    `_lib.lib`, which ops.base._call and ops.base._size reach through the module."""
    if lib_module is None:
        from atvsnet_amd import _lib as lib_module
    calls, original = [], lib_module.lib

    def lib():
        return _Recorder(original(), calls)
    lib_module.lib = lib
    try:
        yield calls
    finally:
        lib_module.lib = original


# ------------------------------------------------------------------------------------------------------------ the three runs
def assert_same_bits(runs, names, what=''):
    """runs: {run name: [tensor, ...]} -- every list has the same length, dtypes and shapes, and the same bits."""
    first_name = next(iter(runs))
    first = runs[first_name]
    found = []
    for name, got in runs.items():
        if len(got) != len(first):
            found.append('%s: %d selected tensors, %s has %d' % (name, len(got), first_name, len(first)))
            continue
        for k, (a, b) in enumerate(zip(first, got)):
            label = names[k] if k < len(names) else '#%d' % k
            if (a is None) != (b is None):
                found.append('%s: %s is None in one run only' % (name, label))
                continue
            if a is None:
                continue
            if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
                found.append('%s: %s is %s %s, %s has %s %s' % (name, label, b.dtype, tuple(b.shape), first_name, a.dtype, tuple(a.shape)))
                continue
            ne = torch.nonzero(bits(a).reshape(-1) != bits(b).reshape(-1)).reshape(-1)
            if len(ne):
                i = int(ne[0])
                found.append('%s: %s differs from %s in %d of %d elements, first at flat index %d: %r against %r' % (
                    name, label, first_name, len(ne), a.numel(), i, a.detach().cpu().reshape(-1)[i].item(),
                    b.detach().cpu().reshape(-1)[i].item()))
    if found:
        raise AssertionError('%s: the runs differ:\n  %s' % (what, '\n  '.join(found)))


Contract = collections.namedtuple('Contract', 'guards selected')


def _identity(t, **kw):
    return t


@contextlib.contextmanager
def _no_weights(place):
    yield


@contextlib.contextmanager
def weights_under(place, ops=None, **switches):
    """`ops.configure(clear_pack_cache=True, **switches)` in which every arranged-weight tensor a packer assigns to a `_Packed`
    (`pk.wp`, `pk.tab`) is replaced by `place(...)` of it: with the guard's place, the launch reads its weights from a guarded
    allocation.  With place None (the plain run) only the switches and the fresh caches remain.  No arranged form may stay in the
    four caches after the block."""
    if ops is None:
        from atvsnet_amd import ops
    packed = ops._Packed
    caches = (ops._pack_cache, ops._fold_cache, ops._virt_cache, ops._xp_cache)

    def set_placed(self, name, value):
        if name in ('wp', 'tab') and isinstance(value, torch.Tensor) and value.device.type != 'meta':
            value = place(value)
        object.__setattr__(self, name, value)
    with ops.configure(clear_pack_cache=True, **switches):
        assert not any(caches), 'the arranged-weight caches were not cleared on entry'
        if place is not None:
            assert '__setattr__' not in vars(packed)
            packed.__setattr__ = set_placed
        try:
            yield
        finally:
            if place is not None:
                del packed.__setattr__
    left = [len(c) for c in caches]
    assert not any(left), 'arranged weights stayed in the caches after the block (pack, fold, virt, xp): %s' % left


def run_contract(run, inputs, select, device, names=(), writable=(), fills=(0x00, 0xFF), what='', warm=None, pools=None,
                 around=_no_weights):
    """The contract of one op at one input.  inputs: {name: CPU tensor or anything else}; run(d, place) -> result with d = the
    inputs on `device` (tensors moved, the rest as it is) and place = the guard's place (the identity in the plain run);
    select(result) -> [tensor or None, ...], the specified part of the result.  Runs plain, then under guarded(fill) for each
    fill with every tensor input placed.  writable: the names the op rewrites in place, or {name: True | bool mask | (lo, hi) of
    the last axis}: what of that input the op may write (`place`).  Asserts that no guard, tail, input or masked element changed
    and that the selections have the same bits in every run.
    warm(): called once before the first run, to make every pooled device buffer the op keeps (a flag word, a counter pool)
    outside the blocks.  pools() -> [(name, tensor)]: asserted inside every block, before its buffers are dropped, to hold no
    tensor of the block.  around(place): a context manager around each of the three runs (place None in the plain one), e.g.
    `weights_under`.
    -> Contract(guards = {fill: the guard}, selected = the plain run's selection on the CPU) for the caller's own assertions."""
    if not isinstance(writable, dict):
        writable = {k: True for k in writable}

    def on_device(place):
        d = {}
        for k, v in inputs.items():
            if isinstance(v, torch.Tensor):
                v = place(v.to(device), writable=writable.get(k, False))
            d[k] = v
        return d

    def keep(selection):
        return [None if t is None else t.detach().cpu().clone() for t in selection]

    def clone(t, **kw):                   # the plain run works on a copy: `inputs` may live on `device` already
        return t.clone()
    if warm is not None:
        warm()
    runs = collections.OrderedDict()
    with around(None):
        runs['plain'] = keep(select(run(on_device(clone), _identity)))
    guards = {}
    violations = []
    for fill in fills:
        with guarded(device, fill) as g:
            with around(g.place):
                d = on_device(g.place)
                runs['fill 0x%02X' % fill] = keep(select(run(d, g.place)))
                try:
                    g.check()
                except AssertionError as e:
                    violations.append('fill 0x%02X: %s' % (fill, e))
            leaked = [name for name, t in (pools() if pools is not None else ()) if g.owns(t)]
            if leaked:
                violations.append('fill 0x%02X: pooled buffers made inside the guarded block, which outlive it: %s' % (fill, ', '.join(leaked)))
            guards[fill] = g
    if violations:
        raise AssertionError('%s: %s' % (what, '\n'.join(violations)))
    assert_same_bits(runs, names, what)
    return Contract(guards, runs['plain'])
