"""tests/network_contract_rows.py is complete and its builders do what they state, without a GPU: every entry point that
include/atvsnet_hip.h declares and that writes through a non-const pointer is named by a row of one of the two tables (this one and
tests/buffer_contract_rows.py) or is a host packer; every ops function of the network side has a row; every row names a size that
reaches each of its entry points; every exclusion of a selection quotes the header; every builder is deterministic with the stated
shapes; every case runs its wrapper's host code on `meta` tensors (the dispatch asserted against ops.conv_plan, the packers run);
and every host packer writes exactly the bytes it reports, between two guards, over 0x00 and over 0xFF."""
import inspect
import re

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import _lib, ops

import buffer_contract_rows as BR
import guarded_alloc as GA
import network_contract_rows as NR
from test_buffer_contract_host import _declarations, _writes

QUERIES = ('_size', '_supported', '_grid', '_rows', '_num_blocks')
PACKERS = ('atvs_conv_pack', 'atvs_conv_tiled_pack', 'atvs_conv_xw_pack', 'atvs_conv_xw_pack_sibling', 'atvs_conv_xb_pack', 'atvs_conv_xb_pack_sibling',
           'atvs_conv2d_lds_pack', 'atvs_conv2d_b_pack', 'atvs_conv1x1_pack', 'atvs_conv1x1_b_pack', 'atvs_conv3d_b_pack', 'atvs_conv3d_s2b_pack',
           'atvs_deconv_up_pack', 'atvs_deconv_up_b_pack', 'atvs_refine_stems_pack', 'atvs_aanet_b_pack', 'atvs_conv_c16_pack', 'atvs_conv_c16b_pack')
CASES = NR.cases()
IDS = ['%s[%s]' % c for c in CASES]


def _named(rows):
    named = set()
    for row in rows.values():
        named.update(row.entries)
        for p in row.sizes.values():
            named.update(p.get('entries', ()))
    return named


def test_every_entry_point_that_writes_is_in_a_row_of_one_of_the_two_tables_or_is_a_packer():
    named = _named(NR.ROWS) | _named(BR.ROWS)
    writers = [n for n, params in _declarations() if _writes(params) and not n.endswith(QUERIES)]
    assert len(writers) > 120 and 'atvs_abi_version' not in writers
    uncovered = [n for n in writers if n not in named and n not in PACKERS]
    assert not uncovered, 'no row of tests/network_contract_rows.py or tests/buffer_contract_rows.py names %s' % uncovered
    assert BR.EXCLUDED_ENTRY_POINTS == {}
    assert all(n in writers for n in PACKERS)
    assert 'atvs_conv3d_b_f32' in _named(NR.ROWS) and 'atvs_deconv_up_f32' in _named(NR.ROWS) and 'atvs_conv_c16b_sum_f32' in _named(NR.ROWS)


def test_every_name_a_row_uses_is_declared():
    declared = set(_lib.prototypes())
    assert _named(NR.ROWS) <= declared, sorted(_named(NR.ROWS) - declared)


def test_every_ops_function_of_the_network_side_has_a_row():
    from atvsnet_amd.ops import aanet, convolution, geometry, norm
    wanted = []
    for module in (geometry, norm, convolution):
        wanted += [n for n, f in vars(module).items() if inspect.isfunction(f) and f.__module__ == module.__name__ and not n.startswith('_')]
    wanted += ['aanet_combine', 'aanet_partial', 'divide', 'aanet_fused', 'conv2d_lds', 'conv1x1', 'bottleneck', 'conv2d_tail']
    assert all(hasattr(aanet, n) for n in wanted[-8:-4]) and len(wanted) >= 45
    # predicates and the flag's accessors launch nothing and write no buffer
    no_buffer = {'nonfinite_flag', 'nonfinite_seen', 'siblings_prologue_ok', 'siblings_ok', 'deconv_sum_ok', 'photo_pieces_ok', 'planar_concat_ok'}
    assert no_buffer <= set(wanted)
    missing = [n for n in wanted if n not in NR.ROWS and n not in no_buffer]
    assert not missing, missing
    assert len(set(n for n in wanted if n in NR.ROWS and getattr(geometry, n, None) is not None)) == 17      # every public function of ops/geometry.py


def test_every_row_names_a_size_that_reaches_each_entry_point():
    for row in NR.ROWS.values():
        somewhere = set()
        for size, p in row.sizes.items():
            assert p['entries'] and row.required(size) == tuple(p['entries']), (row.name, size)
            somewhere.update(row.required(size))
        assert set(row.entries) <= somewhere, (row.name, sorted(set(row.entries) - somewhere))


def test_every_family_conv_plan_can_return_is_a_size_of_the_conv_row():
    import ast
    with open(inspect.getsourcefile(ops.conv_plan)) as f:
        source = f.read()
    families = set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Call) and getattr(node.func, 'id', '') == 'plan' and node.args:
            families.update(c.value for c in ast.walk(node.args[0]) if isinstance(c, ast.Constant) and isinstance(c.value, str))
    assert len(families) >= 15, families
    seen = set(NR.PLAN_FAMILY.get(p['family'], p['family']) for p in NR.ROWS['conv'].sizes.values())
    assert families <= seen, sorted(families - seen)
    kernels = set(p['family'] for p in NR.ROWS['conv'].sizes.values())
    assert {'conv2d_lds', 'conv2d_b', 'conv1x1', 'conv1x1_b', 'xp/xb', 'xp/xw'} <= kernels
    assert {4, 8} <= set(p['tile_y'] for p in NR.ROWS['conv'].sizes.values())


def test_every_exclusion_of_a_selection_quotes_a_header_line_that_says_so():
    with open(_lib.HEADER) as f:
        lines = f.read().split('\n')
    quoted = 0
    for row in NR.ROWS.values():
        for text in row.excluded:
            m = re.search(r'"([^"]+)".*?header line (\d+)', text, flags=re.S)
            assert m is not None, (row.name, text)
            quote, line = ' '.join(m.group(1).replace('...', '\0').split()), int(m.group(2))
            near = ' '.join(' '.join(l.strip().lstrip('*').strip() for l in lines[line - 2:line + 2]).split())
            for part in quote.split('\0'):
                assert part.strip().strip(',') in near, '%s: header line %d does not say %r' % (row.name, line, part)
            quoted += 1
    assert quoted >= 8


def test_no_tensor_above_2_to_the_20_elements_and_every_slice_lies_in_a_placed_buffer():
    for name, size in CASES:
        row = NR.ROWS[name]
        p = row.sizes[size]
        d = row.build(p)
        for k, v in d.items():
            if isinstance(v, torch.Tensor):
                assert v.numel() <= 2 ** 20, (name, size, k, tuple(v.shape))
                assert bool(torch.isfinite(v).all()) and float(v.abs().max() if v.numel() else 0) < 60000.0, (name, size, k)
        for k, spec in row.slices(p).items():
            assert isinstance(d.get(k), torch.Tensor), (name, size, k)
            mask = GA.writable_mask(spec, tuple(d[k].shape))
            assert bool(mask.any()), (name, size, k)
            # a buffer of which a part is held carries a position-dependent pattern: no value twice in a row
            flat = d[k].reshape(-1)
            assert flat.numel() < 2 or float((flat[1:] == flat[:-1]).float().mean()) < 0.01, (name, size, k)


@pytest.mark.parametrize('name,size', CASES, ids=IDS)
def test_builder(name, size):
    row = NR.ROWS[name]
    p = row.sizes[size]
    d, again = row.build(p), row.build(p)
    stated = row.shapes(p)
    tensors = {k: v for k, v in d.items() if isinstance(v, torch.Tensor)}
    assert sorted(tensors) == sorted(stated), (sorted(tensors), sorted(stated))
    for k, (shape, dtype) in stated.items():
        t = tensors[k]
        assert t.device.type == 'cpu' and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape), (k, t.dtype, tuple(t.shape), shape)
        assert torch.equal(t.view(torch.uint8) if t.numel() else t, again[k].view(torch.uint8) if t.numel() else again[k]), '%s is not deterministic' % k
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == np.float32 and np.array_equal(v, again[k]), k
        elif not isinstance(v, torch.Tensor):
            assert again[k] == v, k
    assert set(row.writable) <= set(tensors) and set(row.slices(p)) <= set(tensors)
    assert row.names and row.constants and isinstance(p['cfg'], dict)


# ------------------------------------------------------------------------------------------ host code and host packers under a guard
PAD = 4096


class _HostGuard(object):
    """numpy.empty handing out the middle of a pattern-filled buffer, and a proxy in front of the library that runs every host
    packer twice -- over a payload of 0x00 and of 0xFF -- and holds it to the buffer: both sides intact, the same bytes twice."""

    def __init__(self):
        self.buffers = {}                 # payload address -> (raw uint8 buffer, payload bytes)
        self.packed = []                  # (entry point, payload bytes)
        self._empty = np.empty

    def pattern(self, n):
        i = np.arange(n, dtype=np.int64)
        return ((i * 167 + (i >> 8) * 13 + 0x5A) & 0xFF).astype(np.uint8)

    def empty(self, shape, dtype=float, order='C', **kw):
        dt = np.dtype(dtype)
        count = int(np.prod(shape))
        n = count * dt.itemsize
        raw = self._empty(n + 2 * PAD + 64, np.uint8)
        start = PAD + (-raw.ctypes.data) % 64
        raw[:] = self.pattern(len(raw))
        out = raw[start:start + n].view(dt).reshape(shape)
        self.buffers[out.ctypes.data] = (raw, start, n)
        return out

    def check(self, name, raw, start, n):
        want = self.pattern(len(raw))
        before, after = np.nonzero(raw[:start] != want[:start])[0], np.nonzero(raw[start + n:] != want[start + n:])[0]
        assert not len(before), '%s wrote %d bytes BEFORE its %d-byte output, first at %d' % (name, len(before), n, before[0] - start)
        assert not len(after), '%s wrote %d bytes AFTER its %d-byte output, first at %d' % (name, len(after), n, after[0] + n)

    def lib(self, real):
        guard = self

        class Proxy(object):
            def __getattr__(self, name):
                fn = getattr(real, name)
                if name not in PACKERS:
                    return fn

                def held(*args):
                    outs = [guard.buffers[a] for a in args if isinstance(a, int) and a in guard.buffers]
                    assert outs, '%s was given no output made by numpy.empty' % name
                    seen = []
                    for fill in (0x00, 0xFF):
                        for raw, start, n in outs:
                            raw[start:start + n] = fill
                        rc = fn(*args)
                        assert rc == 0, (name, rc)
                        for raw, start, n in outs:
                            guard.check(name, raw, start, n)
                        seen.append([raw[start:start + n].copy() for raw, start, n in outs])
                    for a, b, (raw, start, n) in zip(seen[0], seen[1], outs):
                        ne = np.nonzero(a != b)[0]
                        assert not len(ne), '%s left %d of the %d bytes it reported unwritten, first at %d' % (name, len(ne), n, ne[0])
                        guard.packed.append((name, n))
                    return 0
                return held
        return Proxy()


@pytest.fixture(scope='module')
def host_guard():
    guard = _HostGuard()
    real = _lib.lib
    np.empty = guard.empty
    _lib.lib = lambda: guard.lib(real())
    try:
        yield guard
    finally:
        np.empty, _lib.lib = guard._empty, real


def _on_meta(d):
    return {k: v.to('meta') if isinstance(v, torch.Tensor) else v for k, v in d.items()}


def _host_half(host_guard, name, size):
    row = NR.ROWS[name]
    p = row.sizes[size]
    host_guard.buffers.clear()
    with GA.weights_under(None, ops, **p['cfg']):
        result = row.select(row.run(ops, _on_meta(row.build(p)), lambda t, **kw: t))
    assert 0 < len(result) <= len(row.names)
    assert all(t is None or t.device.type == 'meta' for t in result)


@pytest.mark.parametrize('name,size', CASES, ids=IDS)
def test_host_code_of_the_case_on_meta_tensors_with_every_packer_under_a_host_guard(host_guard, name, size):
    """The wrapper's host half at this size: its shape checks, the dispatch (the rows assert ops.conv_plan's answer), and the host
    packers of its weights, which write into numpy buffers that carry the pattern on both sides."""
    _host_half(host_guard, name, size)


def test_every_host_packer_runs_under_the_host_guard(host_guard):
    """Each of the 18 packers is called by some row, with every channel pair the rows use, and writes what it reported."""
    del host_guard.packed[:]
    for name, size in CASES:
        if any(isinstance(v, np.ndarray) for v in NR.ROWS[name].build(NR.ROWS[name].sizes[size]).values()):
            _host_half(host_guard, name, size)
    seen = set(n for n, _ in host_guard.packed)
    assert seen == set(PACKERS), (sorted(set(PACKERS) - seen), sorted(seen - set(PACKERS)))
    assert all(n > 0 for _, n in host_guard.packed) and len(host_guard.packed) > 150


def test_the_host_guard_can_fail():
    guard = _HostGuard()
    out = guard.empty(10, np.float32)
    raw, start, n = guard.buffers[out.ctypes.data]
    assert n == 40 and out.ctypes.data % 64 == 0
    guard.check('clean', raw, start, n)
    raw[start + n] ^= 0xFF
    with pytest.raises(AssertionError, match='AFTER its 40-byte output, first at 40'):
        guard.check('overruns', raw, start, n)
    raw[start + n] ^= 0xFF
    raw[start - 1] ^= 0xFF
    with pytest.raises(AssertionError, match='BEFORE its 40-byte output, first at -1'):
        guard.check('underruns', raw, start, n)
    raw[start - 1] ^= 0xFF

    class Lib(object):
        def atvs_conv_c16b_pack(self, w, cin, packed):          # a packer that leaves its last byte unwritten
            import ctypes
            ctypes.memset(packed, 0x11, 39)
            return 0
    with pytest.raises(AssertionError, match='left 1 of the 40 bytes it reported unwritten, first at 39'):
        guard.lib(Lib()).atvs_conv_c16b_pack(0, 8, out.ctypes.data)
