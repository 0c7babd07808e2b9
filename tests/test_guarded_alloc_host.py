"""tests/guarded_alloc.py can fail: fake ops on CPU tensors that write one byte past an output, one byte before it, into the
round-up tail or into an input, that leave an element unwritten or accumulate into scratch they never cleared -- each is reported,
with its site, side and offset.  The stray writes go through ctypes at data_ptr() offsets that stay inside the helper's own buffer."""
import ctypes
import re

import pytest
import torch

import guarded_alloc as GA

CPU = torch.device('cpu')


def _poke(address, value=0xA5, count=1):
    ctypes.memset(address, value, count)


def _violations(g):
    with pytest.raises(AssertionError) as e:
        g.check()
    return str(e.value)


def _alloc_line(offset=1):
    import sys
    return sys._getframe(1).f_lineno + offset


@pytest.mark.parametrize('fill', (0x00, 0xFF, 0xA5))
def test_a_clean_op_passes_and_the_layout_is_as_stated(fill):
    with GA.guarded(CPU, fill) as g:
        out = torch.empty((5, 3), dtype=torch.float32, device='cpu')
        scratch = torch.empty(100, dtype=torch.uint8)
        z = torch.zeros(7, dtype=torch.int64, device=CPU)
        f = torch.full((3,), 2.5, device='cpu')
        like = torch.empty_like(out)
        zl = torch.zeros_like(out)
        for t in (out, scratch, z, f, like, zl):
            assert t.is_contiguous() and t.data_ptr() % 256 == 0
        assert out.dtype == torch.float32 and tuple(out.shape) == (5, 3) and like.shape == out.shape
        assert bool((scratch == fill).all()) and bool((out.view(torch.uint8) == fill).all()) and bool((like.view(torch.uint8) == fill).all())
        assert z.tolist() == [0] * 7 and f.tolist() == [2.5] * 3 and f.dtype == torch.float32 and not zl.any()
        out.copy_(torch.arange(15.0).reshape(5, 3))               # a well-behaved op: writes its payload, all of it
        scratch.fill_(fill ^ 0xFF)
        g.check()
        assert [a.kind for a in g.allocations] == ['empty', 'empty', 'zeros', 'full', 'empty_like', 'zeros_like']
        assert [a.nbytes for a in g.allocations] == [60, 100, 56, 12, 60, 60]
        assert all(a.site.endswith('test_guarded_alloc_host.py') for a in g.allocations)
        assert g.summary() == (6, 348)
    assert torch.empty is GA._ORIGINAL['empty']


def test_the_guards_do_not_depend_on_the_fill_and_are_not_constant():
    seen = []
    for fill in (0x00, 0xFF):
        with GA.guarded(CPU, fill) as g:
            torch.empty(10, dtype=torch.uint8)
            b = g._buffers[0]
            assert b.guard == GA.GUARD
            seen.append((b.raw[b.start - b.guard:b.start].clone(), b.raw[b.start + 10:b.start + 256 + b.guard].clone(), b.start % 256))
    if seen[0][2] == seen[1][2]:                                  # the same alignment shift: the same positions, the same bytes
        assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])
    for before, after, _ in seen:
        assert len(before.unique()) == 256 and len(after.unique()) == 256
        assert int((before == 0xFF).sum()) < len(before) // 64 and int((before == 0).sum()) < len(before) // 64


def test_the_guard_is_as_wide_as_a_large_allocation():
    with GA.guarded(CPU, 0) as g:
        torch.empty(100000, dtype=torch.float32)
        assert g._buffers[0].guard == 400128                       # 400000 rounded up to 256
        g.check()


def test_one_byte_past_the_end_is_named():
    with GA.guarded(CPU, 0xFF) as g:
        line = _alloc_line()
        out = torch.empty(64, dtype=torch.float32)                  # 256 bytes: no tail, the next byte is the guard
        _poke(out.data_ptr() + 256)
        text = _violations(g)
    assert '1 buffer violations' in text
    assert 'test_guarded_alloc_host.py:%d' % line in text and 'out = torch.empty(64' in text
    assert 'AFTER' in text and 'past the 256-byte round-up' in text and 'offsets 256 .. 256' in text
    assert '(64,)' in text and 'torch.float32' in text


def test_one_byte_before_the_start_is_named():
    with GA.guarded(CPU, 0x00) as g:
        line = _alloc_line()
        out = torch.empty((3, 3), dtype=torch.int32)
        _poke(out.data_ptr() - 1)
        text = _violations(g)
    assert 'test_guarded_alloc_host.py:%d' % line in text and 'BEFORE' in text and 'offsets -1 .. -1' in text and '(3, 3)' in text


def test_a_write_of_the_fill_value_outside_the_payload_is_seen():
    for fill in (0x00, 0xFF):
        with GA.guarded(CPU, fill) as g:
            out = torch.empty(256, dtype=torch.uint8)
            ctypes.memset(out.data_ptr() + 256, fill, 4)           # at most one of four neighbouring pattern bytes equals the fill
            text = _violations(g)
        assert 'AFTER' in text


def test_a_write_into_the_round_up_tail_is_named():
    with GA.guarded(CPU, 0xFF) as g:
        out = torch.empty(9, dtype=torch.float32)                   # 36 bytes, tail 36 .. 255
        _poke(out.data_ptr() + 36, count=4)                         # the tenth float of a kernel that rounds 9 up
        text = _violations(g)
    assert 'in the round-up tail' in text and 'offsets 36 .. 39' in text and '4 bytes AFTER' in text


def test_a_write_into_a_placed_input_is_named():
    with GA.guarded(CPU, 0x00) as g:
        x = g.place(torch.arange(12, dtype=torch.float32).reshape(4, 3))
        assert x.data_ptr() % 256 == 0 and x.tolist()[3] == [9.0, 10.0, 11.0]
        g.check()
        _poke(x.data_ptr() + 4 * 7, value=0x7F)
        text = _violations(g)
    assert 'placed INPUT changed' in text and '1 elements, first 7' in text and 'x = g.place(' in text


def test_an_input_whose_nan_payload_changes_is_named_and_a_writable_one_is_not():
    nan = torch.tensor([0x7FC00001, 0x7FC00002], dtype=torch.int32).view(torch.float32)
    with GA.guarded(CPU, 0x00) as g:
        x = g.place(nan)
        w = g.place(nan, writable=True)
        w.view(torch.int32)[1] = 0x7FC00003
        g.check()
        x.view(torch.int32)[1] = 0x7FC00003                         # still a NaN: only its bits say so
        assert 'placed INPUT changed' in _violations(g)


def test_every_violation_is_listed_in_one_error():
    with GA.guarded(CPU, 0x00) as g:
        a = torch.empty(64, dtype=torch.float32)
        b = torch.empty(10, dtype=torch.uint8)
        _poke(a.data_ptr() - 8, count=8)
        _poke(a.data_ptr() + 256 + 100)
        _poke(b.data_ptr() + 10)
        text = _violations(g)
    assert '3 buffer violations' in text and 'offsets -8 .. -1' in text and 'offsets 356 .. 356' in text and 'offsets 10 .. 10' in text


def test_a_zero_size_allocation_is_guarded_and_checked():
    with GA.guarded(CPU, 0xFF) as g:
        out = torch.empty((0, 3), dtype=torch.float32)
        like = torch.empty_like(out)
        assert tuple(out.shape) == (0, 3) and tuple(like.shape) == (0, 3) and [a.nbytes for a in g.allocations] == [0, 0]
        g.check()
        assert g.address(0) % 256 == 0
        _poke(g.address(0))                                         # a kernel that writes row 0 of an output without rows
        text = _violations(g)
    assert 'AFTER' in text and 'offsets 0 .. 0' in text and '(0, 3)' in text and '1 buffer violations' in text


def test_torch_is_restored_after_an_exception():
    with pytest.raises(ZeroDivisionError):
        with GA.guarded(CPU, 0x00):
            assert torch.empty is not GA._ORIGINAL['empty']
            1 / 0
    for name in GA._PATCHED:
        assert getattr(torch, name) is GA._ORIGINAL[name]
    with pytest.raises(RuntimeError, match='nest'):
        with GA.guarded(CPU, 0x00):
            with GA.guarded(CPU, 0xFF):
                pass
    for name in GA._PATCHED:
        assert getattr(torch, name) is GA._ORIGINAL[name]


def test_a_tensor_for_another_device_is_not_guarded():
    with GA.guarded(CPU, 0xFF) as g:
        m = torch.empty((4, 4), device='meta')
        ml = torch.empty_like(m)
        mz = torch.zeros(3, device='meta')
        assert m.device.type == 'meta' and ml.device.type == 'meta' and mz.device.type == 'meta'
        assert g.allocations == []
        c = torch.empty(4)
        assert len(g.allocations) == 1 and c.device.type == 'cpu'
    with GA.guarded(torch.device('meta'), 0xFF) as g:                # ... and a CPU tensor is not, when the guard is elsewhere
        c = torch.empty(4, device='cpu')
        assert g.allocations == [] and c.device.type == 'cpu'


# ------------------------------------------------------------------------------------------------ the cross-fill comparison
def _square(d, place):
    out = torch.empty_like(d['x'])
    out.copy_(d['x'] * d['x'])
    return out


def _skips_row_two(d, place):
    out = torch.empty_like(d['x'])
    for r in range(len(out)):
        if r == 2:
            continue                                                 # an early `continue`: the row keeps what the allocator gave
        out[r] = d['x'][r] * d['x'][r]
    return out


def _dirty_scratch(d, place):
    scratch = torch.empty(4, dtype=torch.int64)                      # never cleared: the op accumulates into what it was given
    scratch += d['x'].to(torch.int64).sum(0)
    out = torch.empty(4, dtype=torch.int64)
    out.copy_(scratch)
    return out


def _overruns(d, place):
    out = torch.empty_like(d['x'])
    out.copy_(d['x'])
    _poke(out.data_ptr() + out.numel() * 4)
    return out


def _writes_its_input(d, place):
    d['x'][0, 0] = 7.0
    return _square(d, place)


X = {'x': torch.arange(20, dtype=torch.float32).reshape(5, 4)}


def test_the_three_runs_pass_a_clean_op():
    done = GA.run_contract(_square, X, lambda r: [r], CPU, names=('out',))
    assert sorted(done.guards) == [0x00, 0xFF] and torch.equal(done.selected[0], X['x'] * X['x'])
    for g in done.guards.values():
        assert [a.kind for a in g.allocations] == ['input', 'empty_like']
        assert '_square' in g.allocations[1].code and g.allocations[1].nbytes == 80


def test_an_unwritten_output_element_is_caught():
    with pytest.raises(AssertionError, match=r'(?s)the runs differ.*out differs from plain in 4 of 20 elements, first at flat index 8'):
        GA.run_contract(_skips_row_two, X, lambda r: [r], CPU, names=('out',), what='skips')


def test_scratch_that_is_accumulated_into_without_a_clear_is_caught():
    with pytest.raises(AssertionError, match=r'(?s)the runs differ.*out differs'):
        GA.run_contract(_dirty_scratch, X, lambda r: [r], CPU, names=('out',))


def test_the_three_runs_report_an_overrun_and_a_written_input():
    with pytest.raises(AssertionError) as e:
        GA.run_contract(_overruns, X, lambda r: [r], CPU, names=('out',), what='overruns')
    assert re.search(r'overruns: fill 0x00: 1 buffer violations', str(e.value)) and 'fill 0xFF' in str(e.value)
    assert 'offsets 80 .. 80' in str(e.value) and 'in the round-up tail' in str(e.value)
    with pytest.raises(AssertionError, match='placed INPUT changed'):
        GA.run_contract(_writes_its_input, X, lambda r: [r], CPU)
    GA.run_contract(_writes_its_input, X, lambda r: [r], CPU, writable=('x',))
    assert X['x'][0, 0] == 0.0                                       # the caller's tensors are never the ones an op sees


def test_nan_bits_and_the_sign_of_zero_count_in_the_comparison():
    a = torch.tensor([0x7FC00000, 0], dtype=torch.int32).view(torch.float32)
    b = torch.tensor([0x7FC00001, 0], dtype=torch.int32).view(torch.float32)
    c = torch.tensor([0x7FC00000, -0x80000000], dtype=torch.int32).view(torch.float32)
    GA.assert_same_bits({'p': [a, None], 'q': [a.clone(), None]}, ('t', 'u'))
    for other in (b, c):
        with pytest.raises(AssertionError, match='t differs'):
            GA.assert_same_bits({'p': [a], 'q': [other]}, ('t',))
    with pytest.raises(AssertionError, match='None in one run only'):
        GA.assert_same_bits({'p': [a], 'q': [None]}, ('t',))
    with pytest.raises(AssertionError, match='is torch.float32 \\(3,\\)'):
        GA.assert_same_bits({'p': [a], 'q': [torch.zeros(3)]}, ('t',))


def test_the_recording_proxy_notes_entry_points_and_restores_the_module():
    class Lib(object):
        def atvs_one(self, x):
            return x + 1

        def atvs_two(self):
            return 0

    class Module(object):
        pass
    module = Module()
    the_lib = Lib()
    module.lib = original = lambda: the_lib
    with pytest.raises(KeyError):
        with GA.recording_lib(module) as calls:
            assert module.lib().atvs_one(4) == 5 and module.lib().atvs_two() == 0 and module.lib().atvs_one(1) == 2
            with pytest.raises(AttributeError):
                module.lib().atvs_missing
            assert calls == ['atvs_one', 'atvs_two', 'atvs_one']
            raise KeyError('x')
    assert module.lib is original


# ------------------------------------------------------------------------------------------------------------- slice masks
def _pattern_rows(rows=6, ld=8):
    return (torch.arange(rows * ld, dtype=torch.float32) * 1.25 + 0.5).reshape(rows, ld)


def _writes_slice(lo, hi, stray=None):
    """A fake op that writes out[:, lo:hi] = 2 x, and then what `stray` does to the buffer."""
    def op(d, place):
        d['out'][:, lo:hi] = 2.0 * d['x']
        if stray is not None:
            stray(d['out'])
        return d['out']
    return op


SLICE = {'x': torch.arange(18, dtype=torch.float32).reshape(6, 3) + 100.0, 'out': _pattern_rows()}


def test_a_channel_slice_may_be_written_and_nothing_else():
    done = GA.run_contract(_writes_slice(2, 5), SLICE, lambda r: [r], CPU, names=('out',), writable={'out': (2, 5)})
    assert torch.equal(done.selected[0][:, 2:5], 2.0 * SLICE['x']) and torch.equal(done.selected[0][:, :2], SLICE['out'][:, :2])
    mask = torch.zeros(6, 8, dtype=torch.bool)
    mask[:, 2:5] = True
    GA.run_contract(_writes_slice(2, 5), SLICE, lambda r: [r], CPU, writable={'out': mask})
    with pytest.raises(AssertionError, match='placed INPUT changed'):                          # not writable at all
        GA.run_contract(_writes_slice(2, 5), SLICE, lambda r: [r], CPU)
    with pytest.raises(ValueError, match='writable range'):
        GA.run_contract(_writes_slice(2, 5), SLICE, lambda r: [r], CPU, writable={'out': (2, 9)})
    with pytest.raises(ValueError, match='bool tensor'):
        GA.run_contract(_writes_slice(2, 5), SLICE, lambda r: [r], CPU, writable={'out': mask[:3]})


def test_one_float_beyond_the_channel_range_is_named_with_its_flat_index():
    def beyond(out):
        out[3, 5] = -1.0                                             # channel 5 of row 3: flat index 29
    with pytest.raises(AssertionError, match=r'elements OUTSIDE the writable slice changed, 1 elements, first 29') as e:
        GA.run_contract(_writes_slice(2, 5, beyond), SLICE, lambda r: [r], CPU, writable={'out': (2, 5)}, what='beyond')
    assert 'fill 0x00' in str(e.value) and 'fill 0xFF' in str(e.value) and str(e.value).count('buffer violations') == 2


def test_the_last_channel_of_the_previous_pixel_is_named():
    def previous(out):
        out[4, 7] = out[4, 7] + 1.0                                  # an offset one too small at c_off = 0 of the next row
    with pytest.raises(AssertionError, match=r'OUTSIDE the writable slice changed, 1 elements, first 39'):
        GA.run_contract(_writes_slice(0, 3, previous), SLICE, lambda r: [r], CPU, writable={'out': (0, 3)})


def test_a_neighbour_copied_over_a_neighbour_is_seen_because_the_buffer_is_no_constant():
    def smear(out):
        out[:, 5] = out[:, 6]                                        # the kernel stores the value next door
    with pytest.raises(AssertionError, match='OUTSIDE the writable slice changed, 6 elements, first 5'):
        GA.run_contract(_writes_slice(2, 5, smear), SLICE, lambda r: [r], CPU, writable={'out': (2, 5)})
    constant = dict(SLICE, out=torch.full((6, 8), 3.0))
    GA.run_contract(_writes_slice(2, 5, smear), constant, lambda r: [r], CPU, writable={'out': (2, 5)})     # ... which a constant buffer hides


def test_a_masked_violation_is_listed_with_the_guards_in_one_error():
    with GA.guarded(CPU, 0x00) as g:
        out = g.place(_pattern_rows(), writable=(0, 4))
        out[:, :4] = 0.0
        g.check()
        out[1, 4] = 9.0
        _poke(out.data_ptr() + out.numel() * 4)
        text = _violations(g)
    assert '2 buffer violations' in text and 'AFTER' in text and 'OUTSIDE the writable slice changed, 1 elements, first 12' in text


# --------------------------------------------------------------------------------------------- arranged weights under the guard
def _fake_packer(ops, key, values):
    """What ops/packing.py does: pack on the host, upload, cache -- with "one zero element behind the last" as the packers end."""
    pk = ops._pack_cache.get(key)
    if pk is None:
        whole = torch.cat([values, torch.zeros(1)])
        pk = ops._Packed(key=key)
        pk.wp = whole[:len(values)]
        ops._pack_cache[key] = pk
    return pk


def _conv_like(read_ahead, store=False):
    def op(d, place):
        from atvsnet_amd import ops
        pk = _fake_packer(ops, 'fake', torch.arange(1.0, 5.0))
        n = pk.wp.numel() + (1 if read_ahead else 0)
        w = torch.tensor((ctypes.c_float * n).from_address(pk.wp.data_ptr())[:])        # the kernel's own walk over the buffer
        if store:
            pk.wp[0] = 7.0
        out = torch.empty(1)
        out[0] = float((w * w).sum()) + float(d['x'].sum())
        return out
    return op


def _weights(place):
    from atvsnet_amd import ops
    return GA.weights_under(place, ops)


def test_arranged_weights_are_placed_and_a_read_ahead_beyond_them_is_caught():
    from atvsnet_amd import ops
    done = GA.run_contract(_conv_like(False), X, lambda r: [r], CPU, names=('out',), around=_weights)
    assert float(done.selected[0]) == 30.0 + float(X['x'].sum())
    for g in done.guards.values():
        placed = [a for a in g.allocations if a.kind == 'input' and '_fake_packer' in a.code]
        assert len(placed) == 1 and placed[0].nbytes == 16 and 'pk.wp = ' in placed[0].code
    assert not ops._pack_cache and '__setattr__' not in vars(ops._Packed)
    # the zero behind the last weight is not part of the buffer the launch is given: under the guard the next bytes are the pattern
    with pytest.raises(AssertionError, match=r'(?s)the runs differ.*out differs from plain'):
        GA.run_contract(_conv_like(True), X, lambda r: [r], CPU, names=('out',), around=_weights)
    GA.run_contract(_conv_like(True), X, lambda r: [r], CPU, names=('out',))                  # without the placement nothing is seen
    ops.clear_pack_cache()
    with pytest.raises(AssertionError, match='placed INPUT changed, 1 elements, first 0'):     # a kernel that stores into its weights
        GA.run_contract(_conv_like(False, store=True), X, lambda r: [r], CPU, around=_weights)
    assert not ops._pack_cache and '__setattr__' not in vars(ops._Packed)


def test_each_run_starts_from_empty_caches_and_no_guarded_payload_stays_in_them():
    from atvsnet_amd import ops
    ops._pack_cache['stale'] = ops._Packed(key='stale')
    ops._fold_cache['stale'] = ops._xp_cache['stale'] = ops._virt_cache['stale'] = 1
    with GA.guarded(CPU, 0xFF) as g:
        with GA.weights_under(g.place, ops, split16=False):
            assert not (ops._pack_cache or ops._fold_cache or ops._xp_cache or ops._virt_cache) and not ops.cfg.split16
            pk = _fake_packer(ops, 'k', torch.arange(3.0))
            assert g.owns(pk.wp) and pk.wp.tolist() == [0.0, 1.0, 2.0] and ops._pack_cache['k'] is pk
            pk.ntaps = 27                                            # any other field is stored as it is
            kept = pk
        assert not ops._pack_cache and ops.cfg.split16 == ops.Config._DEFAULTS['split16']
        assert g.owns(kept.wp)                                       # only a reference the caller kept still points into the block
        g.check()
    with pytest.raises(AttributeError):
        with GA.weights_under(None, ops, no_such_switch=True):
            pass
    assert '__setattr__' not in vars(ops._Packed)


# ------------------------------------------------------------------------------------------------------ pooled device words
def test_a_pooled_buffer_made_inside_a_guarded_block_is_reported_and_a_warmed_one_is_not():
    pool = {}

    def flag():
        if 'flag' not in pool:
            pool['flag'] = torch.zeros(1, dtype=torch.int32)
        return pool['flag']

    def op(d, place):
        out = torch.empty_like(d['x'])
        out.copy_(d['x'] + float(flag()))
        return out
    with pytest.raises(AssertionError, match=r'pooled buffers made inside the guarded block, which outlive it: flag'):
        # (the plain run makes the flag first, so drop it: the first guarded run is the one that makes it)
        GA.run_contract(lambda d, place: (pool.clear() if place is not GA._identity else None, op(d, place))[1], X, lambda r: [r], CPU,
                        pools=lambda: list(pool.items()), what='pool')
    pool.clear()
    GA.run_contract(op, X, lambda r: [r], CPU, warm=flag, pools=lambda: list(pool.items()))
    assert pool['flag'].tolist() == [0]
    with GA.guarded(CPU, 0xFF) as g:
        inside, outside = torch.empty(3), GA._ORIGINAL['empty'](3)
        assert g.owns(inside) and g.owns(inside[1:]) and not g.owns(outside)
