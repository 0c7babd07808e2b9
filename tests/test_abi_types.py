"""The Python side of the boundary takes its types from include/atvsnet_hip.h (no GPU): `_lib.lib()` sets restype and argtypes
of every declared symbol from the header's own declarations, so a wrong arity or a float for an int raises before any launch,
and 64-bit values travel whole in both directions.  What the header says is read here from its text, not from `_lib`'s parse."""
import ctypes
import re

import pytest

from atvsnet_amd import _lib


@pytest.fixture(scope='module')
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope='module')
def header():
    """The header without comments and preprocessor lines."""
    with open(_lib.HEADER) as f:
        return re.sub(r'/\*.*?\*/|^\s*#.*?$', '', f.read(), flags=re.S | re.M)


def test_every_symbol_is_typed_with_the_headers_parameter_count(L, header):
    counts = {name: 0 if params.strip() == 'void' else params.count(',') + 1
              for name, params in re.findall(r'\b(atvs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', header)}
    assert sorted(counts) == _lib.declared_symbols() and len(counts) >= 155
    for name, n in counts.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
        assert fn.restype in (ctypes.c_int, ctypes.c_long, ctypes.c_char_p), name


def test_every_long_function_returns_c_long(L, header):
    longs = re.findall(r'\blong\s+(atvs_[a-z0-9_]+)\s*\(', header)
    assert len(longs) >= 15 and 'atvs_deconv_up_b_grid' in longs
    for name in longs:
        assert getattr(L, name).restype is ctypes.c_long, name
    ints = set(re.findall(r'\bint\s+(atvs_[a-z0-9_]+)\s*\(', header))
    assert ints and all(getattr(L, name).restype is ctypes.c_int for name in ints)
    assert L.atvs_target_arch.restype is ctypes.c_char_p and L.atvs_target_arch() == b'gfx950'


def test_plain_python_ints_travel_as_64_bits_both_ways(L):
    assert L.atvs_conv1x1_rows(2 ** 42) == 2 ** 34                        # 256 pixels a workgroup
    # 512 rows a block: 2^40 rows give exactly 2^31 blocks, the first count an int cannot hold (it reads -2^31 as one)
    assert L.atvs_channel_stats_num_blocks(2 ** 40) == 2 ** 31 > 2 ** 31 - 1
    assert L.atvs_channel_stats_num_blocks(2 ** 41) == 2 ** 32 > 2 ** 31
    assert L.atvs_deconv_up_b_grid.restype is ctypes.c_long


def test_wrong_arity_raises(L):
    n = None
    with pytest.raises(TypeError):
        L.atvs_refine_stems_f32(n, n, n, n, n, n, n, n, 1, 8, 8, 32, n)               # 13 of 14: y_planar is missing
    assert L.atvs_refine_stems_f32(n, n, n, n, n, n, n, n, 1, 8, 8, 32, 0, n) == -1   # ATVS_ERR_NULL


def test_a_float_for_an_int_parameter_raises(L):
    with pytest.raises(ctypes.ArgumentError):
        L.atvs_conv1x1_supported(1.5, 16)
    with pytest.raises(ctypes.ArgumentError):
        L.atvs_conv1x1_rows(64.0)


@pytest.mark.parametrize('text', ['int atvs_x(size_t n);', 'struct foo* atvs_y(void);', 'int atvs_z(unsigned int n);',
                                  'float atvs_w(int n);', 'int atvs_v(int (*f)(int));', 'int atvs_u(int n)\n{ return n; }'])
def test_the_parser_refuses_what_its_rules_do_not_cover(text):
    good = 'int atvs_a(const float* x, long n, atvs_stream_t stream);\n'
    with pytest.raises(RuntimeError, match=re.search(r'atvs_[a-z]', text).group(0)):
        _lib.prototypes(good + text)
    assert _lib.prototypes(good) == {'atvs_a': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p])}


def test_the_rules_on_a_small_header():
    text = ('/* int atvs_commented(int); */\n#define ATVS_X(a) a\ntypedef void* atvs_stream_t;\n'
            'const char* atvs_name(void);\nlong atvs_rows(long n, int c);\n'
            'int atvs_run(const float* const* xs, double* out, float eps, double tol,\n             atvs_stream_t stream);\n')
    assert _lib.prototypes(text) == {
        'atvs_name': (ctypes.c_char_p, []),
        'atvs_rows': (ctypes.c_long, [ctypes.c_long, ctypes.c_int]),
        'atvs_run': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_void_p])}
