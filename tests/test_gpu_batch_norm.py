"""-m gpu: the batch-norm family of csrc/norm.hip held to float64 and to exact bits where the channel means are large.

a. atvs_bn_finalize on hand-built ops.Stats whose float64 partials are integers: every sum is exact in any order, so the
   parameters follow from the kernel's stated sequence in IEEE double (mean = S1/n, var = max(S2/n - mean*mean, 0),
   rstd = 1/sqrt(var + (double)(float)eps); the library is built with -ffp-contract=off, nothing in it is fused): mean and beta
   bit for bit, rstd within one float32 ulp; and the sticky non-finite flag.
b. atvs_channel_stats row by row: each workgroup's (sum, sum of squares) against the float64 sums of the 512 rows it owns, bit
   for bit on integers, within 32u sum|x| / 33u sum x^2 otherwise (an fp32 chain of at most 32 terms, one rounding of v*v).
c. atvs_bn_apply / atvs_bn_add / atvs_bn_add_plus per element against tests/bn_ref.py: 2u * bn_cond, 4u * sum of conds.

Every launch runs under numerics.poison_allocator with NaN-bordered inputs."""
import numpy as np
import pytest
import torch

import bn_ref as B
import numerics as N

pytestmark = pytest.mark.gpu

_WORST = {}


def _note(kernel, regime, r):
    _WORST[(kernel, regime)] = max(_WORST.get((kernel, regime), 0.0), r)


@pytest.fixture(scope='module', autouse=True)
def _report():
    """After the tests: the largest err / cond per kernel and regime, in units of u = 2^-24 (DESIGN.md 8 quotes these)."""
    yield
    for kernel in sorted({k[0] for k in _WORST}):
        print('\n%-14s ' % kernel + '  '.join('%s %.3f u' % (reg, _WORST[(kernel, reg)] / B.U) for reg in B.REGIMES
                                              if (kernel, reg) in _WORST))


def _dev(t, dev):
    return N.nan_bordered(t.to(dev))


# ------------------------------------------------------------------------------------------------------- a. atvs_bn_finalize

KINDS = ('mean_0', 'mean_1e2_std', 'mean_1e4_std', 'constant', 'inconsistent', 'generic')


def _totals(kind, n, rng):
    """Integer (S1, S2) of one channel of one sample over n values, of the kind."""
    r1 = int(rng.integers(1, n)) if n > 1 else 0          # a remainder: S1 / n is not an integer
    if kind == 'mean_0':
        return 0, 4 * n + int(rng.integers(0, n))
    if kind in ('mean_1e2_std', 'mean_1e4_std'):
        # std ~ 2, mean = m + r1/n with m = +-2e2 / +-2e4: S2 = n (4 + m^2) + 2 m r1 + r1 gives var = 4 + r1/n - (r1/n)^2 > 0
        m = (200 if kind == 'mean_1e2_std' else 20000) * (1 if rng.integers(0, 2) else -1)
        return n * m + r1, n * (4 + m * m) + 2 * m * r1 + r1
    k = int(rng.integers(3, 40))
    if kind == 'constant':                                 # every value k: var is exactly 0
        return n * k, n * k * k
    if kind == 'inconsistent':                             # S2/n = k^2 - 1 < mean^2: the clamp
        return n * k, n * (k * k - 1)
    s1 = int(rng.integers(-50 * n, 50 * n + 1))
    return s1, s1 * s1 // n + 1 + int(rng.integers(0, 100 * n))


def _spread(total, cells, rng, signed):
    """`cells` different integers that add up to total exactly (non-negative unless signed)."""
    q, r = divmod(total, cells)
    base = np.full(cells, q, dtype=np.int64)
    base[:r] += 1
    amp = 1000 if signed else int(min(1000, max(q, 0) // 2))
    d = rng.integers(0, amp + 1, size=cells)
    out = base + d - np.roll(d, 1)
    assert int(out.sum()) == total
    return out


def _hand_stats(dev, G, blocks, C, fold, pad, n, seed, poison=None):
    """(ops.Stats on the device, S1 (G,C), S2 (G,C), kinds) with integer partials; the padding columns hold NaN.
    poison = (g, c, value): one partial cell of that sample and channel is replaced by value."""
    from atvsnet_amd import ops
    rng = np.random.default_rng(seed)
    cpad = C * fold + pad
    part = np.full((G, blocks, 2, cpad), np.nan)
    S = np.zeros((2, G, C), dtype=np.int64)
    kinds = [[KINDS[(c + g + seed) % len(KINDS)] for c in range(C)] for g in range(G)]
    for g in range(G):
        for c in range(C):
            s1, s2 = _totals(kinds[g][c], n, rng)
            S[0, g, c], S[1, g, c] = s1, s2
            for k, tot in ((0, s1), (1, s2)):
                cells = _spread(tot, blocks * fold, rng, signed=(k == 0)).reshape(blocks, fold)
                part[g, :, k, c:C * fold:C] = cells            # columns c, c + C, ...: the same channel
    assert float(np.abs(part[np.isfinite(part)]).max()) * blocks * fold < 2.0 ** 53
    if poison is not None:
        g, c, value = poison
        part[g, blocks // 2, int(rng.integers(0, 2)), c + (fold - 1) * C] = value
    st = ops.Stats()
    st.partial = _dev(torch.from_numpy(part), dev)
    st.blocks, st.cpad, st.count, st.groups, st.fold = blocks, cpad, n, G, fold
    return st, S[0], S[1], kinds


def _want_params(S1, S2, n, eps):
    """The kernel's stated sequence in IEEE double (numpy float64, nothing fused)."""
    mean = S1.astype(np.float64) / np.float64(n)
    var = np.maximum(S2.astype(np.float64) / np.float64(n) - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    return mean, var, rstd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _finalize(st, C, dev, beta, eps):
    from atvsnet_amd import ops
    N.poison_allocator(dev)
    par = ops.bn_params(st, C, torch.empty(1, device=dev), beta, eps)
    torch.cuda.synchronize()
    G = st.groups
    assert tuple(par.shape) == ((3, C) if G == 1 else (G, 3, C))
    return par.cpu().numpy().reshape(G, 3, C)


@pytest.mark.parametrize('fold', [1, 2, 8])
@pytest.mark.parametrize('blocks', [1, 255, 256, 257, 1000])
def test_bn_finalize_known_answers(cuda, blocks, fold):
    from atvsnet_amd import ops
    ops.nonfinite_seen(cuda)
    i = 0
    for C in (1, 3, 8, 128):
        for G in (1, 3):
            for pad in (0, 5):
                i += 1
                eps = (1e-3, 1e-5)[i % 2]
                beta = None if (i // 2) % 2 else torch.randn(C, generator=torch.Generator().manual_seed(i))
                n = 8 * blocks * fold + 3
                what = 'blocks %d fold %d C %d G %d pad %d eps %g' % (blocks, fold, C, G, pad, eps)
                st, S1, S2, kinds = _hand_stats(cuda, G, blocks, C, fold, pad, n, seed=i)
                got = _finalize(st, C, cuda, None if beta is None else _dev(beta, cuda), eps)
                assert not ops.nonfinite_seen(cuda), '%s: the flag is up on finite partials' % what
                mean, var, rstd = _want_params(S1, S2, n, eps)
                assert np.array_equal(_bits(got[:, 0]), _bits(mean)), '%s: mean' % what
                wb = np.zeros((G, C), np.float32) if beta is None else np.broadcast_to(beta.numpy(), (G, C))
                assert np.array_equal(_bits(got[:, 2]), _bits(wb)), '%s: beta' % what
                ulps = np.abs(_bits(got[:, 1]).astype(np.int64) - _bits(rstd).astype(np.int64))
                assert int(ulps.max()) <= 1, '%s: rstd %d ulp off at %s' % (what, ulps.max(), np.argwhere(ulps > 1)[:1])
                # a constant channel and the clamp: var is exactly 0, rstd = fl(1 / sqrt(eps))
                flat = np.array(kinds)
                zero = (flat == 'constant') | (flat == 'inconsistent')
                assert bool((var[zero] == 0).all())
                r0 = np.float32(1.0 / np.sqrt(np.float64(np.float32(eps))))
                assert int(np.abs(_bits(got[:, 1][zero]).astype(np.int64) - int(_bits(r0)[0])).max(initial=0)) <= 1, what


@pytest.mark.parametrize('value', [float('nan'), float('inf')])
def test_bn_finalize_sticky_flag(cuda, value):
    """One non-finite partial of one channel of one sample raises the flag, and every other channel keeps its exact bits."""
    from atvsnet_amd import ops
    ops.nonfinite_seen(cuda)
    G, blocks, C, fold, pad, n = 3, 257, 8, 2, 5, 4115
    st, _, _, _ = _hand_stats(cuda, G, blocks, C, fold, pad, n, seed=5)
    clean = _finalize(st, C, cuda, None, 1e-3)
    assert not ops.nonfinite_seen(cuda), 'all-finite partials raised the flag'
    st, _, _, _ = _hand_stats(cuda, G, blocks, C, fold, pad, n, seed=5, poison=(1, 6, value))
    got = _finalize(st, C, cuda, None, 1e-3)
    assert ops.nonfinite_seen(cuda), 'a %r partial did not raise the flag' % value
    assert not ops.nonfinite_seen(cuda), 'reading the flag did not reset it'
    keep = np.ones((G, 3, C), bool)
    keep[1, :2, 6] = False
    assert np.array_equal(_bits(got)[keep], _bits(clean)[keep]), 'another channel changed'
    assert not np.isfinite(got[1, 0, 6]) or not np.isfinite(got[1, 1, 6]) or got[1, 1, 6] == 0.0


# ----------------------------------------------------------------------------------------------------- b. atvs_channel_stats

def _stats_input(kind, G, rows, C, seed):
    if kind == 'integers':
        return torch.randint(448, 577, (G, rows, C), generator=torch.Generator().manual_seed(seed)).float()
    return B.operand(kind, (G, rows, C), seed)[0]


@pytest.mark.parametrize('C', [1, 3, 12, 24, 100, 128, 129, 255, 256])
def test_channel_stats_row_by_row(cuda, C):
    from atvsnet_amd import ops
    for rows in (1, 511, 512, 513, 1537):
        for G in (1, 3):
            for kind in ('integers', 'offset', 'randn'):
                x = _stats_input(kind, G, rows, C, 1000 * C + rows + G)
                N.poison_allocator(cuda)
                st = ops.channel_stats(_dev(x, cuda), groups=G)
                torch.cuda.synchronize()
                what = 'C %d rows %d G %d %s' % (C, rows, G, kind)
                nb = (rows + 511) // 512
                assert (st.blocks, st.cpad, st.count, st.groups, st.fold) == (nb, C, rows, G, 1), what
                got = st.partial.cpu()
                assert tuple(got.shape) == (G, nb, 2, C), what
                x64 = torch.zeros(G, nb * 512, C, dtype=torch.float64)
                x64[:, :rows] = x.double()
                x64 = x64.reshape(G, nb, 512, C)
                for k, want, mass, terms in ((0, x64.sum(2), x64.abs().sum(2), 32), (1, (x64 * x64).sum(2), (x64 * x64).sum(2), 33)):
                    if kind == 'integers':
                        assert torch.equal(got[:, :, k], want), '%s: moment %d is not the integer sum' % (what, k)
                        continue
                    r = N.assert_elementwise(got[:, :, k], want, mass, terms * B.U, 0.0, '%s moment %d' % (what, k))
                    _note('channel_stats S%d' % (k + 1), kind, r)


# ------------------------------------------------------------------------------------ c. bn_apply, bn_add, bn_add_plus

SHAPES = [(1, 210, 8), (3, 4099, 16), (2, 1031, 24), (4, 777, 12)]          # sizes that end inside a span of the launch


def _operand(regime, shape, seed, flat_params=False):
    """(raw, params) on the CPU; flat_params: the (3,C) form of a single sample."""
    raw, par = B.operand(regime, shape, seed)
    return raw, (par[0].contiguous() if flat_params else par)


def _pending(raw, par, relu, dev):
    from atvsnet_amd import ops
    return ops.PendingBN(_dev(raw, dev), _dev(par, dev), relu)


@pytest.mark.parametrize('regime', B.REGIMES)
@pytest.mark.parametrize('G,rows,C', SHAPES)
def test_bn_apply_per_element(cuda, G, rows, C, regime):
    from atvsnet_amd import ops
    raw, par = _operand(regime, (G, rows, C), 300 + C, flat_params=(G == 1))
    cnd = B.bn_cond(raw, par)
    for relu in (False, True):
        N.poison_allocator(cuda)
        got = ops.bn_apply(_dev(raw, cuda), _dev(par, cuda), relu=relu, out=torch.empty(G, rows, C, device=cuda))
        torch.cuda.synchronize()
        _note('bn_apply', regime, N.assert_elementwise(got, B.bn64(raw, par, relu), cnd, B.APPLY_REL, 0.0,
                                                       'bn_apply %s relu %d' % (regime, relu)))
    # the float4 kernel on a channel slice, in place: c_off 4 of rows 2C + 4 wide; every other channel keeps its NaN bits
    for relu in (False, True):
        wide = torch.full((G, rows, 2 * C + 4), float('nan'))
        wide[..., 4:4 + C] = raw
        N.poison_allocator(cuda)
        buf = _dev(wide, cuda)
        ops.bn_apply(buf, _dev(par, cuda), relu=relu, C=C, c_off=4)
        torch.cuda.synchronize()
        _note('bn_apply', regime, N.assert_elementwise(buf[..., 4:4 + C], B.bn64(raw, par, relu), cnd, B.APPLY_REL, 0.0,
                                                       'bn_apply slice %s relu %d' % (regime, relu)))
        N.assert_bits_kept(buf, 4, 4 + C)


@pytest.mark.parametrize('regime', B.REGIMES)
@pytest.mark.parametrize('C', [3, 7])
def test_bn_apply_scalar_kernel(cuda, C, regime):
    """bn_apply_kernel<1> (C, ld or c_off not a multiple of 4): whole rows, and c_off = 2 in a buffer 2C + 5 wide; G = 3."""
    from atvsnet_amd import ops
    G, rows = 3, 1031
    raw, par = _operand(regime, (G, rows, C), 320 + C)
    cnd = B.bn_cond(raw, par)
    for relu in (False, True):
        N.poison_allocator(cuda)
        got = ops.bn_apply(_dev(raw, cuda), _dev(par, cuda), relu=relu, out=torch.empty(G, rows, C, device=cuda))
        torch.cuda.synchronize()
        _note('bn_apply<1>', regime, N.assert_elementwise(got, B.bn64(raw, par, relu), cnd, B.APPLY_REL, 0.0,
                                                          'bn_apply<1> %s relu %d' % (regime, relu)))
        wide = torch.full((G, rows, 2 * C + 5), float('nan'))
        wide[..., 2:2 + C] = raw
        N.poison_allocator(cuda)
        buf = _dev(wide, cuda)
        ops.bn_apply(buf, _dev(par, cuda), relu=relu, C=C, c_off=2)
        torch.cuda.synchronize()
        _note('bn_apply<1>', regime, N.assert_elementwise(buf[..., 2:2 + C], B.bn64(raw, par, relu), cnd, B.APPLY_REL, 0.0,
                                                          'bn_apply<1> slice %s relu %d' % (regime, relu)))
        N.assert_bits_kept(buf, 2, 2 + C)


def _sum_cases(regime, G, rows, C, dev):
    """[(name, items)]: two and three terms, pending and dense mixed, both ReLU settings."""
    shape, flat = (G, rows, C), G == 1
    ops_ = [_operand(regime, shape, 340 + i, flat_params=flat) for i in range(3)]
    dn = B.dense(regime, shape, 350)

    def p(i, relu):
        return _pending(ops_[i][0], ops_[i][1], relu, dev)
    return [('two pending', [p(0, True), p(1, False)]),
            ('pending + dense', [p(0, False), _dev(dn, dev)]),
            ('three pending', [p(0, True), p(1, True), p(2, False)]),
            ('pending, dense, pending', [p(0, False), _dev(dn, dev), p(1, True)])]


@pytest.mark.parametrize('regime', B.REGIMES)
@pytest.mark.parametrize('G,rows,C', SHAPES)
def test_bn_add_per_element(cuda, G, rows, C, regime):
    from atvsnet_amd import ops
    for name, items in _sum_cases(regime, G, rows, C, cuda):
        N.poison_allocator(cuda)
        got = ops.bn_add(items)
        torch.cuda.synchronize()
        want, cnd = B.sum64(items)
        _note('bn_add', regime, N.assert_elementwise(got, want, cnd, B.ADD_REL, 0.0, 'bn_add %s: %s' % (regime, name)))


@pytest.mark.parametrize('regime', B.REGIMES)
@pytest.mark.parametrize('G,rows,C', SHAPES)
def test_bn_add_plus_per_element(cuda, G, rows, C, regime):
    """y = the sum (the bits of bn_add), y2 = base + y with base ONE sample shared by all; keep_sum=False drops y."""
    from atvsnet_amd import ops
    base = B.dense(regime, (rows, C), 360)
    for name, items in _sum_cases(regime, G, rows, C, cuda):
        want, cnd = B.sum64(items)
        N.poison_allocator(cuda)
        alone = ops.bn_add(items)
        for keep in (True, False):
            N.poison_allocator(cuda)
            y, y2 = ops.bn_add(items, plus=_dev(base, cuda), keep_sum=keep)
            torch.cuda.synchronize()
            what = 'bn_add_plus %s: %s keep_sum %s' % (regime, name, keep)
            if keep:
                assert torch.equal(y, alone), what + ': the sum is not bn_add\'s'
            else:
                assert (y is None) if (ops.cfg.sum_on_load and ops.cfg.head_sum) else torch.equal(y, alone), what
            _note('bn_add_plus', regime, N.assert_elementwise(y2, want + base.double(), cnd + base.double().abs(), B.ADD_REL, 0.0,
                                                              what))
