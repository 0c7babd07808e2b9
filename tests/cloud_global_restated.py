"""The global registration's three kernels (include/atvsnet_hip.h: atvs_cloud_fpfh, atvs_cloud_feature_nearest,
atvs_cloud_ransac_score) and register_cloud.global_init restated with numpy, operation for operation: descriptors in float64 with
the header's bin rule, the feature distance a float32 loop in bin order, the hypotheses in float64 in the same order.  Nothing here
imports the product; the limits and the edge table are read from the header's text.

THE DESCRIPTOR'S BAR (FPFH_BAR).  Device and restatement perform the same IEEE operations in the same order, so they agree bit for
bit wherever division and square root are correctly rounded.  The bar does not rely on that: it allows every one of the operations
that reach an output bin to differ by one unit of 2^-53 -- a bin's sum g_b takes at most k additions of one product each, whose
weight r took a product and a division (4 k roundings, k <= 32), its part's sum s 11 such values and 10 additions, the point's own
f_b one division, and (f_b + g_b / s) 0.5 three more: below 4 k + 11 (4 k) + 10 + 4 <= 1600 units of 2^-53 relative to a value that
is at most 1 -- and then one float32
rounding, half a last place of a value below 1 (2^-25), which such a difference can turn into a whole one (2^-24):
FPFH_BAR = 2^-24 + 1600 x 2^-53.  A pair whose feature lies within 1e-9 (relative) of a bin edge can fall into either bin under
such a difference; `fpfh` reports the rows that have one, and the tests leave those rows out (at most 1 % of a cloud)."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_restated as KR  # noqa: E402
import cloud_register_restated as RR  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'atvsnet_hip.h')


def header_value(name, text=None):
    """The text after `#define name` in the header."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    m = re.search(r'^#define\s+%s\s+(.+?)\s*$' % re.escape(name), text, re.M)
    if not m:
        raise RuntimeError('%s defines no %s' % (HEADER, name))
    return m.group(1)


def header_table(name, text=None):
    return [float(v) for v in header_value(name, text).strip('{} ').split(',')]


BINS = int(header_value('ATVS_CLOUD_FPFH_BINS'))
WIDTH = 3 * BINS
MAX_K = int(header_value('ATVS_CLOUD_MAX_K'))
MAX_BEST = int(header_value('ATVS_CLOUD_RANSAC_MAX_BEST'))
MIN_EDGE2 = float(header_value('ATVS_CLOUD_RANSAC_MIN_EDGE2'))
THETA_COS = np.array(header_table('ATVS_CLOUD_FPFH_THETA_COS'), np.float64)
THETA_SIN = np.array(header_table('ATVS_CLOUD_FPFH_THETA_SIN'), np.float64)
LINEAR_EDGES = np.array([2.0 * e - 11.0 for e in range(1, 11)])           # 11 times the edges -9/11 .. 9/11
MIN_SIN2 = 1e-12
EDGE_NEAR = 1e-9
FPFH_BAR = 2.0 ** -24 + 1600 * 2.0 ** -53
PART_SUM_BAR = 2.0 ** -22


def linear_bin(v):
    """The number of the ten edges at or below v (11 v >= 2 e - 11): a tie goes to the upper bin.  -> (bin, near an edge)."""
    v11 = 11.0 * np.asarray(v, np.float64)
    gap = np.abs(v11[..., None] - LINEAR_EDGES)
    return (v11[..., None] >= LINEAR_EDGES).sum(axis=-1), (gap <= EDGE_NEAR * 11.0).any(axis=-1)


def theta_bin(x, y):
    """The number of the ten edge directions with C_e y - S_e x >= 0; no angle is formed.  -> (bin, near an edge)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    cross = THETA_COS * y[..., None] - THETA_SIN * x[..., None]
    size = np.sqrt(x * x + y * y)
    return (cross >= 0.0).sum(axis=-1), (np.abs(cross) <= EDGE_NEAR * size[..., None]).any(axis=-1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def spfh(points, idx, normals, storage=np.float32):
    """-> (hist (n,33) int64: the counts, pairs (n,) int64: the counting pairs, near (n,) bool: a pair's feature near a bin edge).
    storage: what the inputs are rounded to first -- float32 as the kernel reads them; float64 for the invariance test, which moves
    a cloud without rounding it again."""
    P, N = np.asarray(points, storage).reshape(-1, 3).astype(np.float64), np.asarray(normals, storage).reshape(-1, 3).astype(np.float64)
    n = len(P)
    idx = np.asarray(idx, np.int32).reshape(n, -1)
    k = idx.shape[1]
    fin_p, fin_n = np.isfinite(P).all(axis=1), np.isfinite(N).all(axis=1)
    rows = np.arange(n)
    hist, pairs, near = np.zeros((n, WIDTH), np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    with np.errstate(all='ignore'):
        own = fin_p & fin_n & (_dot(N, N) > 0.0)
        c = np.zeros((n, 3))
        for t in range(k):
            i = idx[:, t]
            ok = (i >= 0) & (i < n)
            j = np.where(ok, i, 0)
            ok &= fin_p[j]
            c = c + np.where(ok[:, None], P[j] - P, 0.0)
        u = N * np.where(_dot(N, c) < 0.0, -1.0, 1.0)[:, None]
        for t in range(k):
            i = idx[:, t]
            ok = (i >= 0) & (i < n)
            j = np.where(ok, i, 0)
            m, d = N[j], P[j] - P
            dd = _dot(d, d)
            g = _cross(u, d)
            gg = _dot(g, g)
            counts = ok & own & fin_p[j] & fin_n[j] & (_dot(m, m) > 0.0) & (dd > 0.0) & (gg > 0.0)
            m = m * np.where(_dot(u, m) < 0.0, -1.0, 1.0)[:, None]
            v = g / np.sqrt(gg)[:, None]
            w = _cross(u, v)
            alpha, phi = _dot(v, m), _dot(u, d) / np.sqrt(dd)
            x, y = _dot(u, m), _dot(w, m)
            (ba, na), (bp, npr), (bt, nt) = linear_bin(alpha), linear_bin(phi), theta_bin(x, y)
            r = rows[counts]
            hist[r, ba[counts]] += 1
            hist[r, BINS + bp[counts]] += 1
            hist[r, 2 * BINS + bt[counts]] += 1
            pairs[r] += 1
            near[r] |= (na | npr | nt)[counts]
    return hist, pairs, near


def fpfh(points, idx, normals, storage=np.float32):
    """-> (descriptors (n,33) float32, near (n,) bool: the row, or a row it gathers, has a pair's feature near a bin edge)."""
    P = np.asarray(points, storage).reshape(-1, 3).astype(np.float64)
    n = len(P)
    idx = np.asarray(idx, np.int32).reshape(n, -1)
    hist, pairs, near_own = spfh(points, idx, normals, storage)
    fin_p = np.isfinite(P).all(axis=1)
    near = near_own.copy()
    with np.errstate(all='ignore'):
        f = hist.astype(np.float64) / pairs.astype(np.float64)[:, None]
        g = np.zeros((n, WIDTH))
        for t in range(idx.shape[1]):
            i = idx[:, t]
            ok = (i >= 0) & (i < n)
            j = np.where(ok, i, 0)
            d = P[j] - P
            dd = _dot(d, d)
            ok &= fin_p[j] & (dd > 0.0) & (pairs[j] > 0)
            r = 1.0 / (pairs[j].astype(np.float64) * dd)
            g = g + np.where(ok[:, None], hist[j].astype(np.float64) * r[:, None], 0.0)
            near |= ok & near_own[j]
        out = np.zeros((n, WIDTH), np.float32)
        for part in range(3):
            s = np.zeros(n)
            for b in range(BINS):
                s = s + g[:, part * BINS + b]
            own = f[:, part * BINS:(part + 1) * BINS]
            q = (own + g[:, part * BINS:(part + 1) * BINS] / s[:, None]) * 0.5
            out[:, part * BINS:(part + 1) * BINS] = np.where((s > 0.0)[:, None], q, own).astype(np.float32)
    out[pairs == 0] = 0.0
    return out, near & (pairs > 0)


def feature_nearest(ref, query, chunk=512):
    """-> (d2 (m,) float32, idx (m,) int32): a float32 loop over the 33 bins in ascending order; all-zero reference rows never
    match, an all-zero query gets (+inf, -1); the lowest index wins a tie (argmin returns the first of equals)."""
    R, Q = np.asarray(ref, np.float32).reshape(-1, WIDTH), np.asarray(query, np.float32).reshape(-1, WIDTH)
    m = len(Q)
    d2, idx = np.full(m, np.inf, np.float32), np.full(m, -1, np.int32)
    live = (R != 0).any(axis=1)
    if not live.any():
        return d2, idx
    for lo in range(0, m, chunk):
        q = Q[lo:lo + chunk]
        with np.errstate(all='ignore'):
            e = q[:, None, 0] - R[None, :, 0]
            acc = e * e
            for b in range(1, WIDTH):
                e = q[:, None, b] - R[None, :, b]
                acc = acc + e * e
        assert acc.dtype == np.float32
        acc = np.where(live[None, :] & ~np.isnan(acc), acc, np.float32(np.inf))
        at = acc.argmin(axis=1)
        best = acc[np.arange(len(q)), at]
        found = (best < np.inf) & (q != 0).any(axis=1)
        d2[lo:lo + chunk] = np.where(found, best, np.float32(np.inf))
        idx[lo:lo + chunk] = np.where(found, at, -1)
    return d2, idx


def _frames(P, tri):
    """The frame of every triangle -> (X, Y, Z, L (h,3), G, ok)."""
    x0, x1, x2 = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    p, q, r = x1 - x0, x2 - x0, x2 - x1
    G = ((x0 + x1) + x2) / 3.0
    pp, qq, rr = _dot(p, p), _dot(q, q), _dot(r, r)
    L = np.stack([np.sqrt(pp), np.sqrt(qq), np.sqrt(rr)], 1)
    X = p / L[:, :1]
    z = q - _dot(q, X)[:, None] * X
    zz = _dot(z, z)
    Y = z / np.sqrt(zz)[:, None]
    ok = (pp >= MIN_EDGE2) & (qq >= MIN_EDGE2) & (rr >= MIN_EDGE2) & (zz > MIN_SIN2 * qq)
    return X, Y, _cross(X, Y), L, G, ok


def hypotheses(src, dst, triples, with_scale, edge_ratio=0.9):
    """-> (M (h,3,4) float64, valid (h,) bool, reason (h,) of '', 'index', 'edge', 'area', 'ratio': the first rule that fails)."""
    S, D = np.asarray(src, np.float32).reshape(-1, 3).astype(np.float64), np.asarray(dst, np.float32).reshape(-1, 3).astype(np.float64)
    tri = np.asarray(triples, np.int32).reshape(-1, 3).astype(np.int64)
    c, h = len(S), len(tri)
    inside = ((tri >= 0) & (tri < c)).all(axis=1) & (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    safe = np.where(inside[:, None], tri, np.array([[0, 0, 0]]))
    reason = np.full(h, '', dtype=object)
    with np.errstate(all='ignore'):
        Xs, Ys, Zs, Ls, Gs, oks = _frames(S, safe)
        Xd, Yd, Zd, Ld, Gd, okd = _frames(D, safe)
        scale = ((Ld[:, 0] + Ld[:, 1]) + Ld[:, 2]) / ((Ls[:, 0] + Ls[:, 1]) + Ls[:, 2]) if with_scale else np.ones(h)
        ratio = np.ones(h, bool)
        for e in range(3):
            sl = scale * Ls[:, e]
            ratio &= (Ld[:, e] >= edge_ratio * sl) & (edge_ratio * Ld[:, e] <= sl)
        M = np.zeros((h, 3, 4))
        for r in range(3):
            for col in range(3):
                M[:, r, col] = scale * ((Xd[:, r] * Xs[:, col] + Yd[:, r] * Ys[:, col]) + Zd[:, r] * Zs[:, col])
            M[:, r, 3] = Gd[:, r] - ((M[:, r, 0] * Gs[:, 0] + M[:, r, 1] * Gs[:, 1]) + M[:, r, 2] * Gs[:, 2])
    edges = np.ones(h, bool)
    for P in (S, D):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            e = P[safe[:, b]] - P[safe[:, a]]
            with np.errstate(all='ignore'):
                edges &= _dot(e, e) >= MIN_EDGE2
    valid = inside & oks & okd & ratio
    reason[~ratio] = 'ratio'
    reason[~(oks & okd)] = 'area'
    reason[~edges] = 'edge'
    reason[~inside] = 'index'
    M[~valid] = 0.0
    return M, valid, reason


def ransac(src, dst, triples, tau, with_scale, edge_ratio=0.9, best=4):
    """-> (the `best` dicts {matrix (3,4), count, sum, index} in the order larger count, smaller sum, lower index; slots beyond the
    valid hypotheses: zeros, -1, 0.0, -1), counts (h,) int64 with -1 for the invalid, sums (h,) float64)."""
    S, D = np.asarray(src, np.float32).reshape(-1, 3).astype(np.float64), np.asarray(dst, np.float32).reshape(-1, 3).astype(np.float64)
    M, valid, _ = hypotheses(src, dst, triples, with_scale, edge_ratio)
    h = len(M)
    rows = np.flatnonzero(valid)
    V = M[rows]
    count, total = np.zeros(len(rows), np.int64), np.zeros(len(rows))
    tau2 = float(tau) * float(tau)
    with np.errstate(all='ignore'):
        for i in range(len(S)):
            x, b = S[i], D[i]
            e = [(((V[:, r, 0] * x[0] + V[:, r, 1] * x[1]) + V[:, r, 2] * x[2]) + V[:, r, 3]) - b[r] for r in range(3)]
            d = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            inl = d <= tau2
            count += inl
            total = total + np.where(inl, d, 0.0)
    counts, sums = np.full(h, -1, np.int64), np.zeros(h)
    counts[rows], sums[rows] = count, total
    order = sorted(rows.tolist(), key=lambda j: (-counts[j], sums[j], j))[:best]
    out = [{'matrix': M[j].copy(), 'count': int(counts[j]), 'sum': float(sums[j]), 'index': int(j)} for j in order]
    out += [{'matrix': np.zeros((3, 4)), 'count': -1, 'sum': 0.0, 'index': -1}] * (best - len(out))
    return out, counts, sums


def normals_pca(points, idx):
    """Unoriented PCA normals of a cloud from its own neighbours, the point itself a sample (ops.cloud_normals(self_counts=True) to
    rounding; numpy.linalg.eigh in the place of the fixed Jacobi sweeps) -> (n,3) float32, the zero row below 3 samples or two
    directions."""
    P = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    idx = np.asarray(idx, np.int32).reshape(len(P), -1)
    ok = idx >= 0
    d = np.where(ok[:, :, None], P[np.where(ok, idx, 0)] - P[:, None, :], 0.0)
    c = ok.sum(axis=1) + 1.0
    s = d.sum(axis=1)
    C = np.einsum('nka,nkb->nab', d, d) - s[:, :, None] * s[:, None, :] / c[:, None, None]
    w, V = np.linalg.eigh(C)
    n = V[:, :, 0].copy()
    lead = np.abs(n).argmax(axis=1)
    n *= np.where(n[np.arange(len(n)), lead] < 0.0, -1.0, 1.0)[:, None]
    n[(c < 3) | ~(w[:, 1] > 1e-12 * w[:, 2])] = 0.0
    return n.astype(np.float32)


def bounds_diagonal(points):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    return float(np.sqrt(((p.max(axis=0) - p.min(axis=0)) ** 2).sum()))


def describe(points, feature_voxel, normal_k, feature_k, feature_radius):
    """Steps 1-3 of global_init for one cloud -> (down-sampled points float32, normals, descriptors)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    origin = np.floor(p[np.isfinite(p).all(axis=1)].astype(np.float64).min(axis=0))
    down = RR.voxel_downsample(p, feature_voxel, origin)[0]
    knn = KR.knn(down, down, feature_radius, max(normal_k, feature_k), exclude_same_index=True)[1]     # the first k of a longer list
    nrm = normals_pca(down, knn[:, :normal_k])
    return down, nrm, fpfh(down, knn[:, :feature_k], nrm)[0]


def match(recon, gt, with_scale=False, voxel=None, feature_voxel=None, normal_k=16, feature_k=32, feature_radius=None, tau=None,
          mutual=True):
    """Steps 1-4 of register_cloud.global_init over the restatements -> dict(src, dst: the down-sampled clouds; a, b: the matched
    rows; tau, feature_voxel, n_matches, n_mutual)."""
    if feature_voxel is None:
        fv = (bounds_diagonal(recon) / 64.0, bounds_diagonal(gt) / 64.0) if with_scale else (2.0 * voxel, 2.0 * voxel)
    else:
        fv = tuple(feature_voxel) if np.ndim(feature_voxel) else (float(feature_voxel), float(feature_voxel))
    radius = (5.0 * fv[0], 5.0 * fv[1]) if feature_radius is None else (
        tuple(feature_radius) if np.ndim(feature_radius) else (float(feature_radius),) * 2)
    tau = 1.5 * fv[1] if tau is None else float(tau)
    src, _, fs = describe(recon, fv[0], normal_k, feature_k, radius[0])
    dst, _, fd = describe(gt, fv[1], normal_k, feature_k, radius[1])
    fwd = feature_nearest(fd, fs)[1]
    rows = np.flatnonzero(fwd >= 0)
    n_matches = n_mutual = len(rows)
    if mutual:
        back = feature_nearest(fs, fd)[1]
        agree = rows[back[fwd[rows]] == rows]
        n_mutual = len(agree)
        if 3 * n_mutual >= n_matches:
            rows = agree
    if len(rows) < 3:
        raise ValueError('global_init: %d matches' % len(rows))
    return {'src': src, 'dst': dst, 'a': src[rows], 'b': dst[fwd[rows]], 'tau': tau, 'feature_voxel': fv, 'n_matches': n_matches,
            'n_mutual': n_mutual, 'with_scale': with_scale}


def solve(matched, hypotheses=65536, seed=0, edge_ratio=0.9, best=4):
    """Steps 5-8 over what `match` returned -> dict(matrix 4x4, fitness, n_valid, ...)."""
    src, dst, a, b, tau = (matched[k] for k in ('src', 'dst', 'a', 'b', 'tau'))
    triples = np.random.Generator(np.random.PCG64(seed)).integers(0, len(a), size=(hypotheses, 3), dtype=np.int32)
    cands, counts, _ = ransac(a, b, triples, tau, matched['with_scale'], edge_ratio, best)
    if cands[0]['count'] < 0:
        raise ValueError('global_init: no valid hypothesis')
    fits = []
    for cand in cands:
        if cand['count'] < 0:
            continue
        T = np.vstack([cand['matrix'], [0.0, 0.0, 0.0, 1.0]])
        d2 = RR.nearest(RR.transform(src, T), dst, tau * (1.0 + 2.0 ** -20))[0]
        fits.append((float((d2.astype(np.float64) <= tau * tau).sum()) / len(src), T))
    fitness, T = max(fits, key=lambda f: f[0])              # max returns the first of equals: RANSAC's order
    return {'matrix': T, 'fitness': fitness, 'n_matches': matched['n_matches'], 'n_mutual': matched['n_mutual'],
            'n_valid': int((counts >= 0).sum()), 'n_src': len(src), 'n_dst': len(dst), 'tau': tau, 'feature_voxel': matched['feature_voxel']}


def global_init(recon, gt, hypotheses=65536, seed=0, edge_ratio=0.9, best=4, **options):
    """register_cloud.global_init step for step: `match` (its options), then `solve`."""
    return solve(match(recon, gt, **options), hypotheses, seed, edge_ratio, best)


def sphere(n, seed, radius=1.0):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (radius * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def fpfh_case(case):
    """-> (points float32, k, radius): the five clouds the descriptor is tested on, on the GPU and (the cap on rows near a bin
    edge) on the CPU."""
    rng = np.random.default_rng(11)
    if case == 'plane':
        return np.concatenate([rng.uniform(0, 1, (257, 2)), rng.normal(0, 0.002, (257, 1))], 1).astype(np.float32), 8, 0.2
    if case == 'room':
        return RR.shape(4097, 3, 0.002).astype(np.float32), 16, 0.15
    if case == 'sphere':
        return sphere(4097, 5), 32, 0.2
    if case == 'sparse':
        return sphere(65, 6), 2, 0.25
    p = RR.shape(513, 4, 0.002).astype(np.float32)               # 'edited': duplicates and a non-finite point
    p[100:120] = p[200:220]
    p[7] = np.nan
    return p, 12, 0.3


def fpfh_edits(case, idx, normals):
    """The hand edits of the 'edited' case: zero and non-finite normals, an index past the end, a padded hole."""
    if case == 'edited':
        normals[::17] = 0.0
        normals[5, 1] = np.nan
        normals[6, 2] = np.inf
        idx[9, 3] = len(idx)
        idx[10, 0] = -1
    return idx, normals


def features(n, seed):
    """Rows shaped like descriptors (three parts that sum to 1), with exact duplicates and all-zero rows."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0, 1, (n, 3, 11)) ** 4
    f = (f / f.sum(axis=2, keepdims=True)).reshape(n, 33).astype(np.float32)
    if n > 16:
        f[n // 2] = f[3]                                     # duplicates: the lower index wins
        f[n - 1] = f[3]
        f[5::13] = 0.0
    return f


def ransac_case(c, h, with_scale, seed=0):
    """Planted inliers under a known similarity -> (src, dst, triples, tau, the planted count).  Rows 0, 1, 2 are inliers in a
    good triangle and triple 0 names them; further triples break one rule each (where c and h leave room), the rest are random."""
    rng = np.random.default_rng(seed + c + h)
    src = rng.uniform(-1, 1, (c, 3))
    src[:3] = [[-0.8, -0.7, 0.1], [0.9, -0.2, 0.0], [0.1, 0.8, -0.3]]
    M = RR.similarity(RR.rotation((1, 2, -1), 77.0), (3.0, -2.0, 5.0), 1.7 if with_scale else 1.0, (0.1, 0.2, 0.3))
    planted = max(3, (2 * c) // 5)
    dst = rng.uniform(-1, 1, (c, 3)) * 2.0 + M[:3, 3]
    dst[:planted] = src[:planted] @ M[:3, :3].T + M[:3, 3]
    if c > 16:
        src[6], dst[6] = src[5], dst[5]                          # a zero edge between different indices
        src[7:10] = [[0.0, 0.0, 0.0], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5]]       # three points on a line
        dst[7:10] = src[7:10] @ M[:3, :3].T + M[:3, 3]
    triples = rng.integers(0, c, (h, 3)).astype(np.int32)
    triples[0] = [0, 1, 2]
    special = [[0, 0, 1], [c, 0, 1], [-1, 0, 1], [0, 1, c - 1]]
    if c > 16:
        special += [[5, 6, 0], [7, 8, 9], [1, 0, 2], [2, 1, 0]]
    for j, t in enumerate(special[:max(0, h - 1)]):
        triples[1 + j] = t
    return src.astype(np.float32), dst.astype(np.float32), triples, 1e-3, planted, M


def moved_room(seed, with_scale, n=4097, noise=0.002):
    """The asymmetric room (ground truth, float32) and a source that is the same cloud under the INVERSE of M = a rotation of 150
    degrees about (1, -2, 0.5) through the centroid, a translation of several room sizes and, with_scale, the factor 1.7: M moves
    the source back.  -> (gt, src, M)."""
    gt = RR.shape(n, seed, noise).astype(np.float32)
    g = gt.astype(np.float64)
    M = RR.similarity(RR.rotation((1, -2, 0.5), 150.0), (7.0, -5.0, 9.0), 1.7 if with_scale else 1.0, g.mean(axis=0))
    Mi = np.linalg.inv(M)
    return gt, (g @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32), M


def corner_error(T, M, src):
    """The largest distance between a corner of src's box under T and under M."""
    c = RR.corners_of(src)
    d = (c @ T[:3, :3].T + T[:3, 3]) - (c @ M[:3, :3].T + M[:3, 3])
    return float(np.sqrt((d * d).sum(axis=1)).max())
