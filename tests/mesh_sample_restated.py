"""The surface sampling of include/atvsnet_hip.h (atvs_mesh_sample_counts, atvs_mesh_sample_offsets, atvs_mesh_sample_place) restated in
numpy, float64 and uint64, operation for operation: what tests/test_mesh_sample_host.py holds to plain Python and to statistics, and
tests/test_gpu_mesh_sample.py holds the kernels to.  numpy rounds every operation on its own, as the kernels do
(-ffp-contract=off); the one operation whose last bit may differ between the two is sqrt, which is why `counts` also returns a
margin per face (how far the face's uniform number is from the fraction it is compared with) and the normals are compared to a
float32 spacing."""
import numpy as np

SAMPLE_MAX = 1 << 28
G = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
SURE = 1e-9                     # a face is sure when its margin is at least this
INFO = ('samples', 'skipped_index_faces', 'skipped_nonfinite_faces', 'max_per_face')


def _u64(a):
    return np.atleast_1d(np.asarray(a)).astype(np.uint64)


def mix(z):
    z = _u64(z)
    z = (z ^ (z >> np.uint64(30))) * M1
    z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def hash64(base, index):
    """mix(base + G (index + 1)) mod 2^64, on arrays."""
    return mix(_u64(base) + G * (_u64(index) + np.uint64(1)))


def face_keys(seed, n_faces):
    return hash64(np.uint64(seed), np.arange(n_faces, dtype=np.uint64))


def geometry(vertices, faces):
    """-> (in range (F,) bool, a, e1, e2, n: (F,3) float64, zeros where a face's indices are out of range)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    g = np.where(ok[:, None], f, 0)
    if len(v) == 0:
        z = np.zeros((len(f), 3))
        return ok, z, z, z, z
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(invalid='ignore', over='ignore'):
        e1, e2 = b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return ok, a, e1, e2, n


def _norm(n):
    with np.errstate(invalid='ignore', over='ignore'):
        return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


def counts(vertices, faces, density, seed=0):
    """-> dict: counts (F,) int64 (uint32 on the device; beyond the limit floor(min(x, 2^32))), areas (F,) float64, x (F,), margin
    (F,) = |frac(x) - u_f| / max(1, x) (inf for a skipped face: nothing is compared there), info as ops.mesh_sample_counts gives it,
    over = the limit error's condition."""
    density = float(density)
    ok, a, e1, e2, n = geometry(vertices, faces)
    F = len(ok)
    with np.errstate(invalid='ignore', over='ignore'):
        area = 0.5 * _norm(n)
        finite = np.isfinite(area)
        live = ok & finite
        area = np.where(live, area, 0.0)
        x = area * density
        fl = np.floor(x)
        u = ((face_keys(seed, F) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
        frac = x - fl
        c = np.where(x >= SAMPLE_MAX, np.floor(np.minimum(x, 2.0 ** 32)), fl + (u < frac))
    c = np.where(live, c, 0.0).astype(np.int64)
    margin = np.where(live, np.abs(frac - u) / np.maximum(1.0, x), np.inf)
    info = dict(samples=int(c.sum()), skipped_index_faces=int((~ok).sum()), skipped_nonfinite_faces=int((ok & ~finite).sum()),
                max_per_face=int(c.max(initial=0)))
    return dict(counts=c, areas=area, x=x, margin=margin, info=info,
                over=info['max_per_face'] >= SAMPLE_MAX or info['samples'] > SAMPLE_MAX)


def offsets(count):
    """(F + 1,) int64: the exclusive prefix sum, the total last."""
    return np.concatenate([[0], np.cumsum(np.asarray(count, np.int64))])


def place(vertices, colors, faces, count, seed=0):
    """-> dict: points (S,3) float32, face (S,) int32, colors (S,3) uint8 or None, normals (S,3) float32, u, v (S,) float64."""
    count = np.asarray(count, np.int64)
    ok, a, e1, e2, n = geometry(vertices, faces)
    if (count[~ok] > 0).any():
        raise ValueError('samples on a face with a vertex index out of range')
    F = len(ok)
    off = offsets(count)
    S = int(off[-1])
    s = np.arange(S, dtype=np.int64)
    face = np.searchsorted(off, s, side='right') - 1                # the last face whose offset is <= s
    assert np.array_equal(face, np.repeat(np.arange(F), count))     # a face with count 0 is never chosen
    j = s - off[face]
    w = hash64(face_keys(seed, F)[face], j) if S else np.zeros(0, np.uint64)
    u = ((w >> np.uint64(32)).astype(np.float64) + 0.5) * 2.0 ** -32
    v = ((w & np.uint64(0xffffffff)).astype(np.float64) + 0.5) * 2.0 ** -32
    fold = u + v > 1.0
    u, v = np.where(fold, 1.0 - u, u), np.where(fold, 1.0 - v, v)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        points = ((a[face] + u[:, None] * e1[face]) + v[:, None] * e2[face]).astype(np.float32)
        normals = (n[face] / _norm(n[face])[:, None]).astype(np.float32)
    out_c = None
    if colors is not None:
        col = np.asarray(colors, np.uint8).reshape(-1, 3).astype(np.float64)
        f = np.asarray(faces, np.int64).reshape(-1, 3)[face]
        t = (1.0 - u) - v
        out_c = np.rint((t[:, None] * col[f[:, 0]] + u[:, None] * col[f[:, 1]]) + v[:, None] * col[f[:, 2]]).astype(np.uint8)
    return dict(points=points, face=face.astype(np.int32), colors=out_c, normals=normals, u=u, v=v)


def sample(vertices, colors, faces, density, seed=0):
    """counts then place of those counts -> dict(counts=the dict of `counts`, samples=the dict of `place`, area=the float64 sum)."""
    c = counts(vertices, faces, density, seed)
    if c['over']:
        raise ValueError('needs %d samples' % c['info']['samples'])
    return dict(counts=c, samples=place(vertices, colors, faces, c['counts'], seed), area=float(c['areas'].sum()))
