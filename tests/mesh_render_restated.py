"""The definition of atvs_mesh_render and atvs_depth_occlude (include/atvsnet_hip.h) restated in numpy, DENSE: every face against
every pixel of every camera, no bounding boxes, so a kernel whose box is too small cannot agree with it.  float64 in the stated
order (numpy rounds every operation, nothing is contracted), np.minimum on uint64 keys.  Cameras are independent and run on a few
threads (numpy releases the interpreter lock inside its loops).  With it the helpers the tests share: ring cameras, a subdivided
octahedron on a sphere, a triangle soup, and the two known answers that the host and the device tests both check."""
import concurrent.futures

import numpy as np

from scan_render_restated import ring_cameras  # noqa: F401  (the cameras of the scan renderer's tests)

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
_CHUNK = 1 << 20                                     # (faces x pixels) elements per step: arrays of 8 MB


def camera_space(vertices, cam):
    """-> (V,3) float64: C_k = ((c[3k] X + c[3k+1] Y) + c[3k+2] Z) + c[9+k]."""
    p = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    c = np.asarray(cam, np.float64).reshape(16)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all='ignore'):
        return np.stack([((c[3 * k] * X + c[3 * k + 1] * Y) + c[3 * k + 2] * Z) + c[9 + k] for k in range(3)], 1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def keys(vertices, faces, cam, rows, cols, pixel_centre=0.0):
    """-> (rows, cols) uint64: per pixel the smallest (bits(z) << 32) | face of one camera, all-ones where nothing is covered.
    Every index of `faces` must be valid."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    c = np.asarray(cam, np.float64).reshape(16)
    out = np.full(rows * cols, EMPTY, np.uint64)
    if not len(faces):
        return out.reshape(rows, cols)
    pc = float(pixel_centre)
    with np.errstate(all='ignore'):
        C = camera_space(vertices, cam)
        A, B, D = C[faces[:, 0]], C[faces[:, 1]], C[faces[:, 2]]
        part = np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(D).all(1) & ((A[:, 2] > 0) | (B[:, 2] > 0) | (D[:, 2] > 0))
        N = [_cross(B, D), _cross(D, A), _cross(A, B)]
        det = (A[:, 0] * N[0][:, 0] + A[:, 1] * N[0][:, 1]) + A[:, 2] * N[0][:, 2]
        rx = ((np.arange(cols, dtype=np.float64) + pc) - c[14]) / c[12]
        ry = ((np.arange(rows, dtype=np.float64) + pc) - c[15]) / c[13]
        index = np.flatnonzero(part)
        step = max(1, _CHUNK // (rows * cols))
        for s in range(0, len(index), step):
            f = index[s:s + step]
            # E_i = (Ni_0 rx + Ni_1 ry) + Ni_2 at pixel v * cols + u: the two products are formed per column and per row
            E = [((n[f, 0:1] * rx[None, :])[:, None, :] + (n[f, 1:2] * ry[None, :])[:, :, None]).reshape(len(f), -1) for n in N]
            for e, n in zip(E, N):
                e += n[f, 2:3]
            S = (E[0] + E[1]) + E[2]
            lo = np.minimum(np.minimum(E[0], E[1]), E[2])
            hi = np.maximum(np.maximum(E[0], E[1], out=E[0]), E[2], out=E[0])
            # np.minimum propagates NaN, and a NaN fails the comparison as it fails each of the three
            cover = ((lo >= 0) & (S > 0)) | ((hi <= 0) & (S < 0))
            fi, px = np.nonzero(cover)
            if not len(fi):
                continue
            t = det[f][fi] / S[fi, px]
            z = t.astype(np.float32)
            ok = (t > 0) & np.isfinite(z) & (z > 0)
            key = (z[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | f[fi[ok]].astype(np.uint64)
            np.minimum.at(out, px[ok], key)
    return out.reshape(rows, cols)


def resolve(k):
    """keys -> (depth float32, face int32)."""
    empty = k == EMPTY
    depth = np.where(empty, np.uint32(0), (k >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(np.float32)
    face = np.where(empty, -1, (k & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    return depth, face


def mesh_render(vertices, faces, cams, rows, cols, pixel_centre=0.0):
    """-> (depth (n_cams, rows, cols) float32, face (n_cams, rows, cols) int32)."""
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    depth = np.zeros((len(cams), rows, cols), np.float32)
    face = np.full((len(cams), rows, cols), -1, np.int32)

    def one(k):
        depth[k], face[k] = resolve(keys(vertices, faces, cams[k], rows, cols, pixel_centre))
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, len(cams))) as pool:
        list(pool.map(one, range(len(cams))))
    return depth, face


def depth_occlude(depth, occluder, tol=0.0):
    """out = 0 where occluder > 0 and depth > 0 and not (depth <= occluder (1 + tol)) in float64, else depth."""
    d = np.asarray(depth, np.float32)
    o = np.asarray(occluder, np.float32)
    with np.errstate(all='ignore'):
        hidden = (o > 0) & (d > 0) & ~(d.astype(np.float64) <= o.astype(np.float64) * (1.0 + float(tol)))
    return np.where(hidden, np.float32(0), d).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- helpers

def octahedron_sphere(levels, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """An octahedron subdivided `levels` times (8 * 4^levels faces), vertices pushed onto the sphere and shared between faces ->
    (vertices (V,3) float32, faces (F,3) int32), closed and consistently oriented."""
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    verts = [np.array(v, np.float64) for v in verts]
    for _ in range(levels):
        mid, nxt = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nxt += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = nxt
    v = np.asarray(verts) * float(radius) + np.asarray(centre, np.float64)
    return v.astype(np.float32), np.asarray(faces, np.int32)


def sphere_silhouette(cam, rows, cols, radius, centre=(0.0, 0.0, 0.0), pixel_centre=0.0):
    """-> (hit (rows, cols) bool, depth, cos): whether the ray through each pixel centre meets the sphere in front of the camera,
    the camera depth of the nearer intersection and the cosine of the angle of incidence there (float64, analytic)."""
    c = np.asarray(cam, np.float64).reshape(16)
    o = c[:9].reshape(3, 3) @ np.asarray(centre, np.float64) + c[9:12]              # the centre in the camera's frame
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    r = np.stack([((u + pixel_centre) - c[14]) / c[12], ((v + pixel_centre) - c[15]) / c[13], np.ones_like(u)], -1)
    rr, ro = (r * r).sum(-1), r @ o
    disc = ro * ro - rr * (o @ o - radius * radius)
    with np.errstate(all='ignore'):
        t = (ro - np.sqrt(disc)) / rr
        hit = (disc > 0) & (t > 0)
        normal = (r * t[..., None] - o) / radius
        cos = -(normal * r).sum(-1) / np.sqrt(rr)
    return hit, t, cos


def triangle_soup(n, cams, rows, cols, seed=0):
    """n triangles for the cameras `cams` (ring cameras around the origin) -> (vertices (3n,3) float32, faces (n,3) int32).
    Sizes are log-uniform from a tenth of a pixel to twice the image (measured at the distance of the ring's centre); centres fill a
    box that holds the cameras, so faces cross camera planes, lie behind every camera of a side, and come very near one.  The last
    tenth is degenerate: zero-area (a repeated position), a repeated index, collapsed to a segment, NaN and infinite vertices."""
    rng = np.random.default_rng(seed)
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    radius = float(np.linalg.norm(cams[0, :9].reshape(3, 3).T @ -cams[0, 9:12]))
    pixel = radius / float(cams[0, 12])                                  # a pixel's footprint at the ring's centre
    size = pixel * np.exp(rng.uniform(np.log(0.1), np.log(2.0 * max(rows, cols)), n))
    centre = rng.uniform(-1.3 * radius, 1.3 * radius, (n, 3))
    near = rng.choice(n, n // 20, replace=False)                         # very near a camera: a few thousandths in front of its centre
    k = rng.integers(0, len(cams), len(near))
    R = cams[k, :9].reshape(-1, 3, 3)
    eye = np.einsum('nji,nj->ni', R, -cams[k, 9:12])
    centre[near] = eye + R[:, 2] * rng.uniform(1e-3, 5e-2, (len(near), 1))
    size[near] *= rng.uniform(0.01, 1.0, len(near))
    tri = centre[:, None, :] + rng.normal(size=(n, 3, 3)) * size[:, None, None]
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    bad = np.arange(n - n // 10, n)
    kind = np.arange(len(bad)) % 5
    tri[bad[kind == 0], 1] = tri[bad[kind == 0], 0]                      # zero area: two vertices at one position
    faces[bad[kind == 1], 2] = faces[bad[kind == 1], 0]                  # a repeated index
    seg = bad[kind == 2]
    tri[seg, 2] = 0.5 * (tri[seg, 0] + tri[seg, 1])                      # collapsed to (nearly) a segment
    tri[bad[kind == 3], rng.integers(0, 3, (kind == 3).sum()), rng.integers(0, 3, (kind == 3).sum())] = np.nan
    tri[bad[kind == 4], rng.integers(0, 3, (kind == 4).sum()), rng.integers(0, 3, (kind == 4).sum())] = \
        np.where(rng.random((kind == 4).sum()) < 0.5, np.inf, -np.inf)
    return tri.reshape(-1, 3).astype(np.float32), faces


def soup_sizes(vertices, faces, cams):
    """The longest edge of every face in pixels at the distance of the ring's centre (NaN for a face that is not finite)."""
    cams = np.asarray(cams, np.float64).reshape(-1, 16)
    pixel = float(np.linalg.norm(cams[0, 9:12])) / float(cams[0, 12])
    t = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    with np.errstate(invalid='ignore'):
        edge = np.stack([np.linalg.norm(t[:, i] - t[:, (i + 1) % 3], axis=1) for i in range(3)], 1).max(1)
    return np.where(np.isfinite(edge), edge, np.nan) / pixel


# ------------------------------------------------------------------------------- known answers, for the host and the device

# tests/test_gpu_scan_render.py's LATTICE_CAM: identity rotation, t = (0.5, -0.25, 0.5), fx = fy = 32, cx = 16, cy = 12
LATTICE_CAM = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, -0.25, 0.5, 32, 32, 16, 12], np.float64)


def lattice_square(depth=2.5, x=(5.0, 30.0), y=(3.0, 18.0)):
    """Two triangles over the rectangle of image coordinates x, y at camera depth `depth`: every number is exact."""
    xs = np.array([x[0], x[1], x[1], x[0]])
    ys = np.array([y[0], y[0], y[1], y[1]])
    v = np.stack([(xs - 16.0) * depth / 32.0 - 0.5, (ys - 12.0) * depth / 32.0 + 0.25, np.full(4, depth - 0.5)], 1)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def check_lattice(render):
    """render(vertices, faces, cams, rows, cols, pixel_centre) -> (depth, face) of LATTICE_CAM: shared with the device test."""
    rows, cols = 24, 32
    v, f = lattice_square()
    for centre, (u0, u1, v0, v1) in ((0.0, (5, 30, 3, 18)), (0.5, (5, 29, 3, 17))):     # pixel centres inside [5, 30] x [3, 18]
        depth, face = render(v, f, LATTICE_CAM[None], rows, cols, centre)
        want = np.zeros((rows, cols), np.float32)
        want[v0:v1 + 1, u0:u1 + 1] = np.float32(2.5)
        assert np.array_equal(depth[0], want), centre
        assert np.array_equal(face[0] >= 0, want > 0)
        # face 0 = (0,1,2) lies above the diagonal from (5,3) to (30,18), face 1 below it; the diagonal itself goes to face 0
        uu, vv = np.meshgrid(np.arange(cols) + centre, np.arange(rows) + centre)
        side = (vv - 3.0) * 25.0 - (uu - 5.0) * 15.0                                   # 0 on the diagonal, > 0 below it
        inside = want > 0
        assert np.array_equal(face[0][inside], np.where(side[inside] > 0, 1, 0))
        assert (side[inside] == 0).sum() >= 5


def check_watertight_sphere(render, rows=60, cols=80):
    v, f = octahedron_sphere(3)
    assert len(f) == 512
    cams = ring_cameras(3, rows, cols, radius=3.0)
    depth, face = render(v, f, cams, rows, cols, 0.0)
    for k in range(len(cams)):
        inner, _, _ = sphere_silhouette(cams[k], rows, cols, 0.97)
        outer, t, _ = sphere_silhouette(cams[k], rows, cols, 1.0)
        assert inner.sum() > 500
        assert ((depth[k] == 0) & inner).sum() == 0                  # the chords' sagitta is 0.012 at 3 levels: no crack, no hole
        assert ((depth[k] > 0) & ~outer).sum() == 0                  # the mesh is inscribed
        assert (depth[k][inner] >= t[inner] * (1 - 1e-6)).all()      # and lies behind the sphere's front
