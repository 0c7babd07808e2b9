"""The meshes and spacings the surface sampling is held to (tests/test_mesh_sample_host.py on the restatement alone,
tests/test_gpu_mesh_sample.py on the kernels): the meshes of tests/mesh_simplify_cases.py, each at spacings 0.05 and 0.01
(`big_triangles` at 0.05 and 0.02), seed 0, and `debris` with an added copy of a face with one index out of range.  The smallest
shapes that reach every hazard: `plane` has 9522 faces (the 256-lane workgroup, the 2048-counter scan tile) of which 8667 get no
sample at 0.05, the first two and the last three among them (the face search across runs of equal offsets, in global memory); at
0.01 a workgroup's samples span about 120 faces (the search in LDS); `debris` has zero-area faces, repeated vertices, NaN and inf
vertices, and at 0.01 one face with 9729 samples (many workgroups inside one face); `cube_far` has coordinates near 1000."""
import functools

import numpy as np

import mesh_sample_restated as R
import mesh_simplify_cases as K

SEED = 0
CASES = [(name, spacing) for name in K.NAMES + ['debris_bad_index'] for spacing in ((0.05, 0.02) if name == 'big_triangles' else (0.05, 0.01))]
IDS = ['%s@%g' % c for c in CASES]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (vertices (V,3) float32, colors (V,3) uint8 or None, faces (F,3) int32): read-only."""
    if name == 'debris_bad_index':
        v, c, f = mesh('debris')
        extra = f[[0, 4]].copy()
        extra[0, 1], extra[1, 2] = len(v), -1
        return v, c, np.ascontiguousarray(np.concatenate([f[:5], extra[:1], f[5:], extra[1:]]))
    c = K.case(name)
    return c['vertices'], c['colors'], c['faces']


def density(spacing):
    return 1.0 / (spacing * spacing)


@functools.lru_cache(maxsize=None)
def restated(name, spacing, seed=SEED):
    """The restatement of a case, computed once and shared: treat it as read-only."""
    v, c, f = mesh(name)
    return R.sample(v, c, f, density(spacing), seed)
