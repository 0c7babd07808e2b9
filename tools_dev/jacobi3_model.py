"""A numpy model of the eigen-solver of csrc/cloud_normals.hip: the same cyclic Jacobi rotations, (0,1), (0,2), (1,2) per sweep, the
same operations in the same order in float64, vectorised over a batch of symmetric 3 x 3 matrices.  It is how the sweep count was
chosen, and what DESIGN.md section 12.2a quotes: per family of matrices, the largest off-diagonal norm relative to |C| after every
sweep, the largest residual |C V - V diag(w)| / |C| after the last in units of 2^-53, and the largest |V^T V - I|.

    python tools_dev/jacobi3_model.py [--count 200000] [--sweeps 6] [--seed 0]

It is a model on the host: it says nothing about the compiled kernel, which tests/test_gpu_cloud_normals.py holds to numpy.linalg.eigh
on the device.  tests/test_jacobi3_model.py runs it small.
"""
import argparse
import json

import numpy as np

# eigenvalues of the families: planar, near-equal pairs at either end, a thin line, all equal
FAMILIES = ([1, 1, 1e-6], [1, 1 + 1e-7, 1e-3], [1, 0.5, 0.5 + 1e-9], [1, 1e-8, 1e-9], [1, 1, 1], [1, 1e-3, 1e-3 * (1 + 1e-6)])


def rotate(app, aqq, apq, apr, aqr, V, p, q):
    """One rotation of the pair (p, q) on a batch, as jacobi_rotate in the kernel -> (app, aqq, apq = 0, apr, aqr); V in place."""
    with np.errstate(all='ignore'):
        theta = (aqq - app) / (2.0 * apq)
        mag = np.abs(theta) + np.sqrt(theta * theta + 1.0)
        t = np.where(apq == 0.0, 0.0, np.where(theta < 0.0, -1.0 / mag, 1.0 / mag))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    app, aqq = app - h, aqq + h
    apr, aqr = c * apr - s * aqr, s * apr + c * aqr
    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
    V[:, :, p] = c[:, None] * vp - s[:, None] * vq
    V[:, :, q] = s[:, None] * vp + c[:, None] * vq
    return app, aqq, np.zeros_like(apq), apr, aqr


def jacobi(C, sweeps=6):
    """C (n,3,3) symmetric -> (w (n,3) the diagonal, V (n,3,3) the rotations' product, [off-diagonal norm (n,) after each sweep])."""
    C = np.asarray(C, np.float64)
    a00, a01, a02 = C[:, 0, 0].copy(), C[:, 0, 1].copy(), C[:, 0, 2].copy()
    a11, a12, a22 = C[:, 1, 1].copy(), C[:, 1, 2].copy(), C[:, 2, 2].copy()
    V = np.tile(np.eye(3), (len(C), 1, 1))
    off = []
    for _ in range(sweeps):
        a00, a11, a01, a02, a12 = rotate(a00, a11, a01, a02, a12, V, 0, 1)
        a00, a22, a02, a01, a12 = rotate(a00, a22, a02, a01, a12, V, 0, 2)
        a11, a22, a12, a01, a02 = rotate(a11, a22, a12, a01, a02, V, 1, 2)
        off.append(np.sqrt(a01 ** 2 + a02 ** 2 + a12 ** 2))
    return np.stack([a00, a11, a22], 1), V, off


def families(count, seed):
    """Yields (name, C (count,3,3)): Gram matrices of Gaussian 3 x 3 matrices, then every family of FAMILIES in a random frame."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(count, 3, 3))
    yield 'random A A^T', A @ A.transpose(0, 2, 1)
    Q = np.linalg.qr(rng.normal(size=(count, 3, 3)))[0]
    for lam in FAMILIES:
        yield 'eigenvalues %s' % (lam,), np.einsum('nij,j,nkj->nik', Q, np.array(lam, float), Q)


def measure(C, sweeps=6):
    """-> dict: off-diagonal / |C| after each sweep (max), the eigenpairs' residual / |C| in units of 2^-53 (max), |V^T V - I| (max)."""
    C = (C + C.transpose(0, 2, 1)) / 2.0
    w, V, off = jacobi(C, sweeps)
    norm = np.linalg.norm(C, axis=(1, 2))
    residual = np.linalg.norm(np.einsum('nij,njk->nik', C, V) - V * w[:, None, :], axis=(1, 2)) / norm
    return {'offdiag_over_norm_per_sweep': [float((o / norm).max()) for o in off], 'residual_units': float(residual.max() * 2.0 ** 53),
            'orthogonality': float(np.abs(np.einsum('nji,njk->nik', V, V) - np.eye(3)).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--count', type=int, default=200000, help='matrices per family')
    ap.add_argument('--sweeps', type=int, default=6)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    for name, C in families(a.count, a.seed):
        print(json.dumps(dict(measure(C, a.sweeps), family=name, count=a.count)), flush=True)


if __name__ == '__main__':
    main()
