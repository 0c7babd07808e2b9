"""CPU: the numpy model of csrc/cloud_normals.hip's eigen-solver (tools_dev/jacobi3_model.py), run small: what DESIGN.md section
12.2a quotes from it holds on a fresh draw -- the off-diagonal part below 1e-17 |C| after four sweeps, the eigenpairs' residual within
the solver's stated allowance S = 128 units of 2^-53 |C| after six, and the eigenvectors those of numpy.linalg.eigh."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools_dev'))
import jacobi3_model as JM  # noqa: E402


def test_model_converges_in_four_sweeps_and_stays_within_the_allowance():
    names = []
    for name, C in JM.families(5000, seed=7):
        got = JM.measure(C, sweeps=6)
        print(name, got)
        assert len(got['offdiag_over_norm_per_sweep']) == 6 and max(got['offdiag_over_norm_per_sweep'][3:]) < 1e-17, name
        assert got['residual_units'] <= 128.0 and got['orthogonality'] <= 1e-14, name
        names.append(name)
    assert len(names) == 1 + len(JM.FAMILIES)


def test_model_finds_the_eigenvector_of_the_smallest_eigenvalue():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(2000, 3, 3))
    C = A @ A.transpose(0, 2, 1)
    w, V, _ = JM.jacobi(C)
    want_w, want_V = np.linalg.eigh(C)
    col = w.argmin(axis=1)
    got = V[np.arange(len(C)), :, col]
    gap = (want_w[:, 1] - want_w[:, 0]) / want_w[:, 2]
    sin = np.linalg.norm(np.cross(got, want_V[:, :, 0]), axis=1)
    assert np.abs(np.sort(w, axis=1) - want_w).max() <= 1e-13 * want_w.max()
    assert (sin[gap > 1e-6] <= 1e-9).all() and (gap > 1e-6).sum() > 1900
    # a diagonal matrix and the zero matrix are left as they are: every rotation is the identity
    w, V, off = JM.jacobi(np.array([np.diag([3.0, 1.0, 2.0]), np.zeros((3, 3))]))
    assert w.tolist() == [[3.0, 1.0, 2.0], [0.0, 0.0, 0.0]] and np.array_equal(V, np.tile(np.eye(3), (2, 1, 1))) and not off[-1].any()
