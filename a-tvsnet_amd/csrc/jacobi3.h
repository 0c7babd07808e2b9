// The fixed eigen-solver of a symmetric 3 x 3 matrix in double, ONE definition for cloud_normals.hip (the direction of least variance)
// and mesh_simplify.hip (the minimiser of a cluster's quadric): cyclic Jacobi, kSweeps = 6 sweeps of the three rotations (0,1), (0,2),
// (1,2), 18 rotations, always all of them.  The matrix and the accumulated rotations live in fifteen named doubles; nothing is indexed
// at run time, no trip count depends on the data.  A rotation of the pair (p, q) with the third index r:
//     theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrt(theta theta + 1))   (t = 0 where a_pq == 0)
//     c = 1 / sqrt(t t + 1);  s = t c
//     a_pp -= t a_pq;  a_qq += t a_pq;  a_pq = 0;  (a_pr, a_qr) = (c a_pr - s a_qr, s a_pr + c a_qr)
//     (v_kp, v_kq) = (c v_kp - s v_kq, s v_kp + c v_kq)   for k = 0, 1, 2
// theta theta overflows to +inf for a tiny a_pq, which gives t = +-0: the rotation it should be.  At most 7 roundings reach an entry
// per rotation, so the 18 rotations commit a backward error of at most S = 18 x 7 = 126 < 128 units of 2^-53 |A| (an allowance
// from the operation count; the header states S = 128).  Six sweeps: a 3 x 3 cyclic Jacobi iteration converges quadratically once
// the off-diagonal part is small; in the numpy model of these operations (tools_dev/jacobi3_model.py, tests/test_jacobi3_model.py)
// the off-diagonal part is below 1e-17 |A| after FOUR sweeps on every matrix tried, so two sweeps are margin.
// Built with -ffp-contract=off: every operation is rounded on its own.
#pragma once
#include <math.h>

#include "common.h"

namespace {

constexpr int kSweeps = 6;

// One Jacobi rotation of the pair (p, q); r is the third index.  All arguments are named registers.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q) {
  const double theta = (aqq - app) / (2.0 * apq);
  const double mag = fabs(theta) + sqrt(theta * theta + 1.0);
  const double t = apq == 0.0 ? 0.0 : (theta < 0.0 ? -1.0 / mag : 1.0 / mag);
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  const double pr = c * apr - s * aqr, qr = s * apr + c * aqr;
  apr = pr;
  aqr = qr;
  const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
  const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
  const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
  v0p = a0; v0q = b0;
  v1p = a1; v1q = b1;
  v2p = a2; v2q = b2;
}

// The matrix (its upper triangle) -> its eigenvalues on the diagonal a00, a11, a22 in no particular order, eigenvector i in column i
// (v0i, v1i, v2i).  The caller starts v at the identity.
__device__ __forceinline__ void jacobi3(double& a00, double& a01, double& a02, double& a11, double& a12, double& a22, double& v00,
                                        double& v01, double& v02, double& v10, double& v11, double& v12, double& v20, double& v21,
                                        double& v22) {
#pragma unroll
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < (double)__uint_as_float(0x7f800000u); }

}  // namespace
