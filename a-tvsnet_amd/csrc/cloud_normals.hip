// Normals of an arbitrary cloud (gfx950): per query the direction of least variance of the neighbours atvs_cloud_knn found
// (ops/cloud.py cloud_normals, atvsnet/register_cloud.py normal_side='target', atvsnet/cloud_normals.py).  The definition is in
// include/atvsnet_hip.h; tests/cloud_normals_restated.py restates it with math.fsum and numpy.linalg.eigh.  Built with
// -ffp-contract=off: every operation below is rounded on its own.  No atomics; a row's output depends on that row's inputs alone.
//
// ONE LANE PER QUERY.  A lane reads its own row of idx (k consecutive ints) and gathers k x 12 bytes; nine double accumulators
// (s, and the six sums of products) take the samples in ascending t.  The samples are differences to the query, so every term is of
// the neighbourhood's own size and the one-pass covariance S_ab - s_a s_b / c does not cancel however far the cloud is from the origin.
//
// THE SOLVER (jacobi3.h, shared with mesh_simplify.hip; the same operations in the same order as when it stood here): cyclic
// Jacobi, kSweeps = 6 sweeps of the three rotations (0,1), (0,2), (1,2), 18 rotations, always all of them.  The
// matrix and the accumulated rotations live in fifteen named doubles; nothing is indexed at run time, no trip count depends on the
// data.  A rotation of the pair (p, q) with the third index r:
//     theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrt(theta theta + 1))   (t = 0 where a_pq == 0)
//     c = 1 / sqrt(t t + 1);  s = t c
//     a_pp -= t a_pq;  a_qq += t a_pq;  a_pq = 0;  (a_pr, a_qr) = (c a_pr - s a_qr, s a_pr + c a_qr)
//     (v_kp, v_kq) = (c v_kp - s v_kq, s v_kp + c v_kq)   for k = 0, 1, 2
// theta theta overflows to +inf for a tiny a_pq, which gives t = +-0: the rotation it should be.  At most 7 roundings reach an entry
// per rotation, so the 18 rotations commit a backward error of at most S = 18 x 7 = 126 < 128 units of 2^-53 |C| (an allowance
// from the operation count; the header states S = 128).  Six sweeps: a 3 x 3 cyclic Jacobi iteration converges quadratically once
// the off-diagonal part is small; in the numpy model of these operations (tools_dev/jacobi3_model.py, tests/test_jacobi3_model.py)
// the off-diagonal part is below 1e-17 |C| after FOUR sweeps on every matrix tried, so two sweeps are margin.
#include <math.h>

#include "common.h"
#include "cloud_common.h"
#include "jacobi3.h"

namespace {

constexpr int kMaxK = ATVS_CLOUD_MAX_K;
constexpr double kRankRatio = 1e-12;                     // lambda_1 <= kRankRatio lambda_2: fewer than two directions

__global__ __launch_bounds__(kThreads) void cloud_normals_kernel(const float* __restrict__ points, long n, const float* __restrict__ queries,
                                                                 long m, const int* __restrict__ idx, int k, int self_counts,
                                                                 const double* __restrict__ viewpoints, int n_viewpoints,
                                                                 const int* __restrict__ view_of, float* __restrict__ normals,
                                                                 float* __restrict__ variation) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const float qxf = queries[j * 3 + 0], qyf = queries[j * 3 + 1], qzf = queries[j * 3 + 2];
  const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
  bool ok = finite3(qxf, qyf, qzf);
  const int* __restrict__ row = idx + j * k;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  int count = self_counts ? 1 : 0;
#pragma unroll 4
  for (int t = 0; t < k; ++t) {
    const int i = row[t];
    if (i < 0) continue;
    if ((long)i >= n) {                                    // never read: the row has no normal
      ok = false;
      continue;
    }
    const float px = points[(long)i * 3 + 0], py = points[(long)i * 3 + 1], pz = points[(long)i * 3 + 2];
    ok = ok && finite3(px, py, pz);
    const double d0 = (double)px - qx, d1 = (double)py - qy, d2 = (double)pz - qz;
    count += 1;
    s0 = s0 + d0; s1 = s1 + d1; s2 = s2 + d2;
    xx = xx + d0 * d0; xy = xy + d0 * d1; xz = xz + d0 * d2;
    yy = yy + d1 * d1; yz = yz + d1 * d2; zz = zz + d2 * d2;
  }
  ok = ok && count >= 3;
  const double c = (double)(count > 0 ? count : 1);
  double a00 = xx - (s0 * s0) / c, a01 = xy - (s0 * s1) / c, a02 = xz - (s0 * s2) / c;
  double a11 = yy - (s1 * s1) / c, a12 = yz - (s1 * s2) / c, a22 = zz - (s2 * s2) / c;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  jacobi3(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
  // the smallest eigenvalue's column, the lowest index on ties; the other two in order
  const bool first = a00 <= a11 && a00 <= a22, second = !first && a11 <= a22;
  const double l0 = first ? a00 : (second ? a11 : a22);
  double n0 = first ? v00 : (second ? v01 : v02), n1 = first ? v10 : (second ? v11 : v12), n2 = first ? v20 : (second ? v21 : v22);
  const double u = first ? a11 : a00, w = first || second ? a22 : a11;          // the two that are left
  const double l1 = u <= w ? u : w, l2 = u <= w ? w : u;
  ok = ok && finite_d(l0) && finite_d(l2) && l1 > kRankRatio * l2;
  // the sign: towards the row's viewpoint; the canonical one where there is none, or the normal is perpendicular to its direction
  const int view = view_of ? view_of[j] : 0;
  double dot = 0.0;
  if (viewpoints && view >= 0 && view < n_viewpoints) {
    const double e0 = viewpoints[(long)view * 3 + 0] - qx, e1 = viewpoints[(long)view * 3 + 1] - qy, e2 = viewpoints[(long)view * 3 + 2] - qz;
    dot = (n0 * e0 + n1 * e1) + n2 * e2;
  }
  const double m0 = fabs(n0), m1 = fabs(n1), m2 = fabs(n2);
  const double lead = m0 >= m1 && m0 >= m2 ? n0 : (m1 >= m2 ? n1 : n2);
  // Applied as an exact product with +-1.  The first draft had the SHORT-CIRCUIT predicate `dot < 0.0 || (!(dot > 0.0) && lead < 0.0)`
  // and `if (flip) n = -n`; its code object gave rows with dot == 0 and lead < 0 the unflipped normal (the source, the compiler's
  // version and the instructions are in tools_dev/experiments/cloud_normals_sign_branch.patch and the README beside it).  The
  // bitwise predicate below compiles correctly with either way of applying it; tests/test_gpu_cloud_normals.py holds every row's sign.
  const bool flip = (dot < 0.0) | (!(dot > 0.0) & (lead < 0.0));
  const double sign = flip ? -1.0 : 1.0;
  n0 = n0 * sign;
  n1 = n1 * sign;
  n2 = n2 * sign;
  normals[j * 3 + 0] = ok ? (float)n0 : 0.0f;
  normals[j * 3 + 1] = ok ? (float)n1 : 0.0f;
  normals[j * 3 + 2] = ok ? (float)n2 : 0.0f;
  if (variation) variation[j] = ok ? (float)(l0 / ((l0 + l1) + l2)) : __uint_as_float(0x7fc00000u);
}

}  // namespace

extern "C" int atvs_cloud_normals(const float* points, long n, const float* queries, long m, const int* idx, int k, int self_counts,
                                  const double* viewpoints, int n_viewpoints, const int* view_of, float* normals, float* variation,
                                  atvs_stream_t stream) {
  if (n < 0 || n > kMaxPoints || m < 0 || m > kMaxPoints || k < 1 || k > kMaxK || n_viewpoints < 0) return ATVS_ERR_SHAPE;
  if (self_counts != 0 && self_counts != 1) return ATVS_ERR_ARG;
  if ((n_viewpoints > 0) != (viewpoints != nullptr) || (view_of && !viewpoints)) return ATVS_ERR_ARG;
  if (m == 0) return ATVS_OK;
  if (!queries || !idx || !normals || (n > 0 && !points)) return ATVS_ERR_NULL;
  hipLaunchKernelGGL(cloud_normals_kernel, dim3((unsigned)cdiv(m, kThreads)), dim3(kThreads), 0, as_stream(stream), points, n, queries, m,
                     idx, k, self_counts, viewpoints, n_viewpoints, view_of, normals, variation);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
