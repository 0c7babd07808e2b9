// A triangle mesh simplified by vertex clustering with quadric placement (gfx950): the clusters of the vertices, the clusters'
// quadrics, the representatives' positions, the rewritten faces (ops/mesh_simplify.py, atvsnet/simplify_mesh.py).
// include/atvsnet_hip.h has the definitions, tests/mesh_simplify_restated.py restates them, DESIGN.md section 10.3d has the arguments.
// Built with -ffp-contract=off: every operation below is rounded on its own.  Integer atomics only: which slot a cluster or a set
// of ids gets and who adds first depend on arrival order, no word that is written does.
//
//   cluster    atvs_cloud_voxel_downsample's table (cloud_voxel.h: the cell, the fraction, the slot) with six sums per slot instead of
//              three: insert (one lane per vertex: count, sums, the minimum of the first index), flag and cloud_scan.h's exclusive scan
//              (a cluster's id is the rank of its first vertex), emit (every vertex reads its cluster's id; the first vertex writes
//              the cluster's record).
//   quadrics   one lane per face: the face's plane in double, ten terms per distinct cluster among its three, each rounded to a
//              multiple of 2^-30 and added as a 64-bit integer.
//   place      one lane per cluster: the exact mean, then jacobi3.h's decomposition of the quadric and the minimiser on the eigenpairs
//              above the rank threshold; Lindstrom's fallbacks.
//   faces      an open-addressing table whose slot holds a FACE INDEX, all-ones-but-the-sign = empty.  A face claims a slot by a
//              32-bit compare-and-swap whose return value is the only read of the slot; an occupied slot's owner is compared by
//              recomputing its sorted triple from `faces` and `vertex_cluster` (read-only here); the same set lowers the slot with
//              atomicMin -- the owner only ever changes to a face of the same set, so the comparison does not depend on when it
//              is made, and a set's faces all end at the set's one slot (the first slot of their common probe sequence that was
//              empty when the set's first face came; nothing before it ever empties).  A second launch keeps face f iff its slot
//              holds f.  Every probe loop is bounded by the table; the load is at most 0.5.
#include <math.h>

#include "common.h"
#include "cloud_scan.h"
#include "cloud_voxel.h"
#include "jacobi3.h"

namespace {

constexpr long kMaxFaces = ATVS_MESH_TOPOLOGY_MAX_FACES;
constexpr long kClusterMinSlots = 1024;
constexpr size_t kClusterHeader = 256;
constexpr int kNoFace = 0x7fffffff;
constexpr int kMoveBlocks = 2048;
constexpr double kFix = 1073741824.0;                    // 2^30: the quadrics' fixed point
constexpr double kSliver = 1.0 / 1048576.0;              // 2^-20: lambda_max at or below it is a cluster of slivers only

// *word += the number of lanes of this wavefront with `flag`: one atomic per wavefront.  Called by every lane of the wavefront.
__device__ __forceinline__ void wave_tally(int* __restrict__ word, bool flag) {
  const unsigned long long mask = __ballot(flag);
  if (mask != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(word, __popcll(mask));
}

__device__ __forceinline__ bool in_range(int i, long n) { return i >= 0 && (long)i < n; }

// ---------------------------------------------------------------------------------------------------------------------- cluster

struct ClusterLayout {
  size_t keys, first, zero, sums, cnt, flags, slot, tiles, total;   // [header] 0, [keys | first] all-ones, [sums .. flags] 0
  long slots;
  int shift;                                                          // 64 - log2(slots)
};
inline ClusterLayout cluster_layout(long n) {
  ClusterLayout L;
  long slots = kClusterMinSlots;
  int lg = 10;
  while (slots < 2 * n) {
    slots <<= 1;
    ++lg;
  }
  L.slots = slots;
  L.shift = 64 - lg;
  L.keys = kClusterHeader;
  L.first = L.keys + align256((size_t)slots * 8);
  L.zero = L.first + align256((size_t)slots * 4);
  L.sums = L.zero;
  L.cnt = L.sums + align256((size_t)slots * 48);
  L.flags = L.cnt + align256((size_t)slots * 4);
  L.slot = L.flags + align256((size_t)(n + 1) * 4);
  L.tiles = L.slot + align256((size_t)n * 4);
  L.total = L.tiles + align256((size_t)scan_tiles(n + 1) * 4);
  return L;
}

__global__ __launch_bounds__(kThreads) void cluster_insert_kernel(const float* __restrict__ vertices, const unsigned char* __restrict__ colors,
                                                                  long n, VoxelArgs A, long slots, int shift,
                                                                  unsigned long long* __restrict__ keys, unsigned* __restrict__ first,
                                                                  unsigned long long* __restrict__ sums, unsigned* __restrict__ cnt,
                                                                  int* __restrict__ slot_of, int* __restrict__ err) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  unsigned long long u[3];
  const int s = voxel_slot_of(vertices, i, A, slots, shift, keys, err, u);
  if (s >= 0) {
    atomicAdd(cnt + s, 1u);
    atomicAdd(sums + (long)s * 6 + 0, u[0]);
    atomicAdd(sums + (long)s * 6 + 1, u[1]);
    atomicAdd(sums + (long)s * 6 + 2, u[2]);
    if (colors) {
      atomicAdd(sums + (long)s * 6 + 3, (unsigned long long)colors[i * 3 + 0]);
      atomicAdd(sums + (long)s * 6 + 4, (unsigned long long)colors[i * 3 + 1]);
      atomicAdd(sums + (long)s * 6 + 5, (unsigned long long)colors[i * 3 + 2]);
    }
    atomicMin(first + s, (unsigned)i);
  }
  slot_of[i] = s;
}

__global__ __launch_bounds__(kThreads) void cluster_flag_kernel(const int* __restrict__ slot_of, const unsigned* __restrict__ first, long n,
                                                                unsigned* __restrict__ flags) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int s = slot_of[i];
  flags[i] = (s >= 0 && first[s] == (unsigned)i) ? 1u : 0u;          // flags[n] stays 0: the scan's last word is C
}

__global__ __launch_bounds__(kThreads) void cluster_emit_kernel(const int* __restrict__ slot_of, long n, const unsigned long long* __restrict__ keys,
                                                                const unsigned* __restrict__ first, const unsigned long long* __restrict__ sums,
                                                                const unsigned* __restrict__ cnt, const unsigned* __restrict__ pos,
                                                                const int* __restrict__ err, int with_colors, int* __restrict__ vertex_cluster,
                                                                int* __restrict__ cells, int* __restrict__ counts,
                                                                unsigned long long* __restrict__ position_sums,
                                                                unsigned long long* __restrict__ color_sums, long long* __restrict__ count) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const bool bad = *err != 0;
  if (i == 0) *count = bad ? -1ll : (long long)pos[n];
  if (i >= n) return;
  const int s = slot_of[i];
  if (bad || s < 0) {
    vertex_cluster[i] = -1;
    return;
  }
  const unsigned head = first[s];                                     // < n: the minimum of indices below n
  vertex_cluster[i] = (int)pos[head];
  if (head != (unsigned)i) return;
  const unsigned p = pos[i];
  if ((long)p >= n) return;                                           // never: at most n flags
  const unsigned long long key = keys[s];
  counts[p] = (int)cnt[s];
  for (int a = 0; a < 3; ++a) {
    cells[(long)p * 3 + a] = (int)((key >> (21 * a)) & 0x1fffffull);
    position_sums[(long)p * 3 + a] = sums[(long)s * 6 + a];
    if (with_colors) color_sums[(long)p * 3 + a] = sums[(long)s * 6 + 3 + a];
  }
}

// --------------------------------------------------------------------------------------------------------------------- quadrics

__device__ __forceinline__ void add_fixed(long long* __restrict__ word, double term) {
  const long long q = (long long)rint(term * kFix);                   // |term| <= 1: |q| <= 2^30
  atomicAdd(reinterpret_cast<unsigned long long*>(word), (unsigned long long)q);          // two's complement: the signed sum
}

__global__ __launch_bounds__(kThreads) void cluster_quadrics_kernel(const float* __restrict__ vertices, long n_vertices,
                                                                    const int* __restrict__ faces, long n_faces,
                                                                    const int* __restrict__ vertex_cluster, long n_clusters, VoxelArgs A,
                                                                    long long* __restrict__ quadrics, int* __restrict__ incidences,
                                                                    int* __restrict__ info) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  bool bad = false;
  if (f < n_faces) {
    const int i[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
    bad = !in_range(i[0], n_vertices) | !in_range(i[1], n_vertices) | !in_range(i[2], n_vertices);
    if (!bad) {
      const int k[3] = {vertex_cluster[i[0]], vertex_cluster[i[1]], vertex_cluster[i[2]]};
      bad = (k[0] < -1) | (k[1] < -1) | (k[2] < -1) | ((long)k[0] >= n_clusters) | ((long)k[1] >= n_clusters) | ((long)k[2] >= n_clusters);
      if (!bad && k[0] >= 0 && k[1] >= 0 && k[2] >= 0) {
        double x[3][3];
        for (int j = 0; j < 3; ++j)
          for (int a = 0; a < 3; ++a) x[j][a] = (double)vertices[(long)i[j] * 3 + a];
        const double e0 = x[1][0] - x[0][0], e1 = x[1][1] - x[0][1], e2 = x[1][2] - x[0][2];
        const double h0 = x[2][0] - x[0][0], h1 = x[2][1] - x[0][1], h2 = x[2][2] - x[0][2];
        const double m0 = e1 * h2 - e2 * h1, m1 = e2 * h0 - e0 * h2, m2 = e0 * h1 - e1 * h0;
        const double L2 = (m0 * m0 + m1 * m1) + m2 * m2;
        if (L2 > 0.0 && finite_d(L2)) {
          const double r = sqrt(L2);
          const double n0 = m0 / r, n1 = m1 / r, n2 = m2 / r;
          const double ratio = r / (A.voxel * A.voxel);
          const double w = ratio < 1.0 ? ratio : 1.0;
          for (int j = 0; j < 3; ++j) {
            if ((j > 0 && k[j] == k[0]) || (j > 1 && k[j] == k[1])) continue;              // an earlier vertex lies in this cluster
            double p[3];
            for (int a = 0; a < 3; ++a) {
              const double g = (x[j][a] - A.origin[a]) / A.voxel;
              p[a] = (g - floor(g)) - 0.5;
            }
            const double d = -((n0 * p[0] + n1 * p[1]) + n2 * p[2]);
            const double w0 = w * n0, w1 = w * n1, w2 = w * n2, wd = w * d;
            long long* q = quadrics + (long)k[j] * 10;
            add_fixed(q + 0, w0 * n0);
            add_fixed(q + 1, w0 * n1);
            add_fixed(q + 2, w0 * n2);
            add_fixed(q + 3, w1 * n1);
            add_fixed(q + 4, w1 * n2);
            add_fixed(q + 5, w2 * n2);
            add_fixed(q + 6, wd * n0);
            add_fixed(q + 7, wd * n1);
            add_fixed(q + 8, wd * n2);
            add_fixed(q + 9, wd * d);
            atomicAdd(incidences + k[j], 1);
          }
        }
      }
    }
  }
  wave_tally(info, bad);
}

// ------------------------------------------------------------------------------------------------------------------------ place

__global__ __launch_bounds__(kThreads) void cluster_place_kernel(const int* __restrict__ cells, const int* __restrict__ counts,
                                                                 const unsigned long long* __restrict__ position_sums,
                                                                 const unsigned long long* __restrict__ color_sums,
                                                                 const long long* __restrict__ quadrics, long n_clusters, VoxelArgs A,
                                                                 int placement, double rank_epsilon, float* __restrict__ positions,
                                                                 unsigned char* __restrict__ colors_out, unsigned char* __restrict__ placed) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_clusters) return;
  const int count = counts[j];
  const double k = (double)(count > 0 ? count : 1);
  const double x00 = ((double)position_sums[j * 3 + 0] / k) / 4294967296.0 - 0.5;
  const double x01 = ((double)position_sums[j * 3 + 1] / k) / 4294967296.0 - 0.5;
  const double x02 = ((double)position_sums[j * 3 + 2] / k) / 4294967296.0 - 0.5;
  double x0 = x00, x1 = x01, x2 = x02;
  bool use = false;
  if (placement == ATVS_MESH_PLACE_QUADRIC) {
    const double scale = 1.0 / kFix;
    const long long* q = quadrics + j * 10;
    const double A00 = (double)q[0] * scale, A01 = (double)q[1] * scale, A02 = (double)q[2] * scale;
    const double A11 = (double)q[3] * scale, A12 = (double)q[4] * scale, A22 = (double)q[5] * scale;
    const double b0 = (double)q[6] * scale, b1 = (double)q[7] * scale, b2 = (double)q[8] * scale;
    double a00 = A00, a01 = A01, a02 = A02, a11 = A11, a12 = A12, a22 = A22;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    jacobi3(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    double lmax = a00;
    lmax = a11 > lmax ? a11 : lmax;
    lmax = a22 > lmax ? a22 : lmax;
    const double thr = rank_epsilon * lmax;
    const double g0 = ((A00 * x00 + A01 * x01) + A02 * x02) + b0;
    const double g1 = ((A01 * x00 + A11 * x01) + A12 * x02) + b1;
    const double g2 = ((A02 * x00 + A12 * x01) + A22 * x02) + b2;
    if (a00 > thr) {
      const double t = ((v00 * g0 + v10 * g1) + v20 * g2) / a00;
      x0 = x0 - v00 * t; x1 = x1 - v10 * t; x2 = x2 - v20 * t;
    }
    if (a11 > thr) {
      const double t = ((v01 * g0 + v11 * g1) + v21 * g2) / a11;
      x0 = x0 - v01 * t; x1 = x1 - v11 * t; x2 = x2 - v21 * t;
    }
    if (a22 > thr) {
      const double t = ((v02 * g0 + v12 * g1) + v22 * g2) / a22;
      x0 = x0 - v02 * t; x1 = x1 - v12 * t; x2 = x2 - v22 * t;
    }
    // bitwise, not short-circuit: see the note on the sign predicate in cloud_normals.hip
    use = finite_d(lmax) & (lmax > kSliver) & finite_d(x0) & finite_d(x1) & finite_d(x2) & (fabs(x0) <= 0.5) & (fabs(x1) <= 0.5) &
          (fabs(x2) <= 0.5);
  }
  const double y0 = use ? x0 : x00, y1 = use ? x1 : x01, y2 = use ? x2 : x02;
  positions[j * 3 + 0] = (float)(A.origin[0] + A.voxel * (((double)cells[j * 3 + 0] + 0.5) + y0));
  positions[j * 3 + 1] = (float)(A.origin[1] + A.voxel * (((double)cells[j * 3 + 1] + 0.5) + y1));
  positions[j * 3 + 2] = (float)(A.origin[2] + A.voxel * (((double)cells[j * 3 + 2] + 0.5) + y2));
  placed[j] = use ? 1 : 0;
  if (color_sums) {
    const unsigned long long kk = (unsigned long long)(count > 0 ? count : 1);
    for (int a = 0; a < 3; ++a) colors_out[j * 3 + a] = (unsigned char)((2ull * color_sums[j * 3 + a] + kk) / (2ull * kk));
  }
}

__global__ __launch_bounds__(kThreads) void cluster_max_move_kernel(const float* __restrict__ vertices, long n,
                                                                    const int* __restrict__ vertex_cluster, const float* __restrict__ positions,
                                                                    long n_clusters, unsigned* __restrict__ out) {
  unsigned m = 0u;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const int c = vertex_cluster[i];
    if (c < 0 || (long)c >= n_clusters) continue;
    const double e0 = (double)positions[(long)c * 3 + 0] - (double)vertices[i * 3 + 0];
    const double e1 = (double)positions[(long)c * 3 + 1] - (double)vertices[i * 3 + 1];
    const double e2 = (double)positions[(long)c * 3 + 2] - (double)vertices[i * 3 + 2];
    const float d = (float)((e0 * e0 + e1 * e1) + e2 * e2);
    if (d >= 0.0f) m = max(m, __float_as_uint(d));                   // a non-negative float's bits order as its value; NaN is left out
  }
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// ------------------------------------------------------------------------------------------------------------------------ faces

__device__ __forceinline__ void sort3(int& a, int& b, int& c) {
  int t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {      // the finaliser of MurmurHash3
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

inline unsigned long long faces_slots(long n_faces) {
  unsigned long long s = ATVS_MESH_SIMPLIFY_MIN_SLOTS;
  while (s < 2ull * (unsigned long long)n_faces) s <<= 1;
  return s;
}

struct FacesLayout {
  size_t table, slot, total;
};
inline FacesLayout faces_layout(long n_faces) {
  FacesLayout L;
  L.table = 0;
  L.slot = L.table + align256((size_t)faces_slots(n_faces) * sizeof(int));
  L.total = L.slot + align256((size_t)n_faces * sizeof(int));
  return L;
}

// info: [0] bad index or no slot, [1] non-finite, [2] degenerate.  slot_of[f] = the slot of the face's set, -1 for a face that is dropped here.
__global__ __launch_bounds__(kThreads) void cluster_faces_insert_kernel(const int* __restrict__ faces, long n_faces, long n_vertices,
                                                                        const int* __restrict__ vertex_cluster, int* __restrict__ table,
                                                                        unsigned long long slots, int* __restrict__ slot_of,
                                                                        int* __restrict__ faces_out, unsigned char* __restrict__ keep,
                                                                        int* __restrict__ info) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  bool bad = false, nonfinite = false, degenerate = false;
  if (f < n_faces) {
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    int k0 = -1, k1 = -1, k2 = -1, slot = -1;
    bad = !in_range(i0, n_vertices) | !in_range(i1, n_vertices) | !in_range(i2, n_vertices);
    if (!bad) {
      k0 = vertex_cluster[i0];
      k1 = vertex_cluster[i1];
      k2 = vertex_cluster[i2];
      nonfinite = (k0 < 0) | (k1 < 0) | (k2 < 0);
      degenerate = !nonfinite & ((k0 == k1) | (k1 == k2) | (k0 == k2));
      if (!nonfinite && !degenerate) {
        int a = k0, b = k1, c = k2;
        sort3(a, b, c);
        const unsigned long long mask = slots - 1ull;
        unsigned long long h = mix64(mix64(((unsigned long long)(unsigned)a << 32) | (unsigned long long)(unsigned)b) + (unsigned long long)(unsigned)c) & mask;
        for (unsigned long long probe = 0; probe < slots; ++probe) {          // bounded: at load <= 0.5 an empty slot always exists
          const int old = atomicCAS(table + h, kNoFace, (int)f);
          if (old == kNoFace) {
            slot = (int)h;
            break;
          }
          // the owner: a face below n_faces that passed the checks above (only such faces are stored)
          int oa = vertex_cluster[faces[(long)old * 3 + 0]], ob = vertex_cluster[faces[(long)old * 3 + 1]],
              oc = vertex_cluster[faces[(long)old * 3 + 2]];
          sort3(oa, ob, oc);
          if (oa == a && ob == b && oc == c) {
            atomicMin(table + h, (int)f);
            slot = (int)h;
            break;
          }
          h = (h + 1ull) & mask;
        }
        if (slot < 0) bad = true;
      }
    }
    faces_out[f * 3 + 0] = bad ? -1 : k0;
    faces_out[f * 3 + 1] = bad ? -1 : k1;
    faces_out[f * 3 + 2] = bad ? -1 : k2;
    slot_of[f] = slot;
    if (slot < 0) keep[f] = 0;
  }
  wave_tally(info + 0, bad);
  wave_tally(info + 1, nonfinite);
  wave_tally(info + 2, degenerate);
}

__global__ __launch_bounds__(kThreads) void cluster_faces_keep_kernel(const int* __restrict__ table, const int* __restrict__ slot_of, long n_faces,
                                                                      unsigned char* __restrict__ keep, int* __restrict__ info) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  bool duplicate = false;
  if (f < n_faces) {
    const int slot = slot_of[f];
    if (slot >= 0) {
      duplicate = table[slot] != (int)f;
      keep[f] = duplicate ? 0 : 1;
    }
  }
  wave_tally(info + 3, duplicate);
}

inline bool counts_ok(long n_vertices, long n_faces) {
  return n_vertices >= 0 && n_vertices <= kMaxPoints && n_faces >= 0 && n_faces <= kMaxFaces;
}

}  // namespace

extern "C" int atvs_mesh_cluster_scratch_size(long n_vertices, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n_vertices < 0 || n_vertices > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)cluster_layout(n_vertices).total;
  return ATVS_OK;
}

extern "C" int atvs_mesh_cluster(const float* vertices, const void* colors, long n_vertices, double cell, const double* origin, void* scratch,
                                 long scratch_bytes, int* vertex_cluster, int* cells, int* counts, long* position_sums, long* color_sums,
                                 long* count, atvs_stream_t stream) {
  const long n = n_vertices;
  if (n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!origin || !count ||
      (n > 0 && (!vertices || !scratch || !vertex_cluster || !cells || !counts || !position_sums || (colors && !color_sums))))
    return ATVS_ERR_NULL;
  VoxelArgs A;
  if (!voxel_args(cell, origin, &A)) return ATVS_ERR_ARG;
  hipStream_t st = as_stream(stream);
  if (n == 0) return hipMemsetAsync(count, 0, sizeof(long long), st) == hipSuccess ? ATVS_OK : ATVS_ERR_LAUNCH;
  const ClusterLayout L = cluster_layout(n);
  if (scratch_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  char* s = static_cast<char*>(scratch);
  int* err = reinterpret_cast<int*>(s);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(s + L.keys);
  unsigned* first = reinterpret_cast<unsigned*>(s + L.first);
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(s + L.sums);
  unsigned* cnt = reinterpret_cast<unsigned*>(s + L.cnt);
  unsigned* flags = reinterpret_cast<unsigned*>(s + L.flags);
  int* slot_of = reinterpret_cast<int*>(s + L.slot);
  if (hipMemsetAsync(s, 0, kClusterHeader, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(s + L.keys, 0xff, L.zero - L.keys, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(s + L.zero, 0, L.slot - L.zero, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  const dim3 per_vertex((unsigned)cdiv(n, kThreads));
  hipLaunchKernelGGL(cluster_insert_kernel, per_vertex, dim3(kThreads), 0, st, vertices, static_cast<const unsigned char*>(colors), n, A,
                     L.slots, L.shift, keys, first, sums, cnt, slot_of, err);
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cluster_flag_kernel, per_vertex, dim3(kThreads), 0, st, (const int*)slot_of, (const unsigned*)first, n, flags);
  ATVS_LAUNCH_CHECK();
  const int rc = exclusive_scan(flags, n + 1, reinterpret_cast<unsigned*>(s + L.tiles), st);
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(cluster_emit_kernel, per_vertex, dim3(kThreads), 0, st, (const int*)slot_of, n, (const unsigned long long*)keys,
                     (const unsigned*)first, (const unsigned long long*)sums, (const unsigned*)cnt, (const unsigned*)flags, (const int*)err,
                     colors ? 1 : 0, vertex_cluster, cells, counts, reinterpret_cast<unsigned long long*>(position_sums),
                     reinterpret_cast<unsigned long long*>(color_sums), reinterpret_cast<long long*>(count));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_cluster_quadrics(const float* vertices, long n_vertices, const int* faces, long n_faces, const int* vertex_cluster,
                                          long n_clusters, double cell, const double* origin, long* quadrics, int* incidences, int* info,
                                          atvs_stream_t stream) {
  if (!counts_ok(n_vertices, n_faces) || n_clusters < 0 || n_clusters > n_vertices) return ATVS_ERR_SHAPE;
  if (!origin || !info || (n_clusters > 0 && (!quadrics || !incidences)) || (n_faces > 0 && (!faces || !vertices || !vertex_cluster)))
    return ATVS_ERR_NULL;
  VoxelArgs A;
  if (!voxel_args(cell, origin, &A)) return ATVS_ERR_ARG;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(info, 0, sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_clusters > 0) {
    if (hipMemsetAsync(quadrics, 0, (size_t)n_clusters * 10 * sizeof(long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
    if (hipMemsetAsync(incidences, 0, (size_t)n_clusters * sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  }
  if (n_faces == 0) return ATVS_OK;
  hipLaunchKernelGGL(cluster_quadrics_kernel, dim3((unsigned)cdiv(n_faces, kThreads)), dim3(kThreads), 0, st, vertices, n_vertices, faces,
                     n_faces, vertex_cluster, n_clusters, A, reinterpret_cast<long long*>(quadrics), incidences, info);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_cluster_place(const int* cells, const int* counts, const long* position_sums, const long* color_sums,
                                       const long* quadrics, long n_clusters, double cell, const double* origin, int placement,
                                       double rank_epsilon, float* positions, void* colors_out, void* placed, atvs_stream_t stream) {
  if (n_clusters < 0 || n_clusters > kMaxPoints) return ATVS_ERR_SHAPE;
  if (placement != ATVS_MESH_PLACE_MEAN && placement != ATVS_MESH_PLACE_QUADRIC) return ATVS_ERR_ARG;
  if (!(rank_epsilon > 0.0 && rank_epsilon < 1.0)) return ATVS_ERR_ARG;
  if (!origin || (n_clusters > 0 && (!cells || !counts || !position_sums || !positions || !placed || (color_sums && !colors_out) ||
                                     (placement == ATVS_MESH_PLACE_QUADRIC && !quadrics))))
    return ATVS_ERR_NULL;
  VoxelArgs A;
  if (!voxel_args(cell, origin, &A)) return ATVS_ERR_ARG;
  if (n_clusters == 0) return ATVS_OK;
  hipLaunchKernelGGL(cluster_place_kernel, dim3((unsigned)cdiv(n_clusters, kThreads)), dim3(kThreads), 0, as_stream(stream), cells, counts,
                     reinterpret_cast<const unsigned long long*>(position_sums), reinterpret_cast<const unsigned long long*>(color_sums),
                     reinterpret_cast<const long long*>(quadrics), n_clusters, A, placement, rank_epsilon, positions,
                     static_cast<unsigned char*>(colors_out), static_cast<unsigned char*>(placed));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_cluster_max_move(const float* vertices, long n_vertices, const int* vertex_cluster, const float* positions,
                                          long n_clusters, void* out, atvs_stream_t stream) {
  if (n_vertices < 0 || n_vertices > kMaxPoints || n_clusters < 0 || n_clusters > n_vertices) return ATVS_ERR_SHAPE;
  if (!out || (n_vertices > 0 && (!vertices || !vertex_cluster)) || (n_clusters > 0 && !positions)) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(out, 0, sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_vertices == 0 || n_clusters == 0) return ATVS_OK;
  const int blocks = cdiv(n_vertices, kThreads) < kMoveBlocks ? cdiv(n_vertices, kThreads) : kMoveBlocks;
  hipLaunchKernelGGL(cluster_max_move_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, vertices, n_vertices, vertex_cluster, positions,
                     n_clusters, static_cast<unsigned*>(out));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_cluster_faces_scratch_size(long n_faces, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n_faces < 0 || n_faces > kMaxFaces) return ATVS_ERR_SHAPE;
  *bytes = (long)faces_layout(n_faces).total;
  return ATVS_OK;
}

extern "C" int atvs_mesh_cluster_faces(const int* faces, long n_faces, long n_vertices, const int* vertex_cluster, void* scratch,
                                       long scratch_bytes, int* faces_out, void* keep, int* info, atvs_stream_t stream) {
  if (!counts_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  if (!info || !scratch || (n_faces > 0 && (!faces || !vertex_cluster || !faces_out || !keep))) return ATVS_ERR_NULL;
  const FacesLayout L = faces_layout(n_faces);
  if (scratch_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(info, 0, 4 * sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_faces == 0) return ATVS_OK;
  const unsigned long long slots = faces_slots(n_faces);
  char* base = static_cast<char*>(scratch);
  int* table = reinterpret_cast<int*>(base + L.table);
  int* slot_of = reinterpret_cast<int*>(base + L.slot);
  // kNoFace = 0x7fffffff is not a byte pattern: the table is filled by the 32-bit form of the memset
  if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(table), kNoFace, (size_t)slots, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  const dim3 per_face((unsigned)cdiv(n_faces, kThreads));
  hipLaunchKernelGGL(cluster_faces_insert_kernel, per_face, dim3(kThreads), 0, st, faces, n_faces, n_vertices, vertex_cluster, table, slots,
                     slot_of, faces_out, static_cast<unsigned char*>(keep), info);
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cluster_faces_keep_kernel, per_face, dim3(kThreads), 0, st, (const int*)table, (const int*)slot_of, n_faces,
                     static_cast<unsigned char*>(keep), info);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
