// A triangle mesh smoothed by Taubin's filter and its vertex normals (gfx950): the distinct neighbours of every vertex as an inverted
// index, positions as integers on a power-of-two lattice, one umbrella step as a per-vertex gather, the way back to float32, the
// faces' extents and the area-weighted vertex normals (ops/mesh_smooth.py, atvsnet/smooth_mesh.py).  include/atvsnet_hip.h has the
// definitions, tests/mesh_smooth_restated.py restates them, DESIGN.md section 10.3g has the arguments.  Built with
// -ffp-contract=off: every operation below is rounded on its own.  Integer atomics only: every output is a function of the inputs,
// except the order of a vertex's row of `neighbours`, which nothing that is computed from it can show (integer sums).
//
//   adjacency  vertex_init: flags = finite, degree = 0.  insert: one lane per face, its three pairs sorted and put into an
//              open-addressing table of 64-bit keys (lo << 32) | hi exactly as mesh_topology.hip's census does (all-ones = empty, the
//              atomicCAS's return value is the only read of a slot, the probe loop bounded by the table), one 32-bit counter of faces
//              per slot.  pairs: a walk over the table adds 1 to both endpoints' degree, ors the boundary / non-manifold bits into
//              their flags and reduces the three tallies per workgroup.  offsets: a copy of degree with a zero behind, scanned by
//              cloud_scan.h.  scatter: a second walk; an endpoint's position is offsets[v] + its cursor's atomicAdd.
//   quantize, smooth_pass, dequantize, vertex_normals   one lane per vertex.  The pass loads three 8-byte words per neighbour.
//   face_extent       one lane per face by stride, the tallies and the maximum reduced per workgroup, one atomic each.
//   vertex_normal_sums  one lane per face: nine 64-bit and three 32-bit integer atomic adds.
#include <math.h>

#include "common.h"
#include "cloud_scan.h"

namespace {

constexpr long kMaxFaces = ATVS_MESH_TOPOLOGY_MAX_FACES;
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kWalkBlocks = 2048;                                  // workgroups of a walk over the table or the faces: 8 per CU
constexpr long long kClamp = 1ll << 32;                            // |q| after a pass
constexpr double kTwoTo30 = 1073741824.0;
constexpr double kTwoTo31 = 2147483648.0;
constexpr double kTwoTo62 = 4611686018427387904.0;

__device__ __forceinline__ bool in_range(int i, long n) { return i >= 0 && (long)i < n; }
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < (double)INFINITY; }

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {      // the finaliser of MurmurHash3, as the census
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
  return v;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long y = (unsigned long long)__shfl_xor((long long)v, off);
    v = y > v ? y : v;
  }
  return v;
}

// ------------------------------------------------------------------------------------------------------------------- adjacency

__global__ __launch_bounds__(kThreads) void adjacency_init_kernel(const float* __restrict__ vertices, long n_vertices,
                                                                  int* __restrict__ degree, int* __restrict__ flags) {
  const long v = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (v >= n_vertices) return;
  degree[v] = 0;
  flags[v] = finite3(vertices[v * 3 + 0], vertices[v * 3 + 1], vertices[v * 3 + 2]) ? 1 : 0;
}

// info: [3] faces with an index out of range, [4] self pairs, [5] pairs of a non-finite vertex, [6] pairs that found no slot.
__global__ __launch_bounds__(kThreads) void adjacency_insert_kernel(const int* __restrict__ faces, long n_faces, long n_vertices,
                                                                    const int* __restrict__ flags, unsigned long long* __restrict__ keys,
                                                                    unsigned* __restrict__ counts, unsigned long long slots,
                                                                    unsigned long long* __restrict__ info) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (f >= n_faces) return;
  const int i[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
  if (!in_range(i[0], n_vertices) || !in_range(i[1], n_vertices) || !in_range(i[2], n_vertices)) {
    atomicAdd(info + 3, 1ull);
    return;
  }
  const unsigned long long mask = slots - 1ull;
  for (int e = 0; e < 3; ++e) {
    const unsigned a = (unsigned)i[e], b = (unsigned)i[e == 2 ? 0 : e + 1];
    if (a == b) {
      atomicAdd(info + 4, 1ull);
      continue;
    }
    if (!(flags[a] & 1) || !(flags[b] & 1)) {
      atomicAdd(info + 5, 1ull);
      continue;
    }
    const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
    const unsigned long long key = ((unsigned long long)lo << 32) | (unsigned long long)hi;   // never all-ones: hi < 2^30
    const unsigned long long start = mix64(key);
    bool placed = false;
    for (unsigned long long n = 0; n < slots; ++n) {          // bounded: at load <= 0.5 an empty slot always exists
      const unsigned long long slot = (start + n) & mask;
      const unsigned long long old = atomicCAS(keys + slot, kEmpty, key);
      if (old == kEmpty || old == key) {
        atomicAdd(counts + slot, 1u);
        placed = true;
        break;
      }
    }
    if (!placed) atomicAdd(info + 6, 1ull);
  }
}

// info: [0] distinct pairs, [1] pairs of one face, [2] pairs of more than two.  A key's halves are vertex indices that passed
// in_range in the insert kernel: the degree and flag words they name exist.
__global__ __launch_bounds__(kThreads) void adjacency_pairs_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ counts,
                                                                   unsigned long long slots, int* __restrict__ degree, int* __restrict__ flags,
                                                                   unsigned long long* __restrict__ info) {
  __shared__ unsigned long long part[kThreads / 64][3];
  unsigned long long w[3] = {0ull, 0ull, 0ull};
  for (unsigned long long s = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; s < slots; s += (unsigned long long)gridDim.x * kThreads) {
    const unsigned long long key = keys[s];
    if (key == kEmpty) continue;
    const unsigned lo = (unsigned)(key >> 32), hi = (unsigned)(key & 0xffffffffull), n = counts[s];
    atomicAdd(degree + lo, 1);
    atomicAdd(degree + hi, 1);
    const int bits = (n == 1u ? 2 : 0) | (n > 2u ? 4 : 0);
    if (bits) {
      atomicOr(flags + lo, bits);
      atomicOr(flags + hi, bits);
    }
    w[0] += 1ull;
    w[1] += n == 1u ? 1ull : 0ull;
    w[2] += n > 2u ? 1ull : 0ull;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = 0; k < 3; ++k) {
    const unsigned long long r = wave_sum(w[k]);
    if (lane == 0) part[wv][k] = r;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long r = 0ull;
    for (int j = 0; j < kThreads / 64; ++j) r += part[j][threadIdx.x];
    if (r != 0ull) atomicAdd(info + threadIdx.x, r);
  }
}

// An endpoint's row begins at offsets[v] and has degree[v] places, one per pair that names v: the cursor hands each out once.  The
// position is still held against `capacity` (6 n_faces), so that no store can leave `neighbours`.
__global__ __launch_bounds__(kThreads) void adjacency_scatter_kernel(const unsigned long long* __restrict__ keys, unsigned long long slots,
                                                                     const unsigned* __restrict__ offsets, unsigned* __restrict__ cursor,
                                                                     int* __restrict__ neighbours, unsigned long long capacity) {
  for (unsigned long long s = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; s < slots; s += (unsigned long long)gridDim.x * kThreads) {
    const unsigned long long key = keys[s];
    if (key == kEmpty) continue;
    const unsigned lo = (unsigned)(key >> 32), hi = (unsigned)(key & 0xffffffffull);
    const unsigned long long at_lo = (unsigned long long)offsets[lo] + (unsigned long long)atomicAdd(cursor + lo, 1u);
    const unsigned long long at_hi = (unsigned long long)offsets[hi] + (unsigned long long)atomicAdd(cursor + hi, 1u);
    if (at_lo < capacity) neighbours[at_lo] = (int)hi;
    if (at_hi < capacity) neighbours[at_hi] = (int)lo;
  }
}

struct AdjacencyLayout {
  unsigned long long slots;
  size_t keys, counts, cursor, tiles, total;
};

inline AdjacencyLayout adjacency_layout(long n_vertices, long n_faces) {
  AdjacencyLayout L;
  L.slots = ATVS_MESH_ADJACENCY_MIN_SLOTS;
  while (L.slots < 6ull * (unsigned long long)n_faces) L.slots <<= 1;
  L.keys = 0;
  L.counts = L.keys + (size_t)L.slots * sizeof(unsigned long long);
  L.cursor = L.counts + align256((size_t)L.slots * sizeof(unsigned));
  L.tiles = L.cursor + align256((size_t)(n_vertices + 1) * sizeof(unsigned));
  L.total = L.tiles + align256((size_t)scan_tiles(n_vertices + 1) * sizeof(unsigned));
  return L;
}

inline int walk_blocks(unsigned long long items) {
  const unsigned long long wanted = (items + kThreads - 1) / kThreads;
  return (int)(wanted < (unsigned long long)kWalkBlocks ? wanted : (unsigned long long)kWalkBlocks);
}

// ---------------------------------------------------------------------------------------------------- quantize, pass, dequantize

// info: [0] vertices with a non-finite coordinate, [1] coordinates with |q| > 2^31.
__global__ __launch_bounds__(kThreads) void quantize_kernel(const float* __restrict__ vertices, long n_vertices, double o0, double o1, double o2,
                                                            double step, long long* __restrict__ q, unsigned long long* __restrict__ info) {
  const long v = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (v >= n_vertices) return;
  const float x[3] = {vertices[v * 3 + 0], vertices[v * 3 + 1], vertices[v * 3 + 2]};
  const double o[3] = {o0, o1, o2};
  long long r[3] = {0ll, 0ll, 0ll};
  if (!finite3(x[0], x[1], x[2])) {
    atomicAdd(info + 0, 1ull);
  } else {
    int far = 0;
    for (int k = 0; k < 3; ++k) {
      const double t = rint(((double)x[k] - o[k]) / step);
      far += fabs(t) > kTwoTo31 ? 1 : 0;
      r[k] = fabs(t) < kTwoTo62 ? (long long)t : 0ll;                // (beyond 2^31 no output is defined: only no trap, no garbage)
    }
    if (far) atomicAdd(info + 1, (unsigned long long)far);
  }
  for (int k = 0; k < 3; ++k) q[v * 3 + k] = r[k];
}

// info: [0] clamped coordinates, [1] lanes whose row or a neighbour of it lies outside the arrays (they keep q_in).  Sums and the
// step are formed in unsigned arithmetic, which wraps where a caller's q_in is out of its range: no load depends on them.
__global__ __launch_bounds__(kThreads) void smooth_pass_kernel(const long long* __restrict__ q_in, long n_vertices, const int* __restrict__ degree,
                                                               const int* __restrict__ flags, const int* __restrict__ offsets,
                                                               const int* __restrict__ neighbours, long n_neighbours, double factor,
                                                               int pin_mask, long long* __restrict__ q_out, int* __restrict__ info) {
  const long v = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (v >= n_vertices) return;
  const long long q[3] = {q_in[v * 3 + 0], q_in[v * 3 + 1], q_in[v * 3 + 2]};
  long long out[3] = {q[0], q[1], q[2]};
  const int fl = flags[v], deg = degree[v];
  if ((fl & 1) && deg != 0 && !(fl & pin_mask)) {
    const long start = (long)offsets[v];
    bool bad = deg < 0 || start < 0 || start + (long)deg > n_neighbours;
    unsigned long long S[3] = {0ull, 0ull, 0ull};
    for (int j = 0; !bad && j < deg; ++j) {
      const int n = neighbours[start + j];
      if (!in_range(n, n_vertices)) {
        bad = true;
      } else {
        for (int k = 0; k < 3; ++k) S[k] += (unsigned long long)q_in[(long)n * 3 + k];
      }
    }
    if (bad) {
      atomicAdd(info + 1, 1);
    } else {
      int clamped = 0;
      for (int k = 0; k < 3; ++k) {
        const double m = (double)(long long)S[k] / (double)deg;
        const double d = m - (double)q[k];
        const double t = rint(factor * d);
        long long r;
        if (!(fabs(t) < kTwoTo62)) {
          r = t > 0.0 ? kClamp + 1ll : -kClamp - 1ll;                // only from a q_in out of its range: clamped below
        } else {
          r = (long long)((unsigned long long)q[k] + (unsigned long long)(long long)t);
        }
        if (r > kClamp) {
          r = kClamp;
          ++clamped;
        } else if (r < -kClamp) {
          r = -kClamp;
          ++clamped;
        }
        out[k] = r;
      }
      if (clamped) atomicAdd(info + 0, clamped);
    }
  }
  for (int k = 0; k < 3; ++k) q_out[v * 3 + k] = out[k];
}

__global__ __launch_bounds__(kThreads) void dequantize_kernel(const long long* __restrict__ q, const long long* __restrict__ q0,
                                                              const float* __restrict__ vertices, long n_vertices, double o0, double o1,
                                                              double o2, double step, float* __restrict__ vertices_out) {
  const long i = (long)blockIdx.x * kThreads + (long)threadIdx.x;          // one lane per coordinate
  if (i >= n_vertices * 3) return;
  const int k = (int)(i % 3);
  const double o = k == 0 ? o0 : (k == 1 ? o1 : o2);
  const long long a = q[i];
  const unsigned bits = __float_as_uint(vertices[i]);
  vertices_out[i] = a == q0[i] ? __uint_as_float(bits) : (float)(o + step * (double)a);
}

// --------------------------------------------------------------------------------------------------------------------- normals

// m = (b - a) x (c - a) in double, atvs_mesh_sample_counts' form.  i0, i1, i2 are in range.
__device__ __forceinline__ void face_cross(const float* __restrict__ vertices, int i0, int i1, int i2, double* m) {
  double e1[3], e2[3];
  for (int k = 0; k < 3; ++k) {
    const double a = (double)vertices[(long)i0 * 3 + k];
    e1[k] = (double)vertices[(long)i1 * 3 + k] - a;
    e2[k] = (double)vertices[(long)i2 * 3 + k] - a;
  }
  m[0] = e1[1] * e2[2] - e1[2] * e2[1];
  m[1] = e1[2] * e2[0] - e1[0] * e2[2];
  m[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// info: [0] the largest s as a double's bits, [1] usable faces, [2] faces with an index out of range, [3] faces with a non-finite s.
__global__ __launch_bounds__(kThreads) void face_extent_kernel(const float* __restrict__ vertices, long n_vertices, const int* __restrict__ faces,
                                                               long n_faces, unsigned long long* __restrict__ info) {
  __shared__ unsigned long long part[kThreads / 64][4];
  unsigned long long w[4] = {0ull, 0ull, 0ull, 0ull};
  for (long f = (long)blockIdx.x * kThreads + (long)threadIdx.x; f < n_faces; f += (long)gridDim.x * kThreads) {
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (!in_range(i0, n_vertices) || !in_range(i1, n_vertices) || !in_range(i2, n_vertices)) {
      ++w[2];
      continue;
    }
    double m[3];
    face_cross(vertices, i0, i1, i2, m);
    const double s = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    if (!finite_d(s)) {
      ++w[3];
      continue;
    }
    ++w[1];
    const unsigned long long b = (unsigned long long)__double_as_longlong(s);      // s >= 0: its bits order as its value
    w[0] = b > w[0] ? b : w[0];
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = 0; k < 4; ++k) {
    const unsigned long long r = k == 0 ? wave_max(w[k]) : wave_sum(w[k]);
    if (lane == 0) part[wv][k] = r;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    unsigned long long r = part[0][k];
    for (int j = 1; j < kThreads / 64; ++j) r = k == 0 ? (part[j][k] > r ? part[j][k] : r) : r + part[j][k];
    if (r != 0ull) {
      if (k == 0) atomicMax(info + k, r); else atomicAdd(info + k, r);
    }
  }
}

__global__ __launch_bounds__(kThreads) void normal_sums_kernel(const float* __restrict__ vertices, long n_vertices, const int* __restrict__ faces,
                                                               long n_faces, double area_unit, unsigned long long* __restrict__ sums,
                                                               int* __restrict__ incidences, int* __restrict__ info) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (f >= n_faces) return;
  const int i[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
  if (!in_range(i[0], n_vertices) || !in_range(i[1], n_vertices) || !in_range(i[2], n_vertices)) {
    atomicAdd(info, 1);
    return;
  }
  double m[3];
  face_cross(vertices, i[0], i[1], i[2], m);
  const double s = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  if (!finite_d(s) || !(s > 0.0)) return;
  const double r = s / area_unit, w = r < 1.0 ? r : 1.0;
  long long t[3];
  for (int k = 0; k < 3; ++k) t[k] = (long long)rint((w * (m[k] / s)) * kTwoTo30);          // |w n| <= 1
  for (int c = 0; c < 3; ++c) {
    for (int k = 0; k < 3; ++k) atomicAdd(sums + (long)i[c] * 3 + k, (unsigned long long)t[k]);
    atomicAdd(incidences + i[c], 1);
  }
}

__global__ __launch_bounds__(kThreads) void vertex_normals_kernel(const long long* __restrict__ sums, long n_vertices, float* __restrict__ normals) {
  const long v = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (v >= n_vertices) return;
  const double N[3] = {(double)sums[v * 3 + 0], (double)sums[v * 3 + 1], (double)sums[v * 3 + 2]};
  const double L = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
  for (int k = 0; k < 3; ++k) normals[v * 3 + k] = L > 0.0 ? (float)(N[k] / L) : 0.0f;
}

inline bool sizes_ok(long n_vertices, long n_faces) {
  return n_vertices >= 0 && n_vertices <= kMaxPoints && n_faces >= 0 && n_faces <= kMaxFaces;
}

inline bool finite3_host(const double* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

inline bool power_of_two(double step) {
  if (!(step > 0.0) || !std::isfinite(step)) return false;
  int e = 0;
  return frexp(step, &e) == 0.5;
}

}  // namespace

extern "C" int atvs_mesh_adjacency_scratch_size(long n_vertices, long n_faces, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (!sizes_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  *bytes = (long)adjacency_layout(n_vertices, n_faces).total;
  return ATVS_OK;
}

extern "C" int atvs_mesh_adjacency(const float* vertices, long n_vertices, const int* faces, long n_faces, void* scratch,
                                   long scratch_bytes, int* degree, int* flags, int* offsets, int* neighbours, long* info,
                                   atvs_stream_t stream) {
  if (!sizes_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  if (!scratch || !offsets || !info || (n_vertices > 0 && (!vertices || !degree || !flags)) || (n_faces > 0 && (!faces || !neighbours)))
    return ATVS_ERR_NULL;
  const AdjacencyLayout L = adjacency_layout(n_vertices, n_faces);
  if (scratch_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  char* base = static_cast<char*>(scratch);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + L.keys);
  unsigned* counts = reinterpret_cast<unsigned*>(base + L.counts);
  unsigned* cursor = reinterpret_cast<unsigned*>(base + L.cursor);
  unsigned* tiles = reinterpret_cast<unsigned*>(base + L.tiles);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(info);
  unsigned* off = reinterpret_cast<unsigned*>(offsets);
  if (hipMemsetAsync(info, 0, 7 * sizeof(long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_vertices > 0) {
    hipLaunchKernelGGL(adjacency_init_kernel, dim3((unsigned)cdiv(n_vertices, kThreads)), dim3(kThreads), 0, st, vertices, n_vertices, degree,
                       flags);
    ATVS_LAUNCH_CHECK();
  }
  if (n_faces > 0) {
    if (hipMemsetAsync(keys, 0xFF, (size_t)L.slots * sizeof(unsigned long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
    if (hipMemsetAsync(counts, 0, (size_t)L.slots * sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
    hipLaunchKernelGGL(adjacency_insert_kernel, dim3((unsigned)cdiv(n_faces, kThreads)), dim3(kThreads), 0, st, faces, n_faces, n_vertices,
                       (const int*)flags, keys, counts, L.slots, words);
    ATVS_LAUNCH_CHECK();
    hipLaunchKernelGGL(adjacency_pairs_kernel, dim3((unsigned)walk_blocks(L.slots)), dim3(kThreads), 0, st, (const unsigned long long*)keys,
                       (const unsigned*)counts, L.slots, degree, flags, words);
    ATVS_LAUNCH_CHECK();
  }
  if (n_vertices > 0 && hipMemcpyAsync(off, degree, (size_t)n_vertices * sizeof(int), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(off + n_vertices, 0, sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  const int rc = exclusive_scan(off, n_vertices + 1, tiles, st);
  if (rc != ATVS_OK) return rc;
  if (n_faces > 0 && n_vertices > 0) {
    if (hipMemsetAsync(cursor, 0, (size_t)n_vertices * sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
    hipLaunchKernelGGL(adjacency_scatter_kernel, dim3((unsigned)walk_blocks(L.slots)), dim3(kThreads), 0, st, (const unsigned long long*)keys,
                       L.slots, (const unsigned*)off, cursor, neighbours, 6ull * (unsigned long long)n_faces);
    ATVS_LAUNCH_CHECK();
  }
  return ATVS_OK;
}

extern "C" int atvs_mesh_quantize(const float* vertices, long n_vertices, const double* origin, double step, long* q, long* info,
                                  atvs_stream_t stream) {
  if (n_vertices < 0 || n_vertices > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!origin || !info || (n_vertices > 0 && (!vertices || !q))) return ATVS_ERR_NULL;
  if (!finite3_host(origin) || !power_of_two(step)) return ATVS_ERR_ARG;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(info, 0, 2 * sizeof(long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_vertices == 0) return ATVS_OK;
  hipLaunchKernelGGL(quantize_kernel, dim3((unsigned)cdiv(n_vertices, kThreads)), dim3(kThreads), 0, st, vertices, n_vertices, origin[0],
                     origin[1], origin[2], step, reinterpret_cast<long long*>(q), reinterpret_cast<unsigned long long*>(info));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_smooth_pass(const long* q_in, long n_vertices, const int* degree, const int* flags, const int* offsets,
                                     const int* neighbours, long n_neighbours, double factor, int pin_mask, long* q_out, int* info,
                                     atvs_stream_t stream) {
  if (n_vertices < 0 || n_vertices > kMaxPoints || n_neighbours < 0 || n_neighbours > 6 * kMaxFaces) return ATVS_ERR_SHAPE;
  if (!(fabs(factor) <= 1.0)) return ATVS_ERR_ARG;
  if (!info || (n_vertices > 0 && (!q_in || !q_out || !degree || !flags || !offsets)) || (n_vertices > 0 && n_neighbours > 0 && !neighbours))
    return ATVS_ERR_NULL;
  if (n_vertices > 0 && q_in == q_out) return ATVS_ERR_ARG;
  if (n_vertices == 0) return ATVS_OK;
  hipLaunchKernelGGL(smooth_pass_kernel, dim3((unsigned)cdiv(n_vertices, kThreads)), dim3(kThreads), 0, as_stream(stream),
                     reinterpret_cast<const long long*>(q_in), n_vertices, degree, flags, offsets, neighbours, n_neighbours, factor, pin_mask,
                     reinterpret_cast<long long*>(q_out), info);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_dequantize(const long* q, const long* q0, const float* vertices, long n_vertices, const double* origin,
                                    double step, float* vertices_out, atvs_stream_t stream) {
  if (n_vertices < 0 || n_vertices > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!origin || (n_vertices > 0 && (!q || !q0 || !vertices || !vertices_out))) return ATVS_ERR_NULL;
  if (!finite3_host(origin) || !power_of_two(step)) return ATVS_ERR_ARG;
  if (n_vertices == 0) return ATVS_OK;
  hipLaunchKernelGGL(dequantize_kernel, dim3((unsigned)cdiv(n_vertices * 3, kThreads)), dim3(kThreads), 0, as_stream(stream),
                     reinterpret_cast<const long long*>(q), reinterpret_cast<const long long*>(q0), vertices, n_vertices, origin[0], origin[1],
                     origin[2], step, vertices_out);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_face_extent(const float* vertices, long n_vertices, const int* faces, long n_faces, long* info,
                                     atvs_stream_t stream) {
  if (!sizes_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  if (!info || (n_faces > 0 && !faces) || (n_faces > 0 && n_vertices > 0 && !vertices)) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(info, 0, 4 * sizeof(long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_faces == 0) return ATVS_OK;
  hipLaunchKernelGGL(face_extent_kernel, dim3((unsigned)walk_blocks((unsigned long long)n_faces)), dim3(kThreads), 0, st, vertices, n_vertices,
                     faces, n_faces, reinterpret_cast<unsigned long long*>(info));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_vertex_normal_sums(const float* vertices, long n_vertices, const int* faces, long n_faces, double area_unit,
                                            long* sums, int* incidences, int* info, atvs_stream_t stream) {
  if (!sizes_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  if (!(area_unit > 0.0) || !std::isfinite(area_unit)) return ATVS_ERR_ARG;
  if (!info || (n_vertices > 0 && (!vertices || !sums || !incidences)) || (n_faces > 0 && !faces)) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(info, 0, sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_vertices > 0) {
    if (hipMemsetAsync(sums, 0, (size_t)n_vertices * 3 * sizeof(long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
    if (hipMemsetAsync(incidences, 0, (size_t)n_vertices * sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  }
  if (n_faces == 0) return ATVS_OK;
  hipLaunchKernelGGL(normal_sums_kernel, dim3((unsigned)cdiv(n_faces, kThreads)), dim3(kThreads), 0, st, vertices, n_vertices, faces, n_faces,
                     area_unit, reinterpret_cast<unsigned long long*>(sums), incidences, info);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_vertex_normals(const long* sums, long n_vertices, float* normals, atvs_stream_t stream) {
  if (n_vertices < 0 || n_vertices > kMaxPoints) return ATVS_ERR_SHAPE;
  if (n_vertices > 0 && (!sums || !normals)) return ATVS_ERR_NULL;
  if (n_vertices == 0) return ATVS_OK;
  hipLaunchKernelGGL(vertex_normals_kernel, dim3((unsigned)cdiv(n_vertices, kThreads)), dim3(kThreads), 0, as_stream(stream),
                     reinterpret_cast<const long long*>(sums), n_vertices, normals);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
