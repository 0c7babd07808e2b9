// A triangle mesh's surface sampled uniformly by area (gfx950): per-face sample counts by stochastic rounding, their offsets, the
// samples' points, faces, colours and normals (ops/mesh_sample.py, atvsnet/sample_mesh.py, atvsnet/eval_cloud.py --sample_recon).
// include/atvsnet_hip.h has the definitions, tests/mesh_sample_restated.py restates them, DESIGN.md section 10.3e has the arguments.
// Built with -ffp-contract=off: every operation below is rounded on its own.  Every random number is sample_hash() of (seed, face,
// sample within the face): no state, no order.  Integer atomics only (a sum, a maximum, two tallies): no word depends on who
// arrives first or on the launch shape.
//
//   counts     one lane per face (by stride beyond 2048 workgroups): the area in double, x = area density, floor(x) plus one where the
//              face's own uniform number is below the fraction; the total, the largest count and the skipped faces reduced per
//              workgroup, one atomic each.
//   offsets    a copy of the counts with a zero behind, then cloud_scan.h's exclusive scan: offsets[n_faces] is the total.
//   place      one lane per sample.  Lanes of a workgroup hold 256 consecutive samples, so their faces are the consecutive range
//              [face of the first, face of the last]: two lanes find those by binary search over all offsets, then every lane
//              searches that range only -- in LDS where the range has at most kStage offsets (staged by coalesced loads), in global
//              memory otherwise (sparse samples: runs of faces with count 0).  The search keeps offsets[lo] <= s < offsets[hi], so it
//              ends on the one face with offsets[f] <= s < offsets[f+1]: a face with count 0 is never chosen.  Outputs leave through
//              LDS: consecutive lanes store consecutive words (bytes for the colours) of the (S,3) arrays.
#include <math.h>

#include "common.h"
#include "cloud_scan.h"

namespace {

constexpr long kMaxFaces = ATVS_MESH_TOPOLOGY_MAX_FACES;
constexpr long kMaxSamples = ATVS_MESH_SAMPLE_MAX;
constexpr int kCountBlocks = 2048;                                 // workgroups of the counts kernel: eight per CU, the rest by stride
constexpr int kStage = 1024;                                       // offsets of a workgroup's face range held in LDS
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;
constexpr double kTwoTo32 = 4294967296.0;

// The one hash: mix(base + G (index + 1)), mod 2^64.  A face's key is sample_hash(seed, f), sample j of it draws sample_hash(key, j).
__device__ __forceinline__ unsigned long long sample_hash(unsigned long long base, unsigned long long index) {
  unsigned long long z = base + kGolden * (index + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ bool in_range(int i, long n) { return i >= 0 && (long)i < n; }
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < (double)INFINITY; }

// *word += the number of lanes of this wavefront with `flag`: one atomic per wavefront.  Called by every lane of the wavefront.
__device__ __forceinline__ void wave_tally(unsigned long long* __restrict__ word, bool flag) {
  const unsigned long long mask = __ballot(flag);
  if (mask != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(word, (unsigned long long)__popcll(mask));
}

struct Face {
  double a[3], e1[3], e2[3], n[3];
};

// The face's corner a, its edges b - a and c - a and their cross product, in double.  i0, i1, i2 are in range.
__device__ __forceinline__ void load_face(const float* __restrict__ vertices, int i0, int i1, int i2, Face& F) {
  for (int k = 0; k < 3; ++k) {
    F.a[k] = (double)vertices[(long)i0 * 3 + k];
    F.e1[k] = (double)vertices[(long)i1 * 3 + k] - F.a[k];
    F.e2[k] = (double)vertices[(long)i2 * 3 + k] - F.a[k];
  }
  F.n[0] = F.e1[1] * F.e2[2] - F.e1[2] * F.e2[1];
  F.n[1] = F.e1[2] * F.e2[0] - F.e1[0] * F.e2[2];
  F.n[2] = F.e1[0] * F.e2[1] - F.e1[1] * F.e2[0];
}

// info: [0] the total, [1] faces with an index out of range, [2] faces with a non-finite area, [3] the largest count.  At most
// kCountBlocks workgroups stride over the faces; a lane keeps its four tallies in registers, a wavefront folds them by shuffles, the
// workgroup through LDS, and its first lane issues one atomic per word that is not 0: four words shared by every face would
// otherwise serialise one atomic per wavefront in the L2.  Integer sums and a maximum: the grouping does not show.
__global__ __launch_bounds__(kThreads) void sample_counts_kernel(const float* __restrict__ vertices, long n_vertices,
                                                                 const int* __restrict__ faces, long n_faces, double density,
                                                                 unsigned long long seed, unsigned* __restrict__ counts,
                                                                 double* __restrict__ areas, unsigned long long* __restrict__ info) {
  __shared__ unsigned long long part[kThreads / 64][4];
  unsigned long long sum = 0ull, most = 0ull, n_bad = 0ull, n_nonfinite = 0ull;
  for (long f = (long)blockIdx.x * kThreads + (long)threadIdx.x; f < n_faces; f += (long)gridDim.x * kThreads) {
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    unsigned long long c = 0ull;
    double area = 0.0;
    if (!in_range(i0, n_vertices) | !in_range(i1, n_vertices) | !in_range(i2, n_vertices)) {
      ++n_bad;
    } else {
      Face F;
      load_face(vertices, i0, i1, i2, F);
      const double a = 0.5 * sqrt((F.n[0] * F.n[0] + F.n[1] * F.n[1]) + F.n[2] * F.n[2]);
      if (!finite_d(a)) {
        ++n_nonfinite;
      } else {
        area = a;
        const double x = a * density;
        if (x >= (double)kMaxSamples) {
          c = (unsigned long long)(x < kTwoTo32 ? floor(x) : kTwoTo32);          // beyond the limit: what it takes, at most 2^32
        } else {
          const double fl = floor(x);
          const double u = ((double)(sample_hash(seed, (unsigned long long)f) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
          c = (unsigned long long)fl + (u < x - fl ? 1ull : 0ull);
        }
      }
    }
    counts[f] = c > 0xffffffffull ? 0xffffffffu : (unsigned)c;
    areas[f] = area;
    sum += c;
    most = c > most ? c : most;
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_xor(sum, off);
    n_bad += __shfl_xor(n_bad, off);
    n_nonfinite += __shfl_xor(n_nonfinite, off);
    const unsigned long long o = __shfl_xor(most, off);
    most = o > most ? o : most;
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[w][0] = sum;
    part[w][1] = n_bad;
    part[w][2] = n_nonfinite;
    part[w][3] = most;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kThreads / 64; ++k) {
      sum += part[k][0];
      n_bad += part[k][1];
      n_nonfinite += part[k][2];
      most = part[k][3] > most ? part[k][3] : most;
    }
    if (sum) atomicAdd(info + 0, sum);
    if (n_bad) atomicAdd(info + 1, n_bad);
    if (n_nonfinite) atomicAdd(info + 2, n_nonfinite);
    if (most) atomicMax(info + 3, most);
  }
}

// The face f in [lo, hi) with off[f] <= s < off[f + 1], given off[lo] <= s < off[hi].
template <typename Offsets>
__device__ __forceinline__ long find_face(const Offsets& off, long lo, long hi, unsigned s) {
  while (hi - lo > 1) {
    const long mid = lo + ((hi - lo) >> 1);
    if (off(mid) <= s) lo = mid; else hi = mid;
  }
  return lo;
}

// info: [0] 1 when offsets[n_faces] != n_samples (nothing is written then), [1] samples of a face with an index out of range.
__global__ __launch_bounds__(kThreads) void sample_place_kernel(const float* __restrict__ vertices, const unsigned char* __restrict__ colors,
                                                                long n_vertices, const int* __restrict__ faces, long n_faces,
                                                                const unsigned* __restrict__ offsets, long n_samples,
                                                                unsigned long long seed, float* __restrict__ points,
                                                                int* __restrict__ sample_face, unsigned char* __restrict__ colors_out,
                                                                float* __restrict__ normals, unsigned long long* __restrict__ info) {
  __shared__ unsigned stage[kStage];
  __shared__ long range[2];
  __shared__ float out[kThreads * 3];
  __shared__ unsigned char out_c[kThreads * 3];
  if ((long)offsets[n_faces] != n_samples) {                          // the same in every lane of the launch
    if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = 1ull;
    return;
  }
  const long base = (long)blockIdx.x * kThreads;                      // < n_samples: the grid is cdiv(n_samples, kThreads)
  const long s = base + (long)threadIdx.x;
  const bool live = s < n_samples;
  const auto global_off = [&](long i) { return offsets[i]; };
  if (threadIdx.x == 0) range[0] = find_face(global_off, 0, n_faces, (unsigned)base);
  if (threadIdx.x == 64) {
    const long last = base + kThreads - 1 < n_samples ? base + kThreads - 1 : n_samples - 1;
    range[1] = find_face(global_off, 0, n_faces, (unsigned)last);
  }
  __syncthreads();
  const long f_lo = range[0], f_hi = range[1];                       // offsets[f_lo] <= s < offsets[f_hi + 1] for every live s
  const bool staged = f_hi - f_lo + 2 <= (long)kStage;
  if (staged) {
    for (long i = threadIdx.x; i < f_hi - f_lo + 2; i += kThreads) stage[i] = offsets[f_lo + i];
    __syncthreads();
  }
  long f = f_lo;
  unsigned first = 0u;
  if (live) {
    if (staged) {
      f = f_lo + find_face([&](long i) { return stage[i]; }, 0, f_hi - f_lo + 1, (unsigned)s);
      first = stage[f - f_lo];
    } else {
      f = find_face(global_off, f_lo, f_hi + 1, (unsigned)s);
      first = offsets[f];
    }
  }
  const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  const bool bad = live & (!in_range(i0, n_vertices) | !in_range(i1, n_vertices) | !in_range(i2, n_vertices));
  float p[3] = {0.0f, 0.0f, 0.0f}, m[3] = {0.0f, 0.0f, 0.0f};
  unsigned char col[3] = {0, 0, 0};
  if (live && !bad) {
    Face F;
    load_face(vertices, i0, i1, i2, F);
    const unsigned long long w = sample_hash(sample_hash(seed, (unsigned long long)f), (unsigned long long)((unsigned)s - first));
    double u = ((double)(w >> 32) + 0.5) * (1.0 / kTwoTo32), v = ((double)(w & 0xffffffffull) + 0.5) * (1.0 / kTwoTo32);
    if (u + v > 1.0) {
      u = 1.0 - u;
      v = 1.0 - v;
    }
    for (int k = 0; k < 3; ++k) p[k] = (float)((F.a[k] + u * F.e1[k]) + v * F.e2[k]);
    if (normals) {
      const double r = sqrt((F.n[0] * F.n[0] + F.n[1] * F.n[1]) + F.n[2] * F.n[2]);
      for (int k = 0; k < 3; ++k) m[k] = (float)(F.n[k] / r);
    }
    if (colors) {
      const double t = (1.0 - u) - v;
      for (int k = 0; k < 3; ++k)
        col[k] = (unsigned char)rint((t * (double)colors[(long)i0 * 3 + k] + u * (double)colors[(long)i1 * 3 + k]) +
                                     v * (double)colors[(long)i2 * 3 + k]);
    }
  }
  wave_tally(info + 1, bad);
  if (live) sample_face[s] = bad ? -1 : (int)f;
  const long words = (n_samples - base < (long)kThreads ? n_samples - base : (long)kThreads) * 3;    // this workgroup's share of an (S,3) array
  for (int k = 0; k < 3; ++k) {
    out[threadIdx.x * 3 + k] = p[k];
    out_c[threadIdx.x * 3 + k] = col[k];
  }
  __syncthreads();
  for (long i = threadIdx.x; i < words; i += kThreads) {
    points[base * 3 + i] = out[i];
    if (colors) colors_out[base * 3 + i] = out_c[i];
  }
  if (normals) {
    __syncthreads();
    for (int k = 0; k < 3; ++k) out[threadIdx.x * 3 + k] = m[k];
    __syncthreads();
    for (long i = threadIdx.x; i < words; i += kThreads) normals[base * 3 + i] = out[i];
  }
}

inline bool sizes_ok(long n_vertices, long n_faces) {
  return n_vertices >= 0 && n_vertices <= kMaxPoints && n_faces >= 0 && n_faces <= kMaxFaces;
}

}  // namespace

extern "C" int atvs_mesh_sample_counts(const float* vertices, long n_vertices, const int* faces, long n_faces, double density, long seed,
                                       void* counts, double* areas, long* info, atvs_stream_t stream) {
  if (!sizes_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  if (!(density > 0.0) || !(density < (double)INFINITY) || seed < 0) return ATVS_ERR_ARG;
  if (!info || (n_faces > 0 && (!faces || !counts || !areas)) || (n_faces > 0 && n_vertices > 0 && !vertices)) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(info, 0, 4 * sizeof(long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_faces == 0) return ATVS_OK;
  const int blocks = cdiv(n_faces, kThreads) < kCountBlocks ? cdiv(n_faces, kThreads) : kCountBlocks;
  hipLaunchKernelGGL(sample_counts_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, vertices, n_vertices, faces,
                     n_faces, density, (unsigned long long)seed, static_cast<unsigned*>(counts), areas,
                     reinterpret_cast<unsigned long long*>(info));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_sample_scratch_size(long n_faces, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n_faces < 0 || n_faces > kMaxFaces) return ATVS_ERR_SHAPE;
  *bytes = (long)align256((size_t)scan_tiles(n_faces + 1) * sizeof(unsigned));
  return ATVS_OK;
}

extern "C" int atvs_mesh_sample_offsets(const void* counts, long n_faces, void* scratch, long scratch_bytes, void* offsets,
                                        atvs_stream_t stream) {
  if (n_faces < 0 || n_faces > kMaxFaces) return ATVS_ERR_SHAPE;
  if (!offsets || !scratch || (n_faces > 0 && !counts)) return ATVS_ERR_NULL;
  if (scratch_bytes < (long)align256((size_t)scan_tiles(n_faces + 1) * sizeof(unsigned))) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  unsigned* off = static_cast<unsigned*>(offsets);
  if (n_faces > 0 && hipMemcpyAsync(off, counts, (size_t)n_faces * sizeof(unsigned), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(off + n_faces, 0, sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  return exclusive_scan(off, n_faces + 1, static_cast<unsigned*>(scratch), st);
}

extern "C" int atvs_mesh_sample_place(const float* vertices, const void* colors, long n_vertices, const int* faces, long n_faces,
                                      const void* offsets, long n_samples, long seed, float* points, int* sample_face, void* colors_out,
                                      float* normals, long* info, atvs_stream_t stream) {
  if (!sizes_ok(n_vertices, n_faces) || n_samples < 0 || n_samples > kMaxSamples) return ATVS_ERR_SHAPE;
  if (seed < 0) return ATVS_ERR_ARG;
  if (!info || (n_samples > 0 && (!vertices || !faces || !offsets || !points || !sample_face || (colors && !colors_out))))
    return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(info, 0, 2 * sizeof(long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_samples == 0) return ATVS_OK;
  if (n_faces == 0) return ATVS_ERR_SHAPE;                               // samples of no face
  hipLaunchKernelGGL(sample_place_kernel, dim3((unsigned)cdiv(n_samples, kThreads)), dim3(kThreads), 0, st, vertices,
                     static_cast<const unsigned char*>(colors), n_vertices, faces, n_faces, static_cast<const unsigned*>(offsets),
                     n_samples, (unsigned long long)seed, points, sample_face, static_cast<unsigned char*>(colors_out), normals,
                     reinterpret_cast<unsigned long long*>(info));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
