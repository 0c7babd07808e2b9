// Point-cloud registration (gfx950): moving a cloud through a matrix, the moments of matched pairs that a closed-form similarity fit
// needs, and a sparse voxel down-sampler (ops/cloud.py, atvsnet/register_cloud.py).  The definitions are in include/atvsnet_hip.h;
// tests/cloud_register_restated.py restates them with numpy and Python integers.  Built with -ffp-contract=off (every operation below
// is rounded on its own); integer atomics only, so every output is a function of the inputs alone.
//
// PAIR MOMENTS, the shape of the sum.  Pair i belongs to workgroup i / (256 L), thread (i mod 256), L = kMomentRun: a thread adds
// its at most L terms i, i + 256, ... in that order into an accumulator that starts at +0 (the first addition is exact), the 64
// lanes of a wavefront fold in six steps (lane j takes lane j + 32, then + 16, ... + 1), the four wavefronts as (w0 + w1) + (w2 + w3).
// That is one row of 19 words per workgroup.  Rows are folded 256 at a time by the same eight-step tree (row j takes row j + 128,
// + 64, ... + 1; rows beyond the end are +0, and adding +0 is exact) until one is left: one pass up to 65 536 pairs x L, two up to
// 2^24 x L, three beyond.  An accumulator therefore sees at most L serial additions and then at most
// 8 + ceil(log2(rows)) + (passes - 1) tree levels that round, rows = ceil(m / (256 L)) -- no more than L + ceil(log2 m) in all for
// every m <= 2^30 (m > 256 L (rows - 1) gives log2 m > 8 + log2 L + log2(rows - 1), and log2 L = 4 pays for the passes).
// The point-to-plane moments (atvs_cloud_plane_moments) are the same sum with rows of 38 words.
//
// VOXEL DOWN-SAMPLING.  insert: every finite point finds its voxel's slot in an open-addressing table (capacity = the power of two
// >= max(2 n, 1024); linear probing from a multiplicative hash of the packed cell; one 64-bit compare-and-swap per probe) and adds
// to the slot's count and three unsigned 64-bit sums, and takes the minimum of the slot's first index.  flag: a point that is its
// voxel's first index is marked; an exclusive scan of the marks (cloud_scan.h) gives its output row.  emit: the marked points write
// their voxel's mean and their own index there.  Which slot a voxel gets depends on arrival order; nothing that is written does.
//
// VOXEL-AVERAGED SHARES (atvs_cloud_voxel_shares): the same cells and table, per-voxel hit / observed counters
// per tolerance instead of sums; described where its kernels are.
#include <math.h>

#include "common.h"
#include "cloud_scan.h"
#include "cloud_tree.h"
#include "cloud_voxel.h"

namespace {

constexpr int kWords = 19;                             // pair count (int64) + 18 doubles
constexpr long kMinSlots = 1024;
constexpr size_t kVoxelHeader = 256;

struct Matrix12 {
  double t[12];
};

struct MomentArgs {
  double trim2;          // trim * trim
  double ps[3], pd[3];   // pivots
};

__global__ __launch_bounds__(kThreads) void cloud_transform_kernel(const float* points, long n, Matrix12 M, float* out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double x = (double)points[i * 3 + 0], y = (double)points[i * 3 + 1], z = (double)points[i * 3 + 2];
  const double* T = M.t;
  const float ox = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
  const float oy = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
  const float oz = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
  out[i * 3 + 0] = ox;                                  // `out` may be `points`: all three coordinates were read above
  out[i * 3 + 1] = oy;
  out[i * 3 + 2] = oz;
}

__global__ __launch_bounds__(kThreads) void cloud_pair_moments_kernel(const float* __restrict__ src, const float* __restrict__ dst, long n,
                                                                      const int* __restrict__ idx, const float* __restrict__ d2, long m,
                                                                      MomentArgs A, unsigned long long* __restrict__ rows) {
  __shared__ MomentShared<kWords - 1> sh;
  moment_row<kWords - 1>(m, [&](long i, long long& cnt, double* v) {
    const int j = idx[i];
    const float dd = d2[i];
    if (j < 0 || (long)j >= n || !((double)dd <= A.trim2)) return;
    const double a0 = (double)src[i * 3 + 0] - A.ps[0], a1 = (double)src[i * 3 + 1] - A.ps[1], a2 = (double)src[i * 3 + 2] - A.ps[2];
    const double b0 = (double)dst[(long)j * 3 + 0] - A.pd[0], b1 = (double)dst[(long)j * 3 + 1] - A.pd[1],
                 b2 = (double)dst[(long)j * 3 + 2] - A.pd[2];
    cnt += 1;
    v[0] = v[0] + a0; v[1] = v[1] + a1; v[2] = v[2] + a2;
    v[3] = v[3] + b0; v[4] = v[4] + b1; v[5] = v[5] + b2;
    v[6] = v[6] + a0 * b0; v[7] = v[7] + a0 * b1; v[8] = v[8] + a0 * b2;
    v[9] = v[9] + a1 * b0; v[10] = v[10] + a1 * b1; v[11] = v[11] + a1 * b2;
    v[12] = v[12] + a2 * b0; v[13] = v[13] + a2 * b1; v[14] = v[14] + a2 * b2;
    v[15] = v[15] + ((a0 * a0 + a1 * a1) + a2 * a2);
    v[16] = v[16] + ((b0 * b0 + b1 * b1) + b2 * b2);
    v[17] = v[17] + (double)dd;
  }, rows, sh);
}

// ---- point-to-plane moments ----------------------------------------------------------------------------------------------------
// The sums of a Gauss-Newton step of point-to-plane ICP over the source's normals (include/atvsnet_hip.h states the definition and
// derives the Jacobian; tests/cloud_plane_restated.py restates it).  The same row shape and tree as the pair moments, 37 sums wide.

constexpr int kPlaneSums = 37;                         // 28 J_a J_b (a <= b) + 7 J_a r + r^2 + d2
constexpr int kPlaneWords = kPlaneSums + 1;

struct PlaneArgs {
  double t[12];          // T, rows 0-2
  double rot[9];         // the rotation of T
  double trim2;
  double pivot[3];
};

// where J_a J_b (a <= b) lies among the 28 sums, row-major over the upper triangle of the 7 x 7 matrix
__host__ __device__ constexpr int plane_at(int a, int b) { return a * 7 - a * (a - 1) / 2 + (b - a); }

__global__ __launch_bounds__(kThreads) void cloud_plane_moments_kernel(const float* __restrict__ src, const float* __restrict__ normals,
                                                                       const float* __restrict__ dst, long n, const int* __restrict__ idx,
                                                                       const float* __restrict__ d2, long m, PlaneArgs A,
                                                                       unsigned long long* __restrict__ rows) {
  __shared__ MomentShared<kPlaneSums> sh;
  moment_row<kPlaneSums>(m, [&](long i, long long& cnt, double* v) {
    const int j = idx[i];
    const float dd = d2[i];
    if (j < 0 || (long)j >= n || !((double)dd <= A.trim2)) return;
    const float fx = normals[i * 3 + 0], fy = normals[i * 3 + 1], fz = normals[i * 3 + 2];
    if (!finite3(fx, fy, fz)) return;
    const double nx = (double)fx, ny = (double)fy, nz = (double)fz;
    if (!((nx * nx + ny * ny) + nz * nz > 0.0)) return;                      // the zero normal agrees with nothing
    const double x = (double)src[i * 3 + 0], y = (double)src[i * 3 + 1], z = (double)src[i * 3 + 2];
    const double* T = A.t;
    const double* R = A.rot;
    const double q0 = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - A.pivot[0];
    const double q1 = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - A.pivot[1];
    const double q2 = (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - A.pivot[2];
    const double g0 = (double)dst[(long)j * 3 + 0] - A.pivot[0], g1 = (double)dst[(long)j * 3 + 1] - A.pivot[1],
                 g2 = (double)dst[(long)j * 3 + 2] - A.pivot[2];
    const double n0 = (R[0] * nx + R[1] * ny) + R[2] * nz;
    const double n1 = (R[3] * nx + R[4] * ny) + R[5] * nz;
    const double n2 = (R[6] * nx + R[7] * ny) + R[8] * nz;
    const double e0 = q0 - g0, e1 = q1 - g1, e2 = q2 - g2;
    const double r = (e0 * n0 + e1 * n1) + e2 * n2;
    const double J[7] = {g1 * n2 - g2 * n1, g2 * n0 - g0 * n2, g0 * n1 - g1 * n0, n0, n1, n2, (q0 * n0 + q1 * n1) + q2 * n2};
    cnt += 1;
#pragma unroll
    for (int a = 0; a < 7; ++a) {
#pragma unroll
      for (int b = a; b < 7; ++b) v[plane_at(a, b)] = v[plane_at(a, b)] + J[a] * J[b];
    }
#pragma unroll
    for (int a = 0; a < 7; ++a) v[28 + a] = v[28 + a] + J[a] * r;
    v[35] = v[35] + r * r;
    v[36] = v[36] + (double)dd;
  }, rows, sh);
}

// The same sums over the TARGET's normals (atvs_cloud_plane_moments_target): the normal belongs to the matched point and stays in
// the target's frame, so nothing is rotated and the lever arm is the moved source's, q x n.
struct PlaneTargetArgs {
  double t[12];          // T, rows 0-2
  double trim2;
  double pivot[3];
};

__global__ __launch_bounds__(kThreads) void cloud_plane_moments_target_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                                              const float* __restrict__ dst_normals, long n,
                                                                              const int* __restrict__ idx, const float* __restrict__ d2, long m,
                                                                              PlaneTargetArgs A, unsigned long long* __restrict__ rows) {
  __shared__ MomentShared<kPlaneSums> sh;
  moment_row<kPlaneSums>(m, [&](long i, long long& cnt, double* v) {
    const int j = idx[i];
    const float dd = d2[i];
    if (j < 0 || (long)j >= n || !((double)dd <= A.trim2)) return;
    const float fx = dst_normals[(long)j * 3 + 0], fy = dst_normals[(long)j * 3 + 1], fz = dst_normals[(long)j * 3 + 2];
    if (!finite3(fx, fy, fz)) return;
    const double n0 = (double)fx, n1 = (double)fy, n2 = (double)fz;
    if (!((n0 * n0 + n1 * n1) + n2 * n2 > 0.0)) return;                      // the zero normal agrees with nothing
    const double x = (double)src[i * 3 + 0], y = (double)src[i * 3 + 1], z = (double)src[i * 3 + 2];
    const double* T = A.t;
    const double q0 = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - A.pivot[0];
    const double q1 = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - A.pivot[1];
    const double q2 = (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - A.pivot[2];
    const double g0 = (double)dst[(long)j * 3 + 0] - A.pivot[0], g1 = (double)dst[(long)j * 3 + 1] - A.pivot[1],
                 g2 = (double)dst[(long)j * 3 + 2] - A.pivot[2];
    const double e0 = q0 - g0, e1 = q1 - g1, e2 = q2 - g2;
    const double r = (e0 * n0 + e1 * n1) + e2 * n2;
    const double J[7] = {q1 * n2 - q2 * n1, q2 * n0 - q0 * n2, q0 * n1 - q1 * n0, n0, n1, n2, (q0 * n0 + q1 * n1) + q2 * n2};
    cnt += 1;
#pragma unroll
    for (int a = 0; a < 7; ++a) {
#pragma unroll
      for (int b = a; b < 7; ++b) v[plane_at(a, b)] = v[plane_at(a, b)] + J[a] * J[b];
    }
#pragma unroll
    for (int a = 0; a < 7; ++a) v[28 + a] = v[28 + a] + J[a] * r;
    v[35] = v[35] + r * r;
    v[36] = v[36] + (double)dd;
  }, rows, sh);
}

// ---- voxel down-sampling -------------------------------------------------------------------------------------------------------

struct VoxelLayout {
  size_t keys, first, zero, sums, cnt, slot, flags, tiles, total;   // [header | keys | first] are set to ~0 / 0, [sums .. flags] to 0
  long slots;
  int shift;                                                          // 64 - log2(slots)
};
inline VoxelLayout voxel_layout(long n) {
  VoxelLayout L;
  long slots = kMinSlots;
  int lg = 10;
  while (slots < 2 * n) {
    slots <<= 1;
    ++lg;
  }
  L.slots = slots;
  L.shift = 64 - lg;
  L.keys = kVoxelHeader;
  L.first = L.keys + align256((size_t)slots * 8);
  L.zero = L.first + align256((size_t)slots * 4);
  L.sums = L.zero;
  L.cnt = L.sums + align256((size_t)slots * 24);
  L.flags = L.cnt + align256((size_t)slots * 4);
  L.slot = L.flags + align256((size_t)(n + 1) * 4);
  L.tiles = L.slot + align256((size_t)n * 4);
  L.total = L.tiles + align256((size_t)scan_tiles(n + 1) * 4);
  return L;
}

// The cells, the key and the slot of a point are cloud_voxel.h's (shared with mesh_simplify.hip).
// An empty table in the scratch `s`: the header (the error word) zeroed, [keys, ones_end) all-ones (kEmpty); -> err, keys, slot_of
struct VoxelTable {
  int* err;
  unsigned long long* keys;
  int* slot_of;
};
inline bool voxel_table(char* s, size_t keys, size_t ones_end, size_t slot, hipStream_t st, VoxelTable* T) {
  *T = VoxelTable{reinterpret_cast<int*>(s), reinterpret_cast<unsigned long long*>(s + keys), reinterpret_cast<int*>(s + slot)};
  return hipMemsetAsync(s, 0, kVoxelHeader, st) == hipSuccess && hipMemsetAsync(s + keys, 0xff, ones_end - keys, st) == hipSuccess;
}

__global__ __launch_bounds__(kThreads) void cloud_voxel_insert_kernel(const float* __restrict__ pts, long n, VoxelArgs A, long slots, int shift,
                                                                      unsigned long long* __restrict__ keys, unsigned* __restrict__ first,
                                                                      unsigned long long* __restrict__ sums, unsigned* __restrict__ cnt,
                                                                      int* __restrict__ slot_of, int* __restrict__ err) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  unsigned long long u[3];
  const int s = voxel_slot_of(pts, i, A, slots, shift, keys, err, u);
  if (s >= 0) {
    atomicAdd(cnt + s, 1u);
    atomicAdd(sums + (long)s * 3 + 0, u[0]);
    atomicAdd(sums + (long)s * 3 + 1, u[1]);
    atomicAdd(sums + (long)s * 3 + 2, u[2]);
    atomicMin(first + s, (unsigned)i);
  }
  slot_of[i] = s;
}

__global__ __launch_bounds__(kThreads) void cloud_voxel_flag_kernel(const int* __restrict__ slot_of, const unsigned* __restrict__ first, long n,
                                                                    unsigned* __restrict__ flags) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int s = slot_of[i];
  flags[i] = (s >= 0 && first[s] == (unsigned)i) ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void cloud_voxel_emit_kernel(const int* __restrict__ slot_of, long n, VoxelArgs A,
                                                                    const unsigned long long* __restrict__ keys,
                                                                    const unsigned* __restrict__ first,
                                                                    const unsigned long long* __restrict__ sums,
                                                                    const unsigned* __restrict__ cnt, const unsigned* __restrict__ pos,
                                                                    const int* __restrict__ err, float* __restrict__ out_points,
                                                                    long long* __restrict__ out_count, int* __restrict__ out_first) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const bool bad = *err != 0;
  if (i == 0) *out_count = bad ? -1ll : (long long)pos[n];
  if (i >= n || bad) return;
  const int s = slot_of[i];
  if (s < 0 || first[s] != (unsigned)i) return;
  const unsigned p = pos[i];
  if ((long)p >= n) return;
  const unsigned long long key = keys[s];
  const double k = (double)cnt[s];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double c = (double)((key >> (21 * a)) & 0x1fffffull);
    const double mean = ((double)sums[(long)s * 3 + a] / k) / 4294967296.0;
    out_points[(long)p * 3 + a] = (float)(A.origin[a] + A.voxel * (c + mean));
  }
  out_first[p] = (int)i;
}

// ---- voxel-averaged shares -----------------------------------------------------------------------------------------------------
// The down-sampler's table once more (the same cells: voxel_coord), holding per voxel two counters per tolerance of a pass instead
// of sums.  insert: every finite point finds its voxel's slot.  Then, kSharePass tolerances at a time: count (a point adds 1 to its
// voxel's `hit` or `other` counter per tolerance, or to neither when it is unobserved), reduce (one lane per slot: the voxel's
// fixed-point share q and the counts, summed over the workgroup and added to the four output words of the tolerance).  Unsigned
// integer atomics only: which slot a voxel gets and who adds first depend on arrival order, no word that is written does.

constexpr int kSharePass = 4;                          // tolerances per pass: 8 B of counters per slot each

struct ShareLayout {
  size_t keys, cnt, slot, total;                       // [header | keys] are set to 0 / ~0, cnt to 0 before every pass
  long slots;
  int shift;
};
inline ShareLayout share_layout(long n) {
  const VoxelLayout V = voxel_layout(n);
  ShareLayout L;
  L.slots = V.slots;
  L.shift = V.shift;
  L.keys = kVoxelHeader;
  L.cnt = L.keys + align256((size_t)L.slots * 8);
  L.slot = L.cnt + align256((size_t)L.slots * 8 * kSharePass);
  L.total = L.slot + align256((size_t)n * 4);
  return L;
}

struct ShareArgs {
  double tau2[kSharePass];                             // tau * tau
  double margin;
  int count;                                           // tolerances of this pass
};

__global__ __launch_bounds__(kThreads) void cloud_share_insert_kernel(const float* __restrict__ pts, long n, VoxelArgs A, long slots, int shift,
                                                                      unsigned long long* __restrict__ keys, int* __restrict__ slot_of,
                                                                      int* __restrict__ err) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  unsigned long long u[3];
  slot_of[i] = voxel_slot_of(pts, i, A, slots, shift, keys, err, u);
}

__global__ __launch_bounds__(kThreads) void cloud_share_count_kernel(const int* __restrict__ slot_of, const float* __restrict__ d2,
                                                                     const float* __restrict__ excess, long n, ShareArgs A,
                                                                     unsigned* __restrict__ cnt) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int s = slot_of[i];
  if (s < 0) return;
  const double d = (double)d2[i];
  const bool observed = !excess || (double)excess[i] <= A.margin;      // NaN: unobserved
  unsigned* __restrict__ c = cnt + (size_t)s * (2 * kSharePass);
  for (int k = 0; k < A.count; ++k) {
    if (d <= A.tau2[k]) atomicAdd(c + 2 * k, 1u);
    else if (observed) atomicAdd(c + 2 * k + 1, 1u);
  }
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {      // lane 0 holds the sum of all 64 lanes
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = (unsigned)__shfl_down((int)(unsigned)(v & 0xffffffffull), off);
    const unsigned hi = (unsigned)__shfl_down((int)(unsigned)(v >> 32), off);
    v += ((unsigned long long)hi << 32) | (unsigned long long)lo;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void cloud_share_reduce_kernel(const unsigned long long* __restrict__ keys, long slots,
                                                                      const unsigned* __restrict__ cnt, int count, int total,
                                                                      const int* __restrict__ err, unsigned long long* __restrict__ out,
                                                                      unsigned long long* __restrict__ out_all) {
  __shared__ unsigned long long part[kThreads / 64][4 * kSharePass];
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (*err != 0) {                                            // a point outside the 2^21 cells: every word of the result is -1
    if (i < 4L * total) out_all[i] = ~0ull;
    return;
  }
  const bool used = i < slots && keys[i] != kEmpty;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int k = 0; k < count; ++k) {                           // uniform: every lane takes part in the shuffles
    unsigned long long hit = 0ull, den = 0ull;
    if (used) {
      hit = cnt[(size_t)i * (2 * kSharePass) + 2 * k];
      den = hit + cnt[(size_t)i * (2 * kSharePass) + 2 * k + 1];
    }
    const unsigned long long q = wave_sum64(den ? (hit << 32) / den : 0ull);
    const unsigned long long voxels = wave_sum64(den ? 1ull : 0ull);
    const unsigned long long hits = wave_sum64(hit), dens = wave_sum64(den);
    if (lane == 0) {
      part[w][4 * k + 0] = q;
      part[w][4 * k + 1] = voxels;
      part[w][4 * k + 2] = hits;
      part[w][4 * k + 3] = dens;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 4 * count) {                         // one lane per output word adds the workgroup's four wavefronts
    unsigned long long v = 0ull;
    for (int j = 0; j < kThreads / 64; ++j) v += part[j][threadIdx.x];
    if (v) atomicAdd(out + threadIdx.x, v);
  }
}

}  // namespace

extern "C" int atvs_cloud_transform(const float* points, long n, const double* matrix12, float* out, atvs_stream_t stream) {
  if (n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!matrix12 || (n > 0 && (!points || !out))) return ATVS_ERR_NULL;
  if (n == 0) return ATVS_OK;
  Matrix12 M;
  for (int k = 0; k < 12; ++k) M.t[k] = matrix12[k];
  hipLaunchKernelGGL(cloud_transform_kernel, dim3((unsigned)cdiv(n, kThreads)), dim3(kThreads), 0, as_stream(stream), points, n, M, out);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_cloud_pair_moments_scratch_size(long m, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)moment_scratch_bytes<kWords - 1>(m);
  return ATVS_OK;
}

extern "C" int atvs_cloud_pair_moments(const float* src, const float* dst, long n, const int* idx, const float* d2, long m, double trim,
                                       const double* pivot_src, const double* pivot_dst, void* scratch, long scratch_bytes, void* out,
                                       atvs_stream_t stream) {
  if (m < 0 || m > kMaxPoints || n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!out || !pivot_src || !pivot_dst || (m > 0 && (!src || !idx || !d2 || !scratch)) || (m > 0 && n > 0 && !dst)) return ATVS_ERR_NULL;
  if (!(trim >= 0.0)) return ATVS_ERR_ARG;                  // NaN or negative; +inf is allowed
  MomentArgs A;
  A.trim2 = trim * trim;
  for (int k = 0; k < 3; ++k) {
    if (!(fabs(pivot_src[k]) <= 1.7976931348623157e308) || !(fabs(pivot_dst[k]) <= 1.7976931348623157e308)) return ATVS_ERR_ARG;
    A.ps[k] = pivot_src[k];
    A.pd[k] = pivot_dst[k];
  }
  long need = 0;
  atvs_cloud_pair_moments_scratch_size(m, &need);
  if (m > 0 && scratch_bytes < need) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  unsigned long long* res = static_cast<unsigned long long*>(out);
  if (m == 0) return hipMemsetAsync(out, 0, kWords * 8, st) == hipSuccess ? ATVS_OK : ATVS_ERR_LAUNCH;
  unsigned long long* level = static_cast<unsigned long long*>(scratch);
  hipLaunchKernelGGL(cloud_pair_moments_kernel, dim3((unsigned)moment_rows(m)), dim3(kThreads), 0, st, src, dst, n, idx, d2, m, A,
                     moment_first(m, level, res));
  ATVS_LAUNCH_CHECK();
  return moment_fold<kWords - 1>(m, level, res, st);
}

extern "C" int atvs_cloud_plane_moments_scratch_size(long m, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)moment_scratch_bytes<kPlaneSums>(m);
  return ATVS_OK;
}

extern "C" int atvs_cloud_plane_moments(const float* src, const float* normals, const double* matrix12, const double* rot9, const float* dst,
                                        long n, const int* idx, const float* d2, long m, double trim, const double* pivot, void* scratch,
                                        long scratch_bytes, void* out, atvs_stream_t stream) {
  const double big = 1.7976931348623157e308;
  if (m < 0 || m > kMaxPoints || n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!out || !matrix12 || !rot9 || !pivot || (m > 0 && (!src || !normals || !idx || !d2 || !scratch)) || (m > 0 && n > 0 && !dst))
    return ATVS_ERR_NULL;
  if (!(trim >= 0.0)) return ATVS_ERR_ARG;                  // NaN or negative; +inf is allowed
  PlaneArgs A;
  A.trim2 = trim * trim;
  for (int k = 0; k < 12; ++k) {
    if (!(fabs(matrix12[k]) <= big)) return ATVS_ERR_ARG;
    A.t[k] = matrix12[k];
  }
  for (int k = 0; k < 9; ++k) {
    if (!(fabs(rot9[k]) <= big)) return ATVS_ERR_ARG;
    A.rot[k] = rot9[k];
  }
  for (int k = 0; k < 3; ++k) {
    if (!(fabs(pivot[k]) <= big)) return ATVS_ERR_ARG;
    A.pivot[k] = pivot[k];
  }
  long need = 0;
  atvs_cloud_plane_moments_scratch_size(m, &need);
  if (m > 0 && scratch_bytes < need) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  unsigned long long* res = static_cast<unsigned long long*>(out);
  if (m == 0) return hipMemsetAsync(out, 0, kPlaneWords * 8, st) == hipSuccess ? ATVS_OK : ATVS_ERR_LAUNCH;
  unsigned long long* level = static_cast<unsigned long long*>(scratch);
  hipLaunchKernelGGL(cloud_plane_moments_kernel, dim3((unsigned)moment_rows(m)), dim3(kThreads), 0, st, src, normals, dst, n, idx, d2, m, A,
                     moment_first(m, level, res));
  ATVS_LAUNCH_CHECK();
  return moment_fold<kPlaneSums>(m, level, res, st);
}

extern "C" int atvs_cloud_plane_moments_target_scratch_size(long m, long* bytes) {
  return atvs_cloud_plane_moments_scratch_size(m, bytes);                      // the same rows and tree
}

extern "C" int atvs_cloud_plane_moments_target(const float* src, const double* matrix12, const float* dst, const float* dst_normals, long n,
                                               const int* idx, const float* d2, long m, double trim, const double* pivot, void* scratch,
                                               long scratch_bytes, void* out, atvs_stream_t stream) {
  const double big = 1.7976931348623157e308;
  if (m < 0 || m > kMaxPoints || n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!out || !matrix12 || !pivot || (m > 0 && (!src || !idx || !d2 || !scratch)) || (m > 0 && n > 0 && (!dst || !dst_normals)))
    return ATVS_ERR_NULL;
  if (!(trim >= 0.0)) return ATVS_ERR_ARG;                  // NaN or negative; +inf is allowed
  PlaneTargetArgs A;
  A.trim2 = trim * trim;
  for (int k = 0; k < 12; ++k) {
    if (!(fabs(matrix12[k]) <= big)) return ATVS_ERR_ARG;
    A.t[k] = matrix12[k];
  }
  for (int k = 0; k < 3; ++k) {
    if (!(fabs(pivot[k]) <= big)) return ATVS_ERR_ARG;
    A.pivot[k] = pivot[k];
  }
  long need = 0;
  atvs_cloud_plane_moments_target_scratch_size(m, &need);
  if (m > 0 && scratch_bytes < need) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  unsigned long long* res = static_cast<unsigned long long*>(out);
  if (m == 0) return hipMemsetAsync(out, 0, kPlaneWords * 8, st) == hipSuccess ? ATVS_OK : ATVS_ERR_LAUNCH;
  unsigned long long* level = static_cast<unsigned long long*>(scratch);
  hipLaunchKernelGGL(cloud_plane_moments_target_kernel, dim3((unsigned)moment_rows(m)), dim3(kThreads), 0, st, src, dst, dst_normals, n, idx,
                     d2, m, A, moment_first(m, level, res));
  ATVS_LAUNCH_CHECK();
  return moment_fold<kPlaneSums>(m, level, res, st);
}

extern "C" int atvs_cloud_voxel_downsample_scratch_size(long n, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)voxel_layout(n).total;
  return ATVS_OK;
}

extern "C" int atvs_cloud_voxel_downsample(const float* points, long n, double voxel, const double* origin, void* scratch, long scratch_bytes,
                                           float* out_points, long long* out_count, int* out_first, atvs_stream_t stream) {
  if (n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  if (!origin || !out_count || (n > 0 && (!points || !scratch || !out_points || !out_first))) return ATVS_ERR_NULL;
  VoxelArgs A;
  if (!voxel_args(voxel, origin, &A)) return ATVS_ERR_ARG;
  hipStream_t st = as_stream(stream);
  if (n == 0) return hipMemsetAsync(out_count, 0, sizeof(long long), st) == hipSuccess ? ATVS_OK : ATVS_ERR_LAUNCH;
  const VoxelLayout L = voxel_layout(n);
  if (scratch_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  char* s = static_cast<char*>(scratch);
  VoxelTable T;
  if (!voxel_table(s, L.keys, L.zero, L.slot, st, &T)) return ATVS_ERR_LAUNCH;      // `first` lies behind the keys: all-ones too
  unsigned* first = reinterpret_cast<unsigned*>(s + L.first);
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(s + L.sums);
  unsigned* cnt = reinterpret_cast<unsigned*>(s + L.cnt);
  unsigned* flags = reinterpret_cast<unsigned*>(s + L.flags);
  if (hipMemsetAsync(s + L.zero, 0, L.slot - L.zero, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  const dim3 per_point((unsigned)cdiv(n, kThreads));
  hipLaunchKernelGGL(cloud_voxel_insert_kernel, per_point, dim3(kThreads), 0, st, points, n, A, L.slots, L.shift, T.keys, first, sums, cnt,
                     T.slot_of, T.err);
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cloud_voxel_flag_kernel, per_point, dim3(kThreads), 0, st, (const int*)T.slot_of, (const unsigned*)first, n, flags);
  ATVS_LAUNCH_CHECK();
  const int rc = exclusive_scan(flags, n + 1, reinterpret_cast<unsigned*>(s + L.tiles), st);      // flags[n] = 0 -> the number of voxels
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(cloud_voxel_emit_kernel, per_point, dim3(kThreads), 0, st, (const int*)T.slot_of, n, A,
                     (const unsigned long long*)T.keys, (const unsigned*)first, (const unsigned long long*)sums, (const unsigned*)cnt,
                     (const unsigned*)flags, (const int*)T.err, out_points, out_count, out_first);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_cloud_voxel_shares_scratch_size(long n, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n < 0 || n > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)share_layout(n).total;
  return ATVS_OK;
}

extern "C" int atvs_cloud_voxel_shares(const float* points, const float* d2, const float* excess, long n, double voxel, const double* origin,
                                       const double* tolerances, int n_tolerances, double margin, void* scratch, long scratch_bytes,
                                       long long* out, atvs_stream_t stream) {
  if (n < 0 || n > kMaxPoints || n_tolerances < 1 || n_tolerances > ATVS_CLOUD_MAX_TOLERANCES) return ATVS_ERR_SHAPE;
  if (!origin || !tolerances || !out || (n > 0 && (!points || !d2 || !scratch))) return ATVS_ERR_NULL;
  VoxelArgs A;
  if (!voxel_args(voxel, origin, &A) || margin != margin) return ATVS_ERR_ARG;
  for (int k = 0; k < n_tolerances; ++k)
    if (!(tolerances[k] >= 0.0)) return ATVS_ERR_ARG;        // NaN or negative; +inf is allowed
  const ShareLayout L = share_layout(n);
  if (n > 0 && scratch_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(out, 0, (size_t)n_tolerances * 4 * sizeof(long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n == 0) return ATVS_OK;
  char* s = static_cast<char*>(scratch);
  VoxelTable T;
  if (!voxel_table(s, L.keys, L.cnt, L.slot, st, &T)) return ATVS_ERR_LAUNCH;
  unsigned* cnt = reinterpret_cast<unsigned*>(s + L.cnt);
  const dim3 per_point((unsigned)cdiv(n, kThreads)), per_slot((unsigned)cdiv(L.slots, kThreads));
  hipLaunchKernelGGL(cloud_share_insert_kernel, per_point, dim3(kThreads), 0, st, points, n, A, L.slots, L.shift, T.keys, T.slot_of, T.err);
  ATVS_LAUNCH_CHECK();
  unsigned long long* res = reinterpret_cast<unsigned long long*>(out);
  for (int k0 = 0; k0 < n_tolerances; k0 += kSharePass) {
    ShareArgs S;
    S.margin = margin;
    S.count = n_tolerances - k0 < kSharePass ? n_tolerances - k0 : kSharePass;
    for (int k = 0; k < kSharePass; ++k) S.tau2[k] = k < S.count ? tolerances[k0 + k] * tolerances[k0 + k] : 0.0;
    if (hipMemsetAsync(s + L.cnt, 0, L.slot - L.cnt, st) != hipSuccess) return ATVS_ERR_LAUNCH;
    hipLaunchKernelGGL(cloud_share_count_kernel, per_point, dim3(kThreads), 0, st, (const int*)T.slot_of, d2, excess, n, S, cnt);
    ATVS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cloud_share_reduce_kernel, per_slot, dim3(kThreads), 0, st, (const unsigned long long*)T.keys, L.slots,
                       (const unsigned*)cnt, S.count, n_tolerances, (const int*)T.err, res + 4 * k0, res);
    ATVS_LAUNCH_CHECK();
  }
  return ATVS_OK;
}
