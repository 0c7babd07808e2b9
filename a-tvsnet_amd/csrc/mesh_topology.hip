// The connectivity of a triangle mesh (gfx950): connected components with their face and vertex counts, the selection of faces
// with the vertices compacted and the faces renumbered, and the exact edge census (atvsnet/clean_mesh.py, mesh_fusion.mesh_report).
// include/atvsnet_hip.h has the definitions, tests/mesh_topology_restated.py restates them.  Integer arithmetic and integer atomics
// only: the outputs are a function of the inputs alone, bit for bit on every run (DESIGN.md section 10.3a has the arguments).
//
//   components  union-find over parent (V,).  hook_kernel: one lane per face unites (v0,v1) and (v1,v2): both roots are found, the
//               LARGER is linked under the SMALLER by a 32-bit atomicCAS that expects the root to be its own parent, and a failed
//               CAS retries from the value it returned.  A parent only ever decreases (the CAS and find's atomicMin halving both
//               write a smaller index of the same component), so whatever the order of arrival the one vertex of a component that
//               stays its own parent is the component's smallest.  Inside the hook launch `parent` is read through atomics alone
//               (the CAS's return value, relaxed agent-scope loads): a plain load may return another XCD's stale line.
//               compress_kernel, a launch of its own, walks every vertex to its root; the dense ids are cloud_scan.h's
//               exclusive_scan over "is a root and is referenced"; the counts are integer atomicAdds, one per run of equal
//               components in a wave.  Every loop ends: find and compress walk strictly downward and stop at parent[p] == p.
//   select      two exclusive scans (kept faces, the vertices they name); vertices marked by plain stores of one value.
//   census      an open-addressing table of 64-bit keys (lo << 32) | hi, all-ones = empty, a power of two of at least 6F slots
//               (load <= 0.5), the start slot a mixed hash of the key.  A key is inserted by a 64-bit atomicCAS whose return value
//               is the only read of the slot; then one of the slot's two 32-bit counters is incremented: the pair came as (lo,hi)
//               or as (hi,lo).  The probe loop is bounded by the table size.  census_reduce_kernel walks the table and reduces
//               the words per workgroup before one atomic each: the totals do not depend on which slot a key landed in.
#include "common.h"
#include "cloud_scan.h"

namespace {

constexpr long kMaxFaces = ATVS_MESH_TOPOLOGY_MAX_FACES;
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kReduceBlocks = 2048;                           // workgroups of census_reduce_kernel at most: 8 per CU

__device__ __forceinline__ int load_parent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x: strictly downward (parent[x] < x off a root), so it ends.  On the way parent[x] is lowered to its grandparent:
// an atomicMin with a smaller member of the same component keeps every invariant of the hook.
__device__ __forceinline__ int find_root(int* __restrict__ parent, int x) {
  for (;;) {
    const int p = load_parent(parent + x);
    if (p == x) return x;
    const int g = load_parent(parent + p);
    if (g < p) atomicMin(parent + x, g);
    x = g;                                                    // g <= p < x
  }
}

__device__ __forceinline__ void unite(int* __restrict__ parent, int a, int b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicCAS(parent + a, a, b);              // a > b: the larger root under the smaller
    if (old == a) return;
    a = old;                                                  // somebody hooked a first: old < a, go on from there
  }
}

__device__ __forceinline__ bool in_range(int i, long n) { return i >= 0 && (long)i < n; }

__global__ __launch_bounds__(kThreads) void topo_init_kernel(int* __restrict__ parent, unsigned* __restrict__ ref, long n) {
  const long v = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (v >= n) return;
  parent[v] = (int)v;
  ref[v] = 0u;
}

__global__ __launch_bounds__(kThreads) void hook_kernel(const int* __restrict__ faces, long n_faces, long n_vertices,
                                                        int* __restrict__ parent, unsigned* __restrict__ ref, int* __restrict__ info) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (f >= n_faces) return;
  const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  if (!in_range(i0, n_vertices) || !in_range(i1, n_vertices) || !in_range(i2, n_vertices)) {
    atomicAdd(info, 1);
    return;
  }
  ref[i0] = 1u;                                               // plain stores of one value: any order gives the same word
  ref[i1] = 1u;
  ref[i2] = 1u;
  unite(parent, i0, i1);
  unite(parent, i1, i2);
}

// After the hook launch has ended: parent[v] = the root of v.  A lane may read a parent another lane has already compressed: old or
// new, it is an ancestor with a smaller index, and a root is only ever rewritten with itself.
__global__ __launch_bounds__(kThreads) void compress_kernel(int* parent, const unsigned* __restrict__ ref, unsigned* __restrict__ ids,
                                                            long n) {
  const long v = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (v > n) return;
  if (v == n) {
    ids[n] = 0u;                                              // the scan's last word: the number of components
    return;
  }
  int r = (int)v;
  for (;;) {
    const int p = parent[r];
    if (p == r) break;
    r = p;
  }
  parent[v] = r;
  ids[v] = (r == (int)v && ref[v] != 0u) ? 1u : 0u;
}

// counts[comp] += the number of lanes with this comp: one atomic per distinct component among a wave's first runs, then one per lane.
// Called by every lane of the wave (comp outside 0..limit-1, the words of counts: nothing to add).
__device__ __forceinline__ void wave_count(int* __restrict__ counts, int comp, int limit) {
  const int lane = threadIdx.x & 63;
  bool todo = comp >= 0 && comp < limit;
  for (int round = 0; round < 4; ++round) {
    const unsigned long long active = __ballot(todo);
    if (active == 0ull) return;                               // wave-uniform
    const int leader = __ffsll((long long)active) - 1;
    const int lc = __shfl(comp, leader);
    const bool same = todo && comp == lc;
    const unsigned long long mask = __ballot(same);
    if (lane == leader) atomicAdd(counts + lc, __popcll(mask));
    if (same) todo = false;
  }
  if (todo) atomicAdd(counts + comp, 1);
}

__global__ __launch_bounds__(kThreads) void label_vertices_kernel(const int* __restrict__ parent, const unsigned* __restrict__ ref,
                                                                  const unsigned* __restrict__ ids, long n, int* __restrict__ vertex_component,
                                                                  int* __restrict__ vertex_count, int limit, int* __restrict__ info) {
  const long v = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  int comp = -1;
  if (v < n) {
    if (ref[v] != 0u) comp = (int)ids[parent[v]];
    vertex_component[v] = comp;
  }
  if (v == 0) info[1] = (int)ids[n];
  wave_count(vertex_count, comp, limit);
}

__global__ __launch_bounds__(kThreads) void label_faces_kernel(const int* __restrict__ faces, long n_faces, long n_vertices,
                                                               const int* __restrict__ vertex_component, int* __restrict__ face_component,
                                                               int* __restrict__ face_count, int limit) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  int comp = -1;
  if (f < n_faces) {
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (in_range(i0, n_vertices) && in_range(i1, n_vertices) && in_range(i2, n_vertices)) comp = vertex_component[i0];
    face_component[f] = comp;                                 // -1 only beside an error word that is not 0
  }
  wave_count(face_count, comp, limit);
}

// ---------------------------------------------------------------------------------------------------------------------- select

__global__ __launch_bounds__(kThreads) void select_mark_kernel(const int* __restrict__ faces, const unsigned char* __restrict__ keep,
                                                               long n_faces, long n_vertices, unsigned* __restrict__ vflag,
                                                               unsigned* __restrict__ fflag, int* __restrict__ info) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (f > n_faces) return;
  unsigned kept = 0u;
  if (f < n_faces && keep[f] != 0) {
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (!in_range(i0, n_vertices) || !in_range(i1, n_vertices) || !in_range(i2, n_vertices)) {
      atomicAdd(info, 1);
    } else {
      kept = 1u;
      vflag[i0] = 1u;                                         // plain stores of one value
      vflag[i1] = 1u;
      vflag[i2] = 1u;
    }
  }
  fflag[f] = kept;                                            // fflag[n_faces] = 0: the scan's last word
}

__global__ __launch_bounds__(kThreads) void select_vertices_kernel(const unsigned* __restrict__ vertices, const unsigned char* __restrict__ colors,
                                                                   long n, const unsigned* __restrict__ vscan, const unsigned* __restrict__ fscan,
                                                                   long n_faces, unsigned* __restrict__ vertices_out,
                                                                   unsigned char* __restrict__ colors_out, int* __restrict__ vertex_map,
                                                                   int* __restrict__ info) {
  const long v = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (v == 0) {
    info[1] = (int)vscan[n];
    info[2] = (int)fscan[n_faces];
  }
  if (v >= n) return;
  const unsigned at = vscan[v];
  if (vscan[v + 1] == at) {
    vertex_map[v] = -1;
    return;
  }
  vertex_map[v] = (int)at;
  for (int k = 0; k < 3; ++k) vertices_out[(size_t)at * 3 + k] = vertices[(size_t)v * 3 + k];        // as bits: NaNs pass through
  if (colors)
    for (int k = 0; k < 3; ++k) colors_out[(size_t)at * 3 + k] = colors[(size_t)v * 3 + k];
}

__global__ __launch_bounds__(kThreads) void select_faces_kernel(const int* __restrict__ faces, long n_faces, const unsigned* __restrict__ vscan,
                                                                const unsigned* __restrict__ fscan, int* __restrict__ faces_out) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (f >= n_faces) return;
  const unsigned at = fscan[f];
  if (fscan[f + 1] == at) return;                             // not kept (or refused by select_mark_kernel)
  for (int k = 0; k < 3; ++k) faces_out[(size_t)at * 3 + k] = (int)vscan[faces[f * 3 + k]];
}

// ---------------------------------------------------------------------------------------------------------------------- census

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {      // the finaliser of MurmurHash3
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

__global__ __launch_bounds__(kThreads) void census_insert_kernel(const int* __restrict__ faces, long n_faces, long n_vertices,
                                                                 unsigned long long* __restrict__ keys, unsigned* __restrict__ counters,
                                                                 unsigned long long slots, unsigned long long* __restrict__ census) {
  const long f = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (f >= n_faces) return;
  const int i[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
  if (!in_range(i[0], n_vertices) || !in_range(i[1], n_vertices) || !in_range(i[2], n_vertices)) {
    atomicAdd(census + 7, 1ull);
    return;
  }
  const unsigned long long mask = slots - 1ull;
  for (int e = 0; e < 3; ++e) {
    const unsigned a = (unsigned)i[e], b = (unsigned)i[e == 2 ? 0 : e + 1];
    const unsigned lo = a <= b ? a : b, hi = a <= b ? b : a;
    const unsigned long long key = ((unsigned long long)lo << 32) | (unsigned long long)hi;   // never all-ones: hi < 2^30
    const unsigned long long start = mix64(key);
    bool placed = false;
    for (unsigned long long n = 0; n < slots; ++n) {          // bounded: at load <= 0.5 an empty slot always exists
      const unsigned long long slot = (start + n) & mask;
      const unsigned long long old = atomicCAS(keys + slot, kEmpty, key);
      if (old == kEmpty || old == key) {
        atomicAdd(counters + 2ull * slot + (a <= b ? 0u : 1u), 1u);
        placed = true;
        break;
      }
    }
    if (!placed) atomicAdd(census + 7, 1ull);
  }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_down((long long)v, off);
  return v;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long y = (unsigned long long)__shfl_down((long long)v, off);
    v = y > v ? y : v;
  }
  return v;
}

// census: edges, boundary, manifold, nonmanifold, misoriented, max_faces_per_edge, self_edges, error.
__global__ __launch_bounds__(kThreads) void census_reduce_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ counters,
                                                                 unsigned long long slots, unsigned long long* __restrict__ census) {
  __shared__ unsigned long long part[kThreads / 64][7];
  unsigned long long w[7] = {0, 0, 0, 0, 0, 0, 0};
  for (unsigned long long s = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; s < slots; s += (unsigned long long)gridDim.x * kThreads) {
    const unsigned long long key = keys[s];
    if (key == kEmpty) continue;
    const unsigned fwd = counters[2ull * s], bwd = counters[2ull * s + 1ull];
    const unsigned long long n = (unsigned long long)fwd + (unsigned long long)bwd;
    w[0] += 1ull;
    w[1] += n == 1ull ? 1ull : 0ull;
    w[2] += n == 2ull ? 1ull : 0ull;
    w[3] += n > 2ull ? 1ull : 0ull;
    w[4] += (fwd >= 2u || bwd >= 2u) ? 1ull : 0ull;
    w[5] = n > w[5] ? n : w[5];
    w[6] += (unsigned)(key >> 32) == (unsigned)(key & 0xffffffffull) ? 1ull : 0ull;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = 0; k < 7; ++k) {
    const unsigned long long r = k == 5 ? wave_max(w[k]) : wave_sum(w[k]);
    if (lane == 0) part[wv][k] = r;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    unsigned long long r = part[0][k];
    for (int j = 1; j < kThreads / 64; ++j) r = k == 5 ? (part[j][k] > r ? part[j][k] : r) : r + part[j][k];
    if (r != 0ull) {
      if (k == 5) atomicMax(census + k, r); else atomicAdd(census + k, r);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------- layouts

inline bool counts_ok(long n_vertices, long n_faces) {
  return n_vertices >= 0 && n_vertices <= kMaxPoints && n_faces >= 0 && n_faces <= kMaxFaces;
}

struct ComponentsLayout {
  size_t parent, ref, ids, tiles, total;
};

inline ComponentsLayout components_layout(long n_vertices) {
  ComponentsLayout L;
  L.parent = 0;
  L.ref = L.parent + align256((size_t)(n_vertices + 1) * sizeof(int));
  L.ids = L.ref + align256((size_t)(n_vertices + 1) * sizeof(unsigned));
  L.tiles = L.ids + align256((size_t)(n_vertices + 1) * sizeof(unsigned));
  L.total = L.tiles + align256((size_t)scan_tiles(n_vertices + 1) * sizeof(unsigned));
  return L;
}

struct SelectLayout {
  size_t vscan, fscan, tiles, total;
};

inline SelectLayout select_layout(long n_vertices, long n_faces) {
  SelectLayout L;
  const long most = n_vertices > n_faces ? n_vertices : n_faces;
  L.vscan = 0;
  L.fscan = L.vscan + align256((size_t)(n_vertices + 1) * sizeof(unsigned));
  L.tiles = L.fscan + align256((size_t)(n_faces + 1) * sizeof(unsigned));
  L.total = L.tiles + align256((size_t)scan_tiles(most + 1) * sizeof(unsigned));
  return L;
}

inline unsigned long long census_slots(long n_faces) {
  unsigned long long s = ATVS_MESH_CENSUS_MIN_SLOTS;
  while (s < 6ull * (unsigned long long)n_faces) s <<= 1;
  return s;
}

}  // namespace

extern "C" int atvs_mesh_components_scratch_size(long n_vertices, long n_faces, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (!counts_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  *bytes = (long)components_layout(n_vertices).total;
  return ATVS_OK;
}

extern "C" int atvs_mesh_components(const int* faces, long n_faces, long n_vertices, void* scratch, long scratch_bytes,
                                    int* vertex_component, int* face_component, int* face_count, int* vertex_count, int* info,
                                    atvs_stream_t stream) {
  if (!scratch || !info || !face_count || !vertex_count || (n_faces > 0 && (!faces || !face_component)) ||
      (n_vertices > 0 && !vertex_component))
    return ATVS_ERR_NULL;
  if (!counts_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  const ComponentsLayout L = components_layout(n_vertices);
  if (scratch_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  char* base = static_cast<char*>(scratch);
  int* parent = reinterpret_cast<int*>(base + L.parent);
  unsigned* ref = reinterpret_cast<unsigned*>(base + L.ref);
  unsigned* ids = reinterpret_cast<unsigned*>(base + L.ids);
  unsigned* tiles = reinterpret_cast<unsigned*>(base + L.tiles);
  const long most = n_vertices < n_faces ? n_vertices : n_faces;            // a component has a face and a vertex of its own
  const int limit = (int)(most > 0 ? most : 1);                             // the words of face_count and vertex_count
  const size_t count_bytes = (size_t)limit * sizeof(int);
  if (hipMemsetAsync(info, 0, 2 * sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(face_count, 0, count_bytes, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(vertex_count, 0, count_bytes, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_vertices > 0) {
    hipLaunchKernelGGL(topo_init_kernel, dim3((unsigned)cdiv(n_vertices, kThreads)), dim3(kThreads), 0, st, parent, ref, n_vertices);
    ATVS_LAUNCH_CHECK();
  }
  if (n_faces > 0) {
    hipLaunchKernelGGL(hook_kernel, dim3((unsigned)cdiv(n_faces, kThreads)), dim3(kThreads), 0, st, faces, n_faces, n_vertices, parent,
                       ref, info);
    ATVS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(compress_kernel, dim3((unsigned)cdiv(n_vertices + 1, kThreads)), dim3(kThreads), 0, st, parent,
                     (const unsigned*)ref, ids, n_vertices);
  ATVS_LAUNCH_CHECK();
  const int rc = exclusive_scan(ids, n_vertices + 1, tiles, st);
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(label_vertices_kernel, dim3((unsigned)cdiv(n_vertices + 1, kThreads)), dim3(kThreads), 0, st, (const int*)parent,
                     (const unsigned*)ref, (const unsigned*)ids, n_vertices, vertex_component, vertex_count, limit, info);
  ATVS_LAUNCH_CHECK();
  if (n_faces > 0) {
    hipLaunchKernelGGL(label_faces_kernel, dim3((unsigned)cdiv(n_faces, kThreads)), dim3(kThreads), 0, st, faces, n_faces, n_vertices,
                       (const int*)vertex_component, face_component, face_count, limit);
    ATVS_LAUNCH_CHECK();
  }
  return ATVS_OK;
}

extern "C" int atvs_mesh_select_scratch_size(long n_vertices, long n_faces, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (!counts_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  *bytes = (long)select_layout(n_vertices, n_faces).total;
  return ATVS_OK;
}

extern "C" int atvs_mesh_select(const float* vertices, const void* colors, long n_vertices, const int* faces, const void* keep,
                                long n_faces, void* scratch, long scratch_bytes, float* vertices_out, void* colors_out, int* faces_out,
                                int* vertex_map, int* info, atvs_stream_t stream) {
  if (!scratch || !info || (n_faces > 0 && (!faces || !keep || !faces_out)) ||
      (n_vertices > 0 && (!vertices || !vertices_out || !vertex_map || (colors && !colors_out))))
    return ATVS_ERR_NULL;
  if (!counts_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  const SelectLayout L = select_layout(n_vertices, n_faces);
  if (scratch_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  char* base = static_cast<char*>(scratch);
  unsigned* vscan = reinterpret_cast<unsigned*>(base + L.vscan);
  unsigned* fscan = reinterpret_cast<unsigned*>(base + L.fscan);
  unsigned* tiles = reinterpret_cast<unsigned*>(base + L.tiles);
  if (hipMemsetAsync(info, 0, 3 * sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(vscan, 0, (size_t)(n_vertices + 1) * sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  hipLaunchKernelGGL(select_mark_kernel, dim3((unsigned)cdiv(n_faces + 1, kThreads)), dim3(kThreads), 0, st, faces,
                     static_cast<const unsigned char*>(keep), n_faces, n_vertices, vscan, fscan, info);
  ATVS_LAUNCH_CHECK();
  int rc = exclusive_scan(vscan, n_vertices + 1, tiles, st);
  if (rc != ATVS_OK) return rc;
  rc = exclusive_scan(fscan, n_faces + 1, tiles, st);
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(select_vertices_kernel, dim3((unsigned)cdiv(n_vertices > 0 ? n_vertices : 1, kThreads)), dim3(kThreads), 0, st,
                     reinterpret_cast<const unsigned*>(vertices), static_cast<const unsigned char*>(colors), n_vertices,
                     (const unsigned*)vscan, (const unsigned*)fscan, n_faces, reinterpret_cast<unsigned*>(vertices_out),
                     static_cast<unsigned char*>(colors_out), vertex_map, info);
  ATVS_LAUNCH_CHECK();
  if (n_faces > 0) {
    hipLaunchKernelGGL(select_faces_kernel, dim3((unsigned)cdiv(n_faces, kThreads)), dim3(kThreads), 0, st, faces, n_faces,
                       (const unsigned*)vscan, (const unsigned*)fscan, faces_out);
    ATVS_LAUNCH_CHECK();
  }
  return ATVS_OK;
}

extern "C" int atvs_mesh_edge_census_scratch_size(long n_faces, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n_faces < 0 || n_faces > kMaxFaces) return ATVS_ERR_SHAPE;
  *bytes = (long)(census_slots(n_faces) * 16ull);
  return ATVS_OK;
}

extern "C" int atvs_mesh_edge_census(const int* faces, long n_faces, long n_vertices, void* scratch, long scratch_bytes, long* census,
                                     atvs_stream_t stream) {
  if (!scratch || !census || (n_faces > 0 && !faces)) return ATVS_ERR_NULL;
  if (!counts_ok(n_vertices, n_faces)) return ATVS_ERR_SHAPE;
  const unsigned long long slots = census_slots(n_faces);
  if (scratch_bytes < (long)(slots * 16ull)) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  unsigned long long* keys = static_cast<unsigned long long*>(scratch);
  unsigned* counters = reinterpret_cast<unsigned*>(keys + slots);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(census);
  if (hipMemsetAsync(words, 0, 8 * sizeof(unsigned long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (n_faces == 0) return ATVS_OK;
  if (hipMemsetAsync(keys, 0xFF, (size_t)slots * sizeof(unsigned long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(counters, 0, (size_t)slots * 2 * sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  hipLaunchKernelGGL(census_insert_kernel, dim3((unsigned)cdiv(n_faces, kThreads)), dim3(kThreads), 0, st, faces, n_faces, n_vertices, keys,
                     counters, slots, words);
  ATVS_LAUNCH_CHECK();
  const unsigned long long wanted = (slots + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(census_reduce_kernel, dim3((unsigned)(wanted < (unsigned long long)kReduceBlocks ? wanted : kReduceBlocks)),
                     dim3(kThreads), 0, st, (const unsigned long long*)keys, (const unsigned*)counters, slots, words);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
