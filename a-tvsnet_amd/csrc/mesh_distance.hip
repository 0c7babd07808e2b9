// Exact point-to-triangle distances from a cloud to a mesh's surface (gfx950): a uniform grid of FACE REFERENCES over the mesh, and per
// query the smallest squared distance to a face within a radius, the lowest face that attains it and the closest point on it
// (ops/mesh_distance.py, atvsnet/mesh_distance.py, atvsnet/eval_cloud.py --exact_recon / --exact_gt).  include/atvsnet_hip.h has the
// definition operation by operation, tests/mesh_distance_restated.py restates it, DESIGN.md section 10.3f has the arguments.
// Built with -ffp-contract=off: every operation below is rounded on its own.  Integer atomics only (bit patterns' maxima, counters,
// returning adds for slots): the order of the references inside a cell depends on who arrives first and CANNOT be seen in a result,
// because a query takes the 64-bit minimum of (bits(d2) << 32) | face over whatever it meets, and d2 is a function of (query, face).
//
// THE GRID.  Face f is usable when its three indices are inside 0..V-1 and its nine coordinates are finite; its corners are copied
// into the grid as three 16-byte records (the search gathers 48 contiguous bytes per candidate and never reads the caller's mesh
// again).  The box is the bounding box of the usable faces' corners, the cell edge h >= max(R (1 + 2^-18), `cell`, 2^-60), made
// larger by the rule of cloud.hip where the box would need more cells than cell_cap(n_faces).  A usable face is referenced from every
// cell of the box [cell(min corner), cell(max corner)] of its own corners (cell_coord of cloud_grid.h, the queries' own quotient):
//   faces    one lane per face by stride: usable?, the records, the box by integer atomic max on ordered bit patterns;
//   params   one thread: origin, h, cells per axis;
//   cells    one lane per face by stride: lo cell, spans, count = nx ny nz -> off[f]; the total by a 64-bit atomic add;
//   decide   one thread: built = total <= max_refs; the four info words;
//   scan     off -> exclusive offsets (cloud_scan.h); pair p of [off[f], off[f + 1]) is face f's cell number p - off[f];
//   count    one lane per PAIR by stride (a face of a million cells is a million lanes' work, not one lane's): the face by binary
//            search over off, the cell, one atomic add on the cell's counter;
//   scan     the cells' counters -> starts;
//   scatter  one lane per pair again: a returning atomic add on the cell's start is the slot of the reference.
// Where total > max_refs nothing after `decide` runs (every later kernel reads the flag): the caller asks again with a larger `cell`.
//
// WHY 27 CELLS SUFFICE.  cloud.hip's argument with two changes.  (1) The point that must lie in a neighbouring cell is the closest
// point x on the face, not a vertex: x is a convex combination of the corners (every parameter below is clamped to [0, 1] or is a
// ratio of positive numbers to their sum), so each coordinate lies between the face's minimum and maximum up to a few roundings of
// 2^-53 relative to the coordinates, and cell_coord is monotone: x's cell lies inside the face's box of cells, which references the
// face.  (2) d2 is formed in double and rounded once: the float32 d2 is within 2^-24 relative of the double one, which is within
// a few 2^-53 |coordinate|^2 of the true squared distance to x.  The margin is therefore 2^-18 instead of 2^-20: D / h <=
// (1 + 2^-23) / (1 + 2^-18) < 1 - 2^-19, which leaves the two quotient roundings of 2^-23 and the 2^-53-relative terms at up to 2^28
// cells per axis (2^-25 of a cell) with room to spare.  A larger h only searches more.
//
// THE QUERY.  The queries are sorted by the grid's cells with cloud_grid.h's counting sort; one lane per query in cell order walks
// the 27 cells around it as 9 contiguous runs of references and keeps the 64-bit minimum and the closest point of the face that set
// it in registers.  A face met again from another cell gives the same key.  No face is skipped.
#include <math.h>

#include "common.h"
#include "cloud_grid.h"

namespace {

constexpr long kMaxFaces = ATVS_MESH_TOPOLOGY_MAX_FACES;
constexpr long kMaxRefs = ATVS_MESH_GRID_MAX_REFS;
constexpr int kStrideBlocks = 2048;                    // workgroups of the per-face kernels: eight per CU, the rest by stride
constexpr int kPairBlocks = 8192;                      // ... of the per-pair kernels

struct MeshHeader {                                    // the first kHeaderBytes of a mesh grid: cloud_grid.h's header in front
  GridHeader g;
  unsigned long long total;                            // references the cell edge needs
  unsigned long long usable;                           // usable faces
  int built;                                           // total <= max_refs: the references are there
};
static_assert(sizeof(MeshHeader) <= kHeaderBytes, "header");

// header | S (cap + 2 cell counters) | refs (max_refs faces) | off (n_faces + 1) | cells (n_faces x int4) | tri (n_faces x 3 float4) | tiles
struct MeshLayout {
  size_t S, refs, off, cells, tri, tiles, total;
};
inline MeshLayout mesh_layout(long n_faces, long max_refs) {
  const long cap = cell_cap(n_faces);
  MeshLayout L;
  L.S = kHeaderBytes;
  L.refs = L.S + align256((size_t)(cap + 2) * sizeof(unsigned));
  L.off = L.refs + align256((size_t)max_refs * sizeof(int));
  L.cells = L.off + align256((size_t)(n_faces + 1) * sizeof(unsigned));
  L.tri = L.cells + align256((size_t)n_faces * sizeof(int4));
  L.tiles = L.tri + align256((size_t)n_faces * 3 * sizeof(float4));
  const long longest = cap + 1 > n_faces + 1 ? cap + 1 : n_faces + 1;
  L.total = L.tiles + align256((size_t)scan_tiles(longest) * sizeof(unsigned));
  return L;
}

__device__ __forceinline__ bool in_range(int i, long n) { return i >= 0 && (long)i < n; }

// usable?, the corners' records (w of the first: 1 usable, 0 not), the box of the usable faces' corners, their number
__global__ __launch_bounds__(kThreads) void mesh_faces_kernel(const float* __restrict__ vertices, long n_vertices,
                                                              const int* __restrict__ faces, long n_faces, float4* __restrict__ tri,
                                                              MeshHeader* __restrict__ hdr) {
  unsigned m[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  unsigned n_usable = 0u;
  for (long f = (long)blockIdx.x * kThreads + threadIdx.x; f < n_faces; f += (long)gridDim.x * kThreads) {
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool ok = in_range(i0, n_vertices) & in_range(i1, n_vertices) & in_range(i2, n_vertices);
    if (ok) {
      for (int k = 0; k < 3; ++k) {
        v[k] = vertices[(long)i0 * 3 + k];
        v[3 + k] = vertices[(long)i1 * 3 + k];
        v[6 + k] = vertices[(long)i2 * 3 + k];
      }
      ok = finite3(v[0], v[1], v[2]) & finite3(v[3], v[4], v[5]) & finite3(v[6], v[7], v[8]);
    }
    if (ok) {
      ++n_usable;
      for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) {
          m[k] = max(m[k], ~enc(v[c * 3 + k]));
          m[3 + k] = max(m[3 + k], enc(v[c * 3 + k]));
        }
    } else {
      for (int k = 0; k < 9; ++k) v[k] = 0.f;
    }
    tri[f * 3 + 0] = make_float4(v[0], v[1], v[2], ok ? 1.f : 0.f);
    tri[f * 3 + 1] = make_float4(v[3], v[4], v[5], 0.f);
    tri[f * 3 + 2] = make_float4(v[6], v[7], v[8], 0.f);
  }
  for (int k = 0; k < 6; ++k) {
    unsigned x = m[k];
    for (int off = 32; off > 0; off >>= 1) x = max(x, (unsigned)__shfl_xor((int)x, off));
    if ((threadIdx.x & 63) == 0 && x) atomicMax(hdr->g.box + k, x);
  }
  for (int off = 32; off > 0; off >>= 1) n_usable += (unsigned)__shfl_xor((int)n_usable, off);
  if ((threadIdx.x & 63) == 0 && n_usable) atomicAdd(&hdr->usable, (unsigned long long)n_usable);
}

// cloud.hip's cloud_params_kernel with the mesh grid's margin and the caller's lower bound on the cell edge
__global__ void mesh_params_kernel(MeshHeader* __restrict__ hdr, float radius, double cell, long cap) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  GridHeader g = hdr->g;
  g.r2 = (double)radius * (double)radius;
  double h = fmax(fmax((double)radius * (1.0 + 0x1p-18), cell), 0x1p-60);
  if (g.box[3] == 0u) {                                    // no usable face: one empty cell
    g.origin[0] = g.origin[1] = g.origin[2] = 0.0;
    g.dims[0] = g.dims[1] = g.dims[2] = 1;
  } else {
    float hi[3];
    for (int k = 0; k < 3; ++k) {
      g.origin[k] = (double)dec(~g.box[k]);
      hi[k] = dec(g.box[3 + k]);
    }
    double d[3];
    for (int it = 0;; ++it) {
      for (int k = 0; k < 3; ++k) d[k] = cell_coord(hi[k], g.origin[k], h) + 1.0;
      const double cells = d[0] * d[1] * d[2];
      if (cells <= (double)cap) break;
      if (it == 256) {                                     // cannot happen for finite boxes; one cell is always right
        h = 2.0 * fmax(fmax((double)hi[0] - g.origin[0], (double)hi[1] - g.origin[1]), (double)hi[2] - g.origin[2]);
        continue;
      }
      h *= 1.01 * fmax(cbrt(cells / (double)cap), 1.0);
    }
    for (int k = 0; k < 3; ++k) g.dims[k] = (int)d[k];
  }
  g.h = h;
  g.ncells = g.dims[0] * g.dims[1] * g.dims[2];
  hdr->g = g;
}

// per usable face: the lowest cell of its box, the box's spans in x and y, and off[f] = the number of its cells
__global__ __launch_bounds__(kThreads) void mesh_cells_kernel(const float4* __restrict__ tri, long n_faces, MeshHeader* __restrict__ hdr,
                                                              int4* __restrict__ cells, unsigned* __restrict__ off) {
  const GridHeader g = hdr->g;
  unsigned long long sum = 0ull;
  for (long f = (long)blockIdx.x * kThreads + threadIdx.x; f < n_faces; f += (long)gridDim.x * kThreads) {
    const float4 a = tri[f * 3 + 0], b = tri[f * 3 + 1], c = tri[f * 3 + 2];
    unsigned count = 0u;
    int4 box = make_int4(0, 0, 0, 0);
    if (a.w != 0.f) {
      int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
      cell_of(g, fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z), &lo[0], &lo[1], &lo[2]);
      cell_of(g, fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z), &hi[0], &hi[1], &hi[2]);
      for (int k = 0; k < 3; ++k) {                        // inside the grid by construction; held there whatever the header says
        lo[k] = min(max(lo[k], 0), g.dims[k] - 1);
        hi[k] = min(max(hi[k], lo[k]), g.dims[k] - 1);
      }
      const int nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
      count = (unsigned)((long)nx * ny * nz);              // <= ncells <= 2^28
      box = make_int4((lo[2] * g.dims[1] + lo[1]) * g.dims[0] + lo[0], nx, ny, nz);
    }
    cells[f] = box;
    off[f] = count;
    sum += count;
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&hdr->total, sum);
}

__global__ void mesh_decide_kernel(MeshHeader* __restrict__ hdr, long max_refs, long long* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int built = hdr->total <= (unsigned long long)max_refs ? 1 : 0;
  hdr->built = built;
  info[0] = (long long)hdr->total;
  info[1] = built;
  info[2] = (long long)hdr->usable;
  info[3] = __double_as_longlong(hdr->g.h);
}

// The face f in [0, n_faces) with off[f] <= p < off[f + 1], given off[0] = 0 <= p < off[n_faces].
__device__ __forceinline__ long pair_face(const unsigned* __restrict__ off, long n_faces, unsigned p) {
  long lo = 0, hi = n_faces;
  while (hi - lo > 1) {
    const long mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// Scatter = false: one add on the counter of every pair's cell.  Scatter = true: the returning add on the cell's start is the slot.
template <bool Scatter>
__global__ __launch_bounds__(kThreads) void mesh_pairs_kernel(const MeshHeader* __restrict__ hdr, const unsigned* __restrict__ off,
                                                              const int4* __restrict__ cells, long n_faces, long max_refs,
                                                              unsigned* __restrict__ C, int* __restrict__ refs) {
  if (!hdr->built) return;
  const unsigned long long total = hdr->total;             // <= max_refs < 2^31
  const int d0 = hdr->g.dims[0], d1 = hdr->g.dims[1], ncells = hdr->g.ncells;
  for (unsigned long long p = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; p < total;
       p += (unsigned long long)gridDim.x * kThreads) {
    const long f = pair_face(off, n_faces, (unsigned)p);
    const int4 box = cells[f];
    const unsigned j = (unsigned)p - off[f];
    if (box.y <= 0 || box.z <= 0 || j >= (unsigned)((long)box.y * box.z * box.w)) continue;      // cannot happen: off is the boxes' own scan
    const int jx = (int)(j % (unsigned)box.y), jy = (int)((j / (unsigned)box.y) % (unsigned)box.z), jz = (int)(j / ((unsigned)box.y * (unsigned)box.z));
    const int cell = box.x + (jz * d1 + jy) * d0 + jx;
    if (cell < 0 || cell >= ncells) continue;              // cannot happen: the box lies inside the grid
    const unsigned pos = atomicAdd(C + cell, 1u);
    if (Scatter && pos < (unsigned)max_refs) refs[pos] = (int)f;
  }
}

__device__ __forceinline__ double dot3(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// The closest point of the segment X + t e, t in [0, 1], to p, and its squared distance (the header's "segment rule").
__device__ __forceinline__ double segment_point(const double* p, const double* X, const double* Y, double* x) {
  double e[3], w[3], r[3];
  for (int k = 0; k < 3; ++k) {
    e[k] = Y[k] - X[k];
    w[k] = p[k] - X[k];
  }
  const double den = dot3(e, e), num = dot3(w, e);
  double t = den > 0.0 ? num / den : 0.0;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  for (int k = 0; k < 3; ++k) {
    x[k] = X[k] + t * e[k];
    r[k] = p[k] - x[k];
  }
  return dot3(r, r);
}

// The header's sequence: the closest point x of the closed triangle (a, b, c) to p; returns the double squared distance.
__device__ __forceinline__ double closest_point(const double* p, const double* a, const double* b, const double* c, double* x) {
  double ab[3], ac[3], ap[3], bp[3], cp[3];
  for (int k = 0; k < 3; ++k) {
    ab[k] = b[k] - a[k];
    ac[k] = c[k] - a[k];
    ap[k] = p[k] - a[k];
    bp[k] = p[k] - b[k];
    cp[k] = p[k] - c[k];
  }
  const double n0 = ab[1] * ac[2] - ab[2] * ac[1], n1 = ab[2] * ac[0] - ab[0] * ac[2], n2 = ab[0] * ac[1] - ab[1] * ac[0];
  const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double s = (va + vb) + vc;
  bool done = false;
  if (!(n0 == 0.0 && n1 == 0.0 && n2 == 0.0)) {
    done = true;
    if (d1 <= 0.0 && d2 <= 0.0) {
      for (int k = 0; k < 3; ++k) x[k] = a[k];
    } else if (d3 >= 0.0 && d4 <= d3) {
      for (int k = 0; k < 3; ++k) x[k] = b[k];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
      const double den = d1 - d3, t = den > 0.0 ? d1 / den : 0.0;
      for (int k = 0; k < 3; ++k) x[k] = a[k] + t * ab[k];
    } else if (d6 >= 0.0 && d5 <= d6) {
      for (int k = 0; k < 3; ++k) x[k] = c[k];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
      const double den = d2 - d6, t = den > 0.0 ? d2 / den : 0.0;
      for (int k = 0; k < 3; ++k) x[k] = a[k] + t * ac[k];
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
      const double u = d4 - d3, den = u + (d5 - d6), t = den > 0.0 ? u / den : 0.0;
      for (int k = 0; k < 3; ++k) x[k] = b[k] + t * (c[k] - b[k]);
    } else if (s > 0.0) {
      const double v = vb / s, w = vc / s;
      for (int k = 0; k < 3; ++k) x[k] = (a[k] + v * ab[k]) + w * ac[k];
    } else {
      done = false;
    }
  }
  if (!done) {                                             // the segment rule: AB, AC, BC, the first smallest
    double y[3];
    double best = segment_point(p, a, b, x);
    double dd = segment_point(p, a, c, y);
    if (dd < best) {
      best = dd;
      for (int k = 0; k < 3; ++k) x[k] = y[k];
    }
    dd = segment_point(p, b, c, y);
    if (dd < best) {
      for (int k = 0; k < 3; ++k) x[k] = y[k];
    }
  }
  double r[3];
  for (int k = 0; k < 3; ++k) r[k] = p[k] - x[k];
  return dot3(r, r);
}

__global__ __launch_bounds__(kThreads) void mesh_nearest_kernel(const MeshHeader* __restrict__ hdr, const unsigned* __restrict__ S,
                                                                const int* __restrict__ refs, const float4* __restrict__ tri,
                                                                long n_faces, long max_refs, const unsigned* __restrict__ qS,
                                                                const float4* __restrict__ qrec, long m, float* __restrict__ d2out,
                                                                int* __restrict__ faceout, float* __restrict__ closest) {
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const GridHeader g = hdr->g;
  const float4 q = qrec[j];
  const int orig = __float_as_int(q.w);
  const unsigned long long none = (0x7f800000ull << 32) | 0xffffffffull;
  unsigned long long best = none;
  double bx[3] = {0.0, 0.0, 0.0};
  if (hdr->built && j < (long)qS[g.ncells]) {               // not in the bucket of far / non-finite queries
    const double p[3] = {(double)q.x, (double)q.y, (double)q.z};
    int cx, cy, cz;
    cell_of(g, q.x, q.y, q.z, &cx, &cy, &cz);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dims[0] - 1);
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.dims[2] - 1); ++z) {
      for (int y = max(cy - 1, 0); y <= min(cy + 1, g.dims[1] - 1); ++y) {
        const int row = (z * g.dims[1] + y) * g.dims[0];
        const unsigned b = S[row + x0];
        const unsigned e = min(S[row + x1 + 1], (unsigned)max_refs);
        for (unsigned r = b; r < e; ++r) {
          const int f = refs[r];
          if (!in_range(f, n_faces)) continue;             // cannot happen: the build wrote every slot below the total
          const float4 ta = tri[(long)f * 3 + 0], tb = tri[(long)f * 3 + 1], tc = tri[(long)f * 3 + 2];
          const double a[3] = {(double)ta.x, (double)ta.y, (double)ta.z};
          const double bb[3] = {(double)tb.x, (double)tb.y, (double)tb.z};
          const double c[3] = {(double)tc.x, (double)tc.y, (double)tc.z};
          double x[3];
          const float d2 = (float)closest_point(p, a, bb, c, x);
          const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)f;
          if (key < best) {
            best = key;
            bx[0] = x[0];
            bx[1] = x[1];
            bx[2] = x[2];
          }
        }
      }
    }
  }
  float d2 = __uint_as_float((unsigned)(best >> 32));
  int face = (int)(unsigned)(best & 0xffffffffull);
  const bool found = best != none && (double)d2 <= g.r2;
  if (!found) {
    d2 = __uint_as_float(0x7f800000u);
    face = -1;
  }
  d2out[orig] = d2;
  faceout[orig] = face;
  if (closest) {
    const float nan = __uint_as_float(0x7fc00000u);
    for (int k = 0; k < 3; ++k) closest[(long)orig * 3 + k] = found ? (float)bx[k] : nan;
  }
}

inline bool sizes_ok(long n_vertices, long n_faces, long max_refs) {
  return n_vertices >= 0 && n_vertices <= kMaxPoints && n_faces >= 0 && n_faces <= kMaxFaces && max_refs >= 0 && max_refs <= kMaxRefs;
}

}  // namespace

extern "C" int atvs_mesh_grid_scratch_size(long n_faces, long max_refs, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (!sizes_ok(0, n_faces, max_refs)) return ATVS_ERR_SHAPE;
  *bytes = (long)mesh_layout(n_faces, max_refs).total;
  return ATVS_OK;
}

extern "C" int atvs_mesh_grid_build(const float* vertices, long n_vertices, const int* faces, long n_faces, float radius, double cell,
                                    long max_refs, void* grid, long grid_bytes, long* info, atvs_stream_t stream) {
  if (!sizes_ok(n_vertices, n_faces, max_refs)) return ATVS_ERR_SHAPE;
  if (!(radius > 0.f) || !(radius <= 3.4028234663852886e38f) || !(cell >= 0.0) || !(cell < (double)INFINITY)) return ATVS_ERR_ARG;
  if (max_refs < 8 * n_faces) return ATVS_ERR_ARG;           // what a cell edge of the box's extent needs: the coarsening ends there
  if (!grid || !info || (n_faces > 0 && (!faces || (n_vertices > 0 && !vertices)))) return ATVS_ERR_NULL;
  const MeshLayout L = mesh_layout(n_faces, max_refs);
  if (grid_bytes < (long)L.total) return ATVS_ERR_SHAPE;
  const long cap = cell_cap(n_faces);
  hipStream_t st = as_stream(stream);
  char* base = static_cast<char*>(grid);
  MeshHeader* hdr = reinterpret_cast<MeshHeader*>(base);
  unsigned* S = reinterpret_cast<unsigned*>(base + L.S);
  unsigned* C = S + 1;                                       // S[0] stays 0: cell c is references S[c] .. S[c + 1] after the scatter
  int* refs = reinterpret_cast<int*>(base + L.refs);
  unsigned* off = reinterpret_cast<unsigned*>(base + L.off);
  int4* cells = reinterpret_cast<int4*>(base + L.cells);
  float4* tri = reinterpret_cast<float4*>(base + L.tri);
  unsigned* tiles = reinterpret_cast<unsigned*>(base + L.tiles);
  if (hipMemsetAsync(grid, 0, kHeaderBytes, st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(S, 0, (size_t)(cap + 2) * sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(off + n_faces, 0, sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  const dim3 per_face((unsigned)(cdiv(n_faces, kThreads) < kStrideBlocks ? cdiv(n_faces, kThreads) : kStrideBlocks));
  if (n_faces > 0) {
    hipLaunchKernelGGL(mesh_faces_kernel, per_face, dim3(kThreads), 0, st, vertices, n_vertices, faces, n_faces, tri, hdr);
    ATVS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mesh_params_kernel, dim3(1), dim3(64), 0, st, hdr, radius, cell, cap);
  ATVS_LAUNCH_CHECK();
  if (n_faces > 0) {
    hipLaunchKernelGGL(mesh_cells_kernel, per_face, dim3(kThreads), 0, st, (const float4*)tri, n_faces, hdr, cells, off);
    ATVS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mesh_decide_kernel, dim3(1), dim3(64), 0, st, hdr, max_refs, reinterpret_cast<long long*>(info));
  ATVS_LAUNCH_CHECK();
  if (n_faces == 0) return ATVS_OK;
  int rc = exclusive_scan(off, n_faces + 1, tiles, st);
  if (rc != ATVS_OK) return rc;
  const dim3 per_pair((unsigned)(cdiv(max_refs, kThreads) < kPairBlocks ? cdiv(max_refs, kThreads) : kPairBlocks));
  hipLaunchKernelGGL(mesh_pairs_kernel<false>, per_pair, dim3(kThreads), 0, st, (const MeshHeader*)hdr, (const unsigned*)off,
                     (const int4*)cells, n_faces, max_refs, C, refs);
  ATVS_LAUNCH_CHECK();
  rc = exclusive_scan(C, cap + 1, tiles, st);
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(mesh_pairs_kernel<true>, per_pair, dim3(kThreads), 0, st, (const MeshHeader*)hdr, (const unsigned*)off,
                     (const int4*)cells, n_faces, max_refs, C, refs);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_mesh_nearest_scratch_size(long n_faces, long m, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (n_faces < 0 || n_faces > kMaxFaces || m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  *bytes = (long)layout_for(cell_cap(n_faces), m, 0).total;
  return ATVS_OK;
}

extern "C" int atvs_mesh_nearest(const void* grid, long grid_bytes, long n_faces, long max_refs, const float* queries, long m,
                                 void* scratch, long scratch_bytes, float* d2, int* face, float* closest, atvs_stream_t stream) {
  if (!sizes_ok(0, n_faces, max_refs) || m < 0 || m > kMaxPoints) return ATVS_ERR_SHAPE;
  if (m == 0) return ATVS_OK;
  if (!grid || !queries || !scratch || !d2 || !face) return ATVS_ERR_NULL;
  const long cap = cell_cap(n_faces);
  const MeshLayout L = mesh_layout(n_faces, max_refs);
  const Layout Q = layout_for(cap, m, 0);
  if (grid_bytes < (long)L.total || scratch_bytes < (long)Q.total) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  const char* g = static_cast<const char*>(grid);
  const MeshHeader* hdr = reinterpret_cast<const MeshHeader*>(g);
  char* q = static_cast<char*>(scratch);
  const int rc = counting_sort(queries, m, &hdr->g, q, Q, cap, st);
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(mesh_nearest_kernel, dim3((unsigned)cdiv(m, kThreads)), dim3(kThreads), 0, st, hdr,
                     reinterpret_cast<const unsigned*>(g + L.S), reinterpret_cast<const int*>(g + L.refs),
                     reinterpret_cast<const float4*>(g + L.tri), n_faces, max_refs, reinterpret_cast<const unsigned*>(q + Q.S),
                     reinterpret_cast<const float4*>(q + Q.rec), m, d2, face, closest);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}
