// A surface from depth maps (gfx950): a block-sparse truncated-signed-distance volume integrated from a scene's depth maps, and the
// marching-tetrahedra extractor that turns it into an indexed, coloured triangle mesh (the definitions are in
// include/atvsnet_hip.h, restated in tests/tsdf_restated.py; ops/tsdf.py and atvsnet/mesh_fusion.py are built on it).
//
// The volume is a box of bx x by x bz blocks of 8^3 voxels.  Which blocks exist is decided by MARKING: one lane per pixel and view
// forms the box of the pixel's frustum between d - trunc and d + trunc, padded by a voxel, and stores a 1 into a dense directory
// word of every block the box meets (plain vector stores of one value: no atomic).  A voxel that a view contributes to projects
// into that pixel with its depth inside the segment, so it lies in the hull of the segment's corners: marking is conservative, and
// because a view outside the narrow band adds nothing to a voxel, the integrated values do not depend on what else was marked.  The
// directory is scanned (cloud_scan.h: integers, exact) into slots; a second marking pass ORs each view's bit into the slot's view mask
// (64-bit vector atomics on integers: order-free).  INTEGRATE runs one workgroup per slot and one lane per voxel: the slot's mask is
// read once and made wave-uniform, so the view loop and the cameras' 16 doubles are scalar, each lane keeps its five float64 sums in
// registers, projects through scan_project.h (the one float64 projection) and gathers one depth and three colour words per
// contributing view.  A per-slot any-weight flag is scanned and the non-empty slots gathered into the result.  No float atomics:
// the same inputs give the same bits.
// What bounds integrate: per (voxel, view of the mask) ~40 float64 operations with two divisions and one 4-byte gather that lands
// in the L2 (a block's voxels look at a few neighbouring pixels of a map); which of the two dominates is what tools_dev/mesh_rate.py
// measures.
// FREE-SPACE CARVING (opt-in, atvs_tsdf_integrate_carve): a view whose depth lies beyond a voxel's band has seen past the voxel and
// pulls its value outside.  Such a view is in no band mask, so atvs_tsdf_free_views gives every slot the views that can see into
// its block at all (a ballot per mask word), and the kernel's second form loops over band | free.
// VIEW WEIGHTS (opt-in, atvs_tsdf_integrate_weighted): every pixel of every view carries a float32 weight that replaces the 1 a
// sample counts for (fusion_support.hip makes one from the fusion's agreement count); the kernel's third form, with or without carving.
//
// The extractor splits the cube of every voxel whose eight corners are valid into six Kuhn tetrahedra (one per permutation of the
// axes), which tile space by translation: neighbouring cubes agree on their shared faces without a special case.  Every vertex
// lives on one of seven edge types owned by the edge's lower voxel.  Four passes over the blocks, one lane per voxel, neighbour
// blocks found by binary search in the ascending block list: (1) cube validity and face counts, (2) the edges that cross the
// surface and belong to a meshed cube, (3) vertices, (4) faces, between them two exclusive scans.  A face finds a neighbour's vertex
// as that voxel's start + the rank of the edge type among its set bits.
#include "common.h"
#include "scan_project.h"
#include "cloud_scan.h"

#include <math.h>

namespace {

constexpr int kVox = 512;                               // voxels of a block, [z][y][x]
constexpr long kMaxDirectory = ATVS_TSDF_MAX_DIRECTORY;
constexpr long kMaxMeshBlocks = ATVS_TSDF_MAX_MESH_BLOCKS;
constexpr int kMaxPixelBlocks = ATVS_TSDF_MAX_PIXEL_BLOCKS;

struct TsdfBox {
  double ox, oy, oz, voxel;
  int bx, by, bz;
};

__host__ __device__ inline bool finite_d(double v) { return fabs(v) < (double)INFINITY; }

static inline int check_box(const double* origin, double voxel, int bx, int by, int bz, TsdfBox* B) {
  if (!origin) return ATVS_ERR_NULL;
  if (bx < 1 || by < 1 || bz < 1) return ATVS_ERR_SHAPE;
  if ((double)bx * (double)by * (double)bz > (double)kMaxDirectory) return ATVS_ERR_SHAPE;
  if (!(voxel > 0.0) || !finite_d(voxel) || !finite_d(origin[0]) || !finite_d(origin[1]) || !finite_d(origin[2])) return ATVS_ERR_ARG;
  B->ox = origin[0];
  B->oy = origin[1];
  B->oz = origin[2];
  B->voxel = voxel;
  B->bx = bx;
  B->by = by;
  B->bz = bz;
  return ATVS_OK;
}

// entry i of an exclusive scan of 0/1 flags (or counts) as the count it came from
__device__ __forceinline__ unsigned scanned_count(const unsigned* __restrict__ a, long i, long count, unsigned total) {
  return (i + 1 < count ? a[i + 1] : total) - a[i];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Marking.  slots == nullptr: store 1 into dir[] of every block the pixel's padded frustum box meets.  Otherwise dir[] holds the
// slots and the view's bit is ORed into the slot's mask words.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tsdf_mark_kernel(const float* __restrict__ depths, const double* __restrict__ cams, int n,
                                                             int rows, int cols, TsdfBox B, double trunc, double pixel_centre,
                                                             unsigned* __restrict__ dir, unsigned long long* __restrict__ masks,
                                                             int words, int* __restrict__ err) {
  const long plane = (long)rows * cols;
  const long p = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (p >= plane * n) return;
  const int view = (int)(p / plane);
  const int pix = (int)(p - (long)view * plane);
  const int v = pix / cols, u = pix - v * cols;
  const float d = depths[p];
  if (!(d > 0.f && d < INFINITY)) return;
  const double* __restrict__ c = cams + (size_t)view * kCam;
  const double z0 = fmax((double)d - trunc, 0.0), z1 = (double)d + trunc;
  // the inverse of the camera's 3x3 by cofactors (a camera may carry its intrinsics inside it: no transpose); its rounding is far
  // below the voxel the box is padded by, and a singular matrix gives no finite box
  const double a00 = c[4] * c[8] - c[5] * c[7], a01 = c[2] * c[7] - c[1] * c[8], a02 = c[1] * c[5] - c[2] * c[4];
  const double a10 = c[5] * c[6] - c[3] * c[8], a11 = c[0] * c[8] - c[2] * c[6], a12 = c[2] * c[3] - c[0] * c[5];
  const double a20 = c[3] * c[7] - c[4] * c[6], a21 = c[1] * c[6] - c[0] * c[7], a22 = c[0] * c[4] - c[1] * c[3];
  const double det = (c[0] * a00 + c[1] * a10) + c[2] * a20;
  double lo[3] = {(double)INFINITY, (double)INFINITY, (double)INFINITY};
  double hi[3] = {-(double)INFINITY, -(double)INFINITY, -(double)INFINITY};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double x = ((double)u + pixel_centre) + ((k & 1) ? 0.5 : -0.5);
    const double y = ((double)v + pixel_centre) + ((k & 2) ? 0.5 : -0.5);
    const double z = (k & 4) ? z1 : z0;
    const double w0 = ((x - c[14]) / c[12]) * z - c[9];
    const double w1 = ((y - c[15]) / c[13]) * z - c[10];
    const double w2 = z - c[11];
    const double P[3] = {((a00 * w0 + a01 * w1) + a02 * w2) / det, ((a10 * w0 + a11 * w1) + a12 * w2) / det,
                         ((a20 * w0 + a21 * w1) + a22 * w2) / det};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fmin(lo[a], P[a]);        // fmin drops a NaN: the check below then meets the infinity that is left, or the others' box
      hi[a] = fmax(hi[a], P[a]);
    }
  }
  const double org[3] = {B.ox, B.oy, B.oz};
  const int nb[3] = {B.bx, B.by, B.bz};
  const double edge = 8.0 * B.voxel;
  int l[3], h[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double fl = floor(((lo[a] - B.voxel) - org[a]) / edge), fh = floor(((hi[a] + B.voxel) - org[a]) / edge);
    if (!(finite_d(fl) && finite_d(fh))) return;                                 // a corner at infinity or not a number: no box
    if (!(fh >= 0.0 && fl <= (double)(nb[a] - 1))) return;                       // outside the volume: compared in double
    fl = fmax(fl, 0.0);
    fh = fmin(fh, (double)(nb[a] - 1));
    l[a] = (int)fl;
    h[a] = (int)fh;
  }
  const long met = (long)(h[0] - l[0] + 1) * (long)(h[1] - l[1] + 1) * (long)(h[2] - l[2] + 1);
  if (met > kMaxPixelBlocks) {
    *err = 1;                           // every lane that gets here stores the same word
    return;
  }
  const unsigned long long bit = 1ull << (view & 63);
  for (int z = l[2]; z <= h[2]; ++z)
    for (int y = l[1]; y <= h[1]; ++y)
      for (int x = l[0]; x <= h[0]; ++x) {
        const size_t lin = ((size_t)z * B.by + y) * B.bx + x;
        if (masks == nullptr)
          dir[lin] = 1u;
        else {
          // most pixels of a view find their bit set already: look first (a stale look only costs the atomic it would have saved)
          unsigned long long* word = masks + (size_t)dir[lin] * words + (view >> 6);
          if ((*(volatile unsigned long long*)word & bit) == 0ull) atomicOr(word, bit);
        }
      }
}

__global__ __launch_bounds__(kThreads) void tsdf_coords_kernel(const unsigned* __restrict__ dir, long nbk, unsigned total, int bx, int by,
                                                               int* __restrict__ coords) {
  const long i = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  if (i >= nbk) return;
  if (scanned_count(dir, i, nbk, total) == 0u) return;
  const unsigned s = dir[i];
  const long zy = i / bx;
  coords[(size_t)s * 3 + 0] = (int)(i - zy * bx);
  coords[(size_t)s * 3 + 1] = (int)(zy % by);
  coords[(size_t)s * 3 + 2] = (int)(zy / by);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Integration: one workgroup per slot, one lane per voxel.
// ---------------------------------------------------------------------------------------------------------------------------------
// kCarve (free-space carving): the view loop runs over band mask | free mask, a view whose depth lies
// beyond the band (sdf > trunc) adds 1 to a sixth sum Wf, and the epilogue forms (S + cw Wf) / (W + cw Wf) and writes `free`.
// Without it every added line is compiled out: the plain form is the code it was.
// kWeighted (per-pixel view weights; the third form, always with kCarve): the pixel a view lands on carries a
// float32 weight w; the view is a sample only when w > 0 and w is finite, and it adds w where the other forms add 1 -- w * (sdf /
// trunc) to S, w to W, w * image[c] to C, w to Wf.  Whether this form carves is decided at run time (free_masks == nullptr: the view
// loop runs over the band mask alone, the epilogue is the plain one, `free` is not written); the branch is uniform over the launch.
// `weights` is the kernel's LAST parameter, so the two older forms keep their kernel-argument offsets, and they compile every
// weighted line out.
template <bool kCarve, bool kWeighted>
__global__ __launch_bounds__(kVox) void tsdf_integrate_kernel(const float* __restrict__ depths, const float* __restrict__ images, int ch,
                                                              const double* __restrict__ cams, int rows, int cols, TsdfBox B, double trunc,
                                                              double pixel_centre, const int* __restrict__ coords,
                                                              const unsigned long long* __restrict__ masks, int words,
                                                              float* __restrict__ tsdf, float* __restrict__ weight,
                                                              float* __restrict__ color, unsigned* __restrict__ any,
                                                              const unsigned long long* __restrict__ free_masks, double cw,
                                                              float* __restrict__ freev, const float* __restrict__ weights) {
  static_assert(kCarve || !kWeighted, "the weighted form is built on the carving form");
  [[maybe_unused]] const bool carving = !kWeighted || free_masks != nullptr;      // kWeighted: uniform over the launch; otherwise a constant
  const size_t slot = blockIdx.x;
  const int t = threadIdx.x;
  const int gx = coords[slot * 3 + 0] * 8 + (t & 7), gy = coords[slot * 3 + 1] * 8 + ((t >> 3) & 7), gz = coords[slot * 3 + 2] * 8 + (t >> 6);
  const double X = B.ox + ((double)gx + 0.5) * B.voxel;
  const double Y = B.oy + ((double)gy + 0.5) * B.voxel;
  const double Z = B.oz + ((double)gz + 0.5) * B.voxel;
  const size_t plane = (size_t)rows * cols;
  double S = 0.0, W = 0.0, C0 = 0.0, C1 = 0.0, C2 = 0.0;
  double Wf = 0.0;                                      // kCarve only: the views that saw past this voxel
  for (int w = 0; w < words; ++w) {
    unsigned long long m = masks[slot * words + w];
    if constexpr (kCarve) {
      if (carving) m |= free_masks[slot * words + w];
    }
    for (int half = 0; half < 2; ++half) {
      unsigned mm = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(half ? m >> 32 : m));      // wave-uniform: scalar loop
      while (mm) {
        const int view = w * 64 + half * 32 + __builtin_ctz(mm);
        mm &= mm - 1u;
        ScanProjection P;
        if (!scan_project(cams + (size_t)view * kCam, X, Y, Z, pixel_centre, 0.0, (double)cols, (double)rows, &P)) continue;
        const size_t pix = (size_t)view * plane + (size_t)((int)floor(P.ys)) * cols + (size_t)((int)floor(P.xs));
        const float d = depths[pix];
        if (!(d > 0.f && d < INFINITY)) continue;
        [[maybe_unused]] double wv = 1.0;               // kWeighted only: this pixel's weight
        if constexpr (kWeighted) {
          const float wp = weights[pix];
          if (!(wp > 0.f && wp < INFINITY)) continue;   // 0, negative, NaN, +inf: the view is no sample here, it neither adds nor carves
          wv = (double)wp;
        }
        const double sdf = (double)d - P.c2;
        if (!(sdf >= -trunc && sdf <= trunc)) {
          if constexpr (kCarve) {
            // free: the view looks through the voxel; sdf < -trunc (occluded) adds nothing
            if constexpr (kWeighted) {
              if (carving && sdf > trunc) Wf += wv;
            } else {
              if (sdf > trunc) Wf += 1.0;
            }
          }
          continue;
        }
        if constexpr (kWeighted) {
          S += wv * (sdf / trunc);
          W += wv;
        } else {
          S += sdf / trunc;
          W += 1.0;
        }
        if (images != nullptr) {
          const float* __restrict__ px = images + pix * ch;
          if constexpr (kWeighted) {
            C0 += wv * (double)px[0];
            C1 += wv * (double)px[1];
            C2 += wv * (double)px[2];
          } else {
            C0 += (double)px[0];
            C1 += (double)px[1];
            C2 += (double)px[2];
          }
        }
      }
    }
  }
  const bool has = W > 0.0;
  const size_t o = slot * kVox + t;
  if constexpr (kWeighted) {
    if (carving) {
      const double f = cw * Wf;                         // formed once
      tsdf[o] = has ? (float)((S + f) / (W + f)) : 0.f;
      freev[o] = has ? (float)Wf : 0.f;
    } else {
      tsdf[o] = has ? (float)(S / W) : 0.f;
    }
  } else if constexpr (kCarve) {
    const double f = cw * Wf;                           // formed once
    tsdf[o] = has ? (float)((S + f) / (W + f)) : 0.f;
    freev[o] = has ? (float)Wf : 0.f;
  } else {
    tsdf[o] = has ? (float)(S / W) : 0.f;
  }
  weight[o] = (float)W;
  if (color != nullptr) {
    color[o * 3 + 0] = has ? (float)(C0 / W) : 0.f;
    color[o * 3 + 1] = has ? (float)(C1 / W) : 0.f;
    color[o * 3 + 2] = has ? (float)(C2 / W) : 0.f;
  }
  const int some = __syncthreads_or(has ? 1 : 0);
  if (t == 0) any[slot] = some ? 1u : 0u;
}

__global__ __launch_bounds__(kVox) void tsdf_gather_kernel(const int* __restrict__ coords, const float* __restrict__ tsdf,
                                                           const float* __restrict__ weight, const float* __restrict__ color,
                                                           const unsigned* __restrict__ keep, long count, unsigned kept,
                                                           int* __restrict__ coords_out, float* __restrict__ tsdf_out,
                                                           float* __restrict__ weight_out, float* __restrict__ color_out,
                                                           const float* __restrict__ freev, float* __restrict__ free_out) {
  const size_t slot = blockIdx.x;
  if (scanned_count(keep, (long)slot, count, kept) == 0u) return;
  const size_t dst = keep[slot];
  const int t = threadIdx.x;
  if (t < 3) coords_out[dst * 3 + t] = coords[slot * 3 + t];
  tsdf_out[dst * kVox + t] = tsdf[slot * kVox + t];
  weight_out[dst * kVox + t] = weight[slot * kVox + t];
  if (freev != nullptr) free_out[dst * kVox + t] = freev[slot * kVox + t];
  if (color != nullptr)
    for (int c = 0; c < 3; ++c) color_out[dst * kVox * 3 + c * kVox + t] = color[slot * kVox * 3 + c * kVox + t];     // 1536 words, coalesced
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Which views can see into a block (free-space carving): one wavefront per (slot, mask word), one lane per view; the ballot of the 64
// lanes is the word (no atomic).  A lane projects the eight corners of the block's cube in scan_project's operation order.  No corner
// in front of the camera: clear.  Some in front and some not, or a NaN among xs, ys: set.  All in front: the cube's image lies in the
// hull of the corners' images, so the bit is set iff their bounding box, padded by a pixel, meets the image.  Depths are not read.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kFreeWaves = 4;                           // wavefronts of a workgroup
constexpr long kFreeMaxGroups = 1L << 20;               // beyond this the wavefronts stride over the (slot, word) items

__global__ __launch_bounds__(64 * kFreeWaves) void tsdf_free_views_kernel(const int* __restrict__ coords, long count,
                                                                          const double* __restrict__ cams, int n, int rows, int cols,
                                                                          TsdfBox B, double pixel_centre,
                                                                          unsigned long long* __restrict__ masks, int words) {
  const int lane = threadIdx.x & 63;
  const long items = count * words;
  const long first = (long)blockIdx.x * kFreeWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (long item = first; item < items; item += (long)gridDim.x * kFreeWaves) {      // wave-uniform: every lane reaches the ballot
    const long slot = item / words;
    const int view = (int)(item - slot * words) * 64 + lane;
    bool set = false;
    if (view < n) {                                     // the lanes beyond the last view vote 0
      const double* __restrict__ c = cams + (size_t)view * kCam;
      const int b0 = coords[slot * 3 + 0], b1 = coords[slot * 3 + 1], b2 = coords[slot * 3 + 2];
      int pos = 0;
      bool nan = false;
      double lox = (double)INFINITY, hix = -(double)INFINITY, loy = (double)INFINITY, hiy = -(double)INFINITY;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const double X = B.ox + (double)(8 * (b0 + (k & 1))) * B.voxel;
        const double Y = B.oy + (double)(8 * (b1 + ((k >> 1) & 1))) * B.voxel;
        const double Z = B.oz + (double)(8 * (b2 + (k >> 2))) * B.voxel;
        const double c2 = ((c[6] * X + c[7] * Y) + c[8] * Z) + c[11];
        if (!(c2 > 0.0)) continue;                      // behind the camera, on its plane, or NaN
        ++pos;
        const double c0 = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[9];
        const double c1 = ((c[3] * X + c[4] * Y) + c[5] * Z) + c[10];
        const double x = (c0 / c2) * c[12] + c[14];
        const double y = (c1 / c2) * c[13] + c[15];
        const double xs = (x - pixel_centre) + 0.5;
        const double ys = (y - pixel_centre) + 0.5;
        nan = nan || xs != xs || ys != ys;
        lox = fmin(lox, xs);
        hix = fmax(hix, xs);
        loy = fmin(loy, ys);
        hiy = fmax(hiy, ys);
      }
      if (pos == 8 && !nan)
        set = hix >= -1.0 && lox < (double)cols + 1.0 && hiy >= -1.0 && loy < (double)rows + 1.0;
      else
        set = pos > 0;
    }
    const unsigned long long word = __ballot(set ? 1 : 0);
    if (lane == 0) masks[item] = word;
  }
}

// exclusive scan in place with its total: last = the last counter before, + the last entry after
__global__ void tsdf_total_kernel(const unsigned* __restrict__ a, long count, long long* __restrict__ total, int after) {
  if (threadIdx.x == 0 && blockIdx.x == 0) total[0] = (after ? total[0] : 0ll) + (long long)a[count - 1];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Marching tetrahedra.  Corners of a cube are coded dx + 2 dy + 4 dz.  The tetrahedron of the axis permutation (a, b, c) has the
// local vertices 0 = corner 0, 1 = +e_a, 2 = +e_a + e_b, 3 = corner 7: ascending local order is ascending in every coordinate, so the
// lower local vertex of an edge is the edge's owner.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kPerms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};      // read in constant evaluation only

constexpr unsigned long long make_perm_bits() {          // per permutation six bits: the corner codes of local vertices 1 and 2
  unsigned long long v = 0ull;
  for (int p = 0; p < 6; ++p) {
    const unsigned long long c1 = 1ull << kPerms[p][0], c2 = c1 | (1ull << kPerms[p][1]);
    v |= (c1 | (c2 << 3)) << (6 * p);
  }
  return v;
}
constexpr unsigned long long kPermBits = make_perm_bits();

__host__ __device__ constexpr int perm_code(int p, int q) {                  // the corner code of local vertex q of permutation p
  return q == 0 ? 0 : q == 3 ? 7 : (int)((kPermBits >> (6 * p + 3 * (q - 1))) & 7ull);
}

// The triangles of one tetrahedron for each of the 16 inside masks (bit q: local vertex q inside), oriented: entry = the number of
// triangles << 24 | triangle k's three edges in bits 12 k + 4 j (lower local vertex | upper << 2).  The orientation is derived, not
// tabulated: with every crossing at its edge's midpoint the normal must not point against (centroid of the outside corners - centroid
// of the inside corners); otherwise the last two vertices are swapped.  Integer arithmetic in half-voxel units: exact.
struct TetTable {
  unsigned v[96];
};

constexpr TetTable make_tet_table() {
  TetTable T{};
  for (int p = 0; p < 6; ++p)
    for (int mask = 0; mask < 16; ++mask) {
      int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
      for (int q = 0; q < 4; ++q) {
        if ((mask >> q) & 1)
          in[ni++] = q;
        else
          out[no++] = q;
      }
      int tri[2][3][2] = {};
      int nt = 0;
      if (ni == 2) {
        const int a = in[0], b = in[1], c = out[0], d = out[1];
        const int t0[3][2] = {{a, c}, {a, d}, {b, d}}, t1[3][2] = {{a, c}, {b, d}, {b, c}};
        for (int j = 0; j < 3; ++j)
          for (int e = 0; e < 2; ++e) {
            tri[0][j][e] = t0[j][e];
            tri[1][j][e] = t1[j][e];
          }
        nt = 2;
      } else if (ni == 1 || ni == 3) {
        const int s = ni == 1 ? in[0] : out[0];
        int k = 0;
        for (int q = 0; q < 4; ++q)
          if (q != s) {
            tri[0][k][0] = s;
            tri[0][k][1] = q;
            ++k;
          }
        nt = 1;
      }
      int dir[3] = {0, 0, 0};                          // ni * sum(outside) - no * sum(inside): the centroids' difference times ni * no
      for (int a = 0; a < 3; ++a) {
        int so = 0, si = 0;
        for (int k = 0; k < no; ++k) so += (perm_code(p, out[k]) >> a) & 1;
        for (int k = 0; k < ni; ++k) si += (perm_code(p, in[k]) >> a) & 1;
        dir[a] = ni * so - no * si;
      }
      unsigned entry = (unsigned)nt << 24;
      for (int k = 0; k < nt; ++k) {
        int m[3][3] = {};
        for (int j = 0; j < 3; ++j)
          for (int a = 0; a < 3; ++a) m[j][a] = ((perm_code(p, tri[k][j][0]) >> a) & 1) + ((perm_code(p, tri[k][j][1]) >> a) & 1);
        const int u[3] = {m[1][0] - m[0][0], m[1][1] - m[0][1], m[1][2] - m[0][2]};
        const int w[3] = {m[2][0] - m[0][0], m[2][1] - m[0][1], m[2][2] - m[0][2]};
        const int nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
        const bool flip = nx * dir[0] + ny * dir[1] + nz * dir[2] < 0;
        for (int j = 0; j < 3; ++j) {
          const int src = flip ? (j == 0 ? 0 : 3 - j) : j;
          const int x0 = tri[k][src][0], x1 = tri[k][src][1];
          const int lo = x0 < x1 ? x0 : x1, hi = x0 < x1 ? x1 : x0;
          entry |= (unsigned)(lo | (hi << 2)) << (12 * k + 4 * j);
        }
      }
      T.v[p * 16 + mask] = entry;
    }
  return T;
}

__constant__ TetTable kTet = make_tet_table();

// edge type of an offset code: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) = 0..6, a nibble per code
constexpr unsigned kEdgeType = 0x65423100u;
__device__ __forceinline__ int edge_type(int code) { return (int)((kEdgeType >> (4 * code)) & 7u); }
__device__ __forceinline__ int edge_code(int e) { return (int)((0x7653421u >> (4 * e)) & 7u); }      // ... and back

__device__ int find_block(const int* __restrict__ blocks, int nb, int bx, int by, int bz, int x, int y, int z) {
  if (x < 0 || y < 0 || z < 0 || x >= bx || y >= by || z >= bz) return -1;
  const int key = (z * by + y) * bx + x;
  int lo = 0, hi = nb - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const int k = (blocks[mid * 3 + 2] * by + blocks[mid * 3 + 1]) * bx + blocks[mid * 3 + 0];
    if (k == key) return mid;
    if (k < key)
      lo = mid + 1;
    else
      hi = mid - 1;
  }
  return -1;
}

// the 27 blocks around this workgroup's block, [dz + 1][dy + 1][dx + 1], into LDS
__device__ __forceinline__ void load_neighbours(const int* __restrict__ blocks, int nb, int bx, int by, int bz, int* nbr) {
  const int t = threadIdx.x, b = blockIdx.x;
  if (t < 27)
    nbr[t] = find_block(blocks, nb, bx, by, bz, blocks[b * 3 + 0] + t % 3 - 1, blocks[b * 3 + 1] + (t / 3) % 3 - 1, blocks[b * 3 + 2] + t / 9 - 1);
  __syncthreads();
}

// voxel (i, j, k) relative to this block, each in -8..15 -> its index in the block-major arrays, or -1 where the block is missing
__device__ __forceinline__ long voxel_at(const int* nbr, int i, int j, int k) {
  const int s = nbr[((k >> 3) + 1) * 9 + ((j >> 3) + 1) * 3 + ((i >> 3) + 1)];        // >> of a negative int: arithmetic, -1
  return s < 0 ? -1L : (long)s * kVox + ((k & 7) * 64 + (j & 7) * 8 + (i & 7));
}

__global__ __launch_bounds__(kVox) void tsdf_cubes_kernel(const int* __restrict__ blocks, int nb, int bx, int by, int bz,
                                                          const float* __restrict__ tsdf, const float* __restrict__ weight, float min_weight,
                                                          unsigned char* __restrict__ cube_ok, unsigned* __restrict__ fcount) {
  __shared__ int nbr[27];
  load_neighbours(blocks, nb, bx, by, bz, nbr);
  const int t = threadIdx.x, i = t & 7, j = (t >> 3) & 7, k = t >> 6;
  bool ok = true;
  unsigned in8 = 0u;
  for (int c = 0; c < 8; ++c) {
    const long g = voxel_at(nbr, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2));
    if (g < 0 || !(weight[g] >= min_weight)) {
      ok = false;
      break;
    }
    in8 |= (tsdf[g] < 0.f ? 1u : 0u) << c;
  }
  unsigned faces = 0u;
  if (ok && in8 != 0u && in8 != 255u)
    for (int p = 0; p < 6; ++p) {
      unsigned in4 = 0u;
      for (int q = 0; q < 4; ++q) in4 |= ((in8 >> perm_code(p, q)) & 1u) << q;
      faces += kTet.v[p * 16 + in4] >> 24;
    }
  const size_t o = (size_t)blockIdx.x * kVox + t;
  cube_ok[o] = ok ? 1 : 0;
  fcount[o] = faces;
}

__global__ __launch_bounds__(kVox) void tsdf_edges_kernel(const int* __restrict__ blocks, int nb, int bx, int by, int bz,
                                                          const float* __restrict__ tsdf, const unsigned char* __restrict__ cube_ok,
                                                          unsigned char* __restrict__ emask, unsigned* __restrict__ vcount) {
  __shared__ int nbr[27];
  load_neighbours(blocks, nb, bx, by, bz, nbr);
  const int t = threadIdx.x, i = t & 7, j = (t >> 3) & 7, k = t >> 6;
  const size_t o = (size_t)blockIdx.x * kVox + t;
  const bool in_a = tsdf[o] < 0.f;
  unsigned m = 0u;
  for (int e = 0; e < 7; ++e) {
    const int code = edge_code(e);
    const int dx = code & 1, dy = (code >> 1) & 1, dz = code >> 2;
    bool used = false;                                  // a meshed cube that has both endpoints among its corners
    for (int sz = 0; sz <= 1 - dz; ++sz)
      for (int sy = 0; sy <= 1 - dy; ++sy)
        for (int sx = 0; sx <= 1 - dx; ++sx) {
          const long g = voxel_at(nbr, i - sx, j - sy, k - sz);
          if (g >= 0 && cube_ok[g]) used = true;
        }
    if (!used) continue;
    const long g = voxel_at(nbr, i + dx, j + dy, k + dz);
    if (g < 0) continue;                                // cannot be: a meshed cube's corners exist
    if ((tsdf[g] < 0.f) != in_a) m |= 1u << e;
  }
  emask[o] = (unsigned char)m;
  vcount[o] = (unsigned)__popc(m);
}

__global__ __launch_bounds__(kVox) void tsdf_vertices_kernel(const int* __restrict__ blocks, int nb, int bx, int by, int bz, TsdfBox B,
                                                             const float* __restrict__ tsdf, const float* __restrict__ color,
                                                             const unsigned char* __restrict__ emask, const unsigned* __restrict__ vstart,
                                                             float* __restrict__ vertices, unsigned char* __restrict__ colors) {
  __shared__ int nbr[27];
  load_neighbours(blocks, nb, bx, by, bz, nbr);
  const int t = threadIdx.x, i = t & 7, j = (t >> 3) & 7, k = t >> 6;
  const size_t o = (size_t)blockIdx.x * kVox + t;
  const unsigned m = emask[o];
  if (m == 0u) return;
  const int g[3] = {blocks[blockIdx.x * 3 + 0] * 8 + i, blocks[blockIdx.x * 3 + 1] * 8 + j, blocks[blockIdx.x * 3 + 2] * 8 + k};
  const double org[3] = {B.ox, B.oy, B.oz};
  const double fa = (double)tsdf[o];
  size_t out = vstart[o];
  for (int e = 0; e < 7; ++e) {
    if (!((m >> e) & 1u)) continue;
    const int code = edge_code(e);
    const int d[3] = {code & 1, (code >> 1) & 1, code >> 2};
    const long q = voxel_at(nbr, i + d[0], j + d[1], k + d[2]);
    const double fb = (double)tsdf[q];
    const double tt = fa / (fa - fb);
    for (int a = 0; a < 3; ++a) {
      const double pa = org[a] + ((double)g[a] + 0.5) * B.voxel;
      const double pb = org[a] + ((double)(g[a] + d[a]) + 0.5) * B.voxel;
      vertices[out * 3 + a] = (float)(pa + tt * (pb - pa));
    }
    if (color != nullptr)
      for (int c = 0; c < 3; ++c) {
        const double ca = (double)color[o * 3 + c], cb = (double)color[(size_t)q * 3 + c];
        double v = floor((ca + tt * (cb - ca)) + 0.5);
        v = v >= 0.0 ? v : 0.0;                         // a NaN goes to 0
        v = v <= 255.0 ? v : 255.0;
        colors[out * 3 + (2 - c)] = (unsigned char)(int)v;      // b, g, r -> r, g, b
      }
    ++out;
  }
}

__global__ __launch_bounds__(kVox) void tsdf_faces_kernel(const int* __restrict__ blocks, int nb, int bx, int by, int bz,
                                                          const float* __restrict__ tsdf, const unsigned char* __restrict__ emask,
                                                          const unsigned* __restrict__ vstart, const unsigned* __restrict__ fstart,
                                                          long voxels, unsigned total_faces, int* __restrict__ faces) {
  __shared__ int nbr[27];
  __shared__ unsigned s_vs[7][kVox];                    // per corner 0..6 (corner 7 owns no edge of this cube): its vertices' start
  __shared__ unsigned char s_em[7][kVox];               // ... and its edge mask
  load_neighbours(blocks, nb, bx, by, bz, nbr);
  const int t = threadIdx.x, i = t & 7, j = (t >> 3) & 7, k = t >> 6;
  const size_t o = (size_t)blockIdx.x * kVox + t;
  if (scanned_count(fstart, (long)o, voxels, total_faces) == 0u) return;          // no barrier follows: each lane reads its own column
  unsigned in8 = 0u;
  for (int c = 0; c < 8; ++c) {
    const long g = voxel_at(nbr, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2));    // a cube with faces is meshed: its corners exist
    in8 |= (tsdf[g] < 0.f ? 1u : 0u) << c;
    if (c < 7) {
      s_vs[c][t] = vstart[g];
      s_em[c][t] = emask[g];
    }
  }
  size_t f = fstart[o];
  for (int p = 0; p < 6; ++p) {
    unsigned in4 = 0u, codes = 0u;
    for (int q = 0; q < 4; ++q) {
      in4 |= ((in8 >> perm_code(p, q)) & 1u) << q;
      codes |= (unsigned)perm_code(p, q) << (3 * q);
    }
    const unsigned entry = kTet.v[p * 16 + in4];
    const int nt = (int)(entry >> 24);
    for (int n = 0; n < nt; ++n) {
      int idx[3];
      for (int e = 0; e < 3; ++e) {
        const unsigned pair = (entry >> (12 * n + 4 * e)) & 15u;
        const int cl = (int)((codes >> (3 * (pair & 3u))) & 7u), ch = (int)((codes >> (3 * (pair >> 2))) & 7u);
        const int type = edge_type(cl ^ ch);
        idx[e] = (int)(s_vs[cl][t] + (unsigned)__popc((unsigned)s_em[cl][t] & ((1u << type) - 1u)));
      }
      int a = idx[0], b = idx[1], c = idx[2];
      if (b < a && b <= c) {                            // the smallest index first, the cyclic order kept
        const int x = a;
        a = b;
        b = c;
        c = x;
      } else if (c < a && c < b) {
        const int x = c;
        c = b;
        b = a;
        a = x;
      }
      faces[f * 3 + 0] = a;
      faces[f * 3 + 1] = b;
      faces[f * 3 + 2] = c;
      ++f;
    }
  }
}

static inline int check_blocks(int nb, int bx, int by, int bz) {
  if (bx < 1 || by < 1 || bz < 1 || nb < 0) return ATVS_ERR_SHAPE;
  if ((double)bx * (double)by * (double)bz > (double)kMaxDirectory) return ATVS_ERR_SHAPE;
  if ((long)nb > kMaxMeshBlocks || (long)nb > (long)bx * by * bz) return ATVS_ERR_SHAPE;
  return ATVS_OK;
}

}  // namespace

extern "C" int atvs_tsdf_scan_scratch_size(long count, long* bytes) {
  if (!bytes) return ATVS_ERR_NULL;
  if (count < 0 || count > (1L << 31)) return ATVS_ERR_SHAPE;
  *bytes = (long)align256((size_t)scan_tiles(count > 0 ? count : 1) * sizeof(unsigned));
  return ATVS_OK;
}

extern "C" int atvs_tsdf_scan(void* counters, long count, void* scratch, long scratch_bytes, long long* total, atvs_stream_t stream) {
  long need = 0;
  if (atvs_tsdf_scan_scratch_size(count, &need) != ATVS_OK) return ATVS_ERR_SHAPE;
  if (!total || (count > 0 && (!counters || !scratch))) return ATVS_ERR_NULL;
  if (scratch_bytes < need) return ATVS_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  if (count == 0) return hipMemsetAsync(total, 0, sizeof(long long), st) == hipSuccess ? ATVS_OK : ATVS_ERR_LAUNCH;
  unsigned* a = static_cast<unsigned*>(counters);
  hipLaunchKernelGGL(tsdf_total_kernel, dim3(1), dim3(64), 0, st, (const unsigned*)a, count, total, 0);
  ATVS_LAUNCH_CHECK();
  const int rc = exclusive_scan(a, count, static_cast<unsigned*>(scratch), st);
  if (rc != ATVS_OK) return rc;
  hipLaunchKernelGGL(tsdf_total_kernel, dim3(1), dim3(64), 0, st, (const unsigned*)a, count, total, 1);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

static int tsdf_mark_args(const float* depths, const double* cams, int n, int rows, int cols, double voxel, double trunc,
                          const double* origin, int bx, int by, int bz, double pixel_centre, TsdfBox* B) {
  if (check_maps(n, rows, cols) != ATVS_OK) return ATVS_ERR_SHAPE;
  if (!depths || !cams) return ATVS_ERR_NULL;
  const int rc = check_box(origin, voxel, bx, by, bz, B);
  if (rc != ATVS_OK) return rc;
  if (!(trunc > 0.0) || !finite_d(trunc) || !finite_d(pixel_centre)) return ATVS_ERR_ARG;
  return ATVS_OK;
}

extern "C" int atvs_tsdf_mark(const float* depths, const double* cams, int n, int rows, int cols, double voxel, double trunc,
                              const double* origin, int bx, int by, int bz, double pixel_centre, void* directory, int* err,
                              atvs_stream_t stream) {
  TsdfBox B;
  const int rc = tsdf_mark_args(depths, cams, n, rows, cols, voxel, trunc, origin, bx, by, bz, pixel_centre, &B);
  if (rc != ATVS_OK) return rc;
  if (!directory || !err) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  const size_t nbk = (size_t)bx * by * bz;
  if (hipMemsetAsync(directory, 0, nbk * sizeof(unsigned), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  const long pixels = (long)n * rows * cols;
  hipLaunchKernelGGL(tsdf_mark_kernel, dim3((unsigned)cdiv(pixels, kThreads)), dim3(kThreads), 0, st, depths, cams, n, rows, cols, B, trunc,
                     pixel_centre, static_cast<unsigned*>(directory), (unsigned long long*)nullptr, 0, err);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_tsdf_assign(const float* depths, const double* cams, int n, int rows, int cols, double voxel, double trunc,
                                const double* origin, int bx, int by, int bz, double pixel_centre, const void* slots, long count,
                                int* coords, void* masks, int* err, atvs_stream_t stream) {
  TsdfBox B;
  const int rc = tsdf_mark_args(depths, cams, n, rows, cols, voxel, trunc, origin, bx, by, bz, pixel_centre, &B);
  if (rc != ATVS_OK) return rc;
  const long nbk = (long)bx * by * bz;
  if (count < 0 || count > nbk) return ATVS_ERR_SHAPE;
  if (!slots || !err || (count > 0 && (!coords || !masks))) return ATVS_ERR_NULL;
  if (count == 0) return ATVS_OK;
  hipStream_t st = as_stream(stream);
  const int words = (n + 63) / 64;
  if (hipMemsetAsync(masks, 0, (size_t)count * words * sizeof(unsigned long long), st) != hipSuccess) return ATVS_ERR_LAUNCH;
  hipLaunchKernelGGL(tsdf_coords_kernel, dim3((unsigned)cdiv(nbk, kThreads)), dim3(kThreads), 0, st, static_cast<const unsigned*>(slots), nbk,
                     (unsigned)count, bx, by, coords);
  ATVS_LAUNCH_CHECK();
  const long pixels = (long)n * rows * cols;
  // the slots are only read here: the kernel's one pointer serves both passes
  hipLaunchKernelGGL(tsdf_mark_kernel, dim3((unsigned)cdiv(pixels, kThreads)), dim3(kThreads), 0, st, depths, cams, n, rows, cols, B, trunc,
                     pixel_centre, const_cast<unsigned*>(static_cast<const unsigned*>(slots)), static_cast<unsigned long long*>(masks), words,
                     err);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_tsdf_integrate(const float* depths, const float* images, int channels, const double* cams, int n, int rows, int cols,
                                   double voxel, double trunc, const double* origin, int bx, int by, int bz, double pixel_centre,
                                   const int* coords, const void* masks, long count, float* tsdf, float* weight, float* color, void* any,
                                   atvs_stream_t stream) {
  TsdfBox B;
  const int rc = tsdf_mark_args(depths, cams, n, rows, cols, voxel, trunc, origin, bx, by, bz, pixel_centre, &B);
  if (rc != ATVS_OK) return rc;
  if (count < 0 || count > (long)bx * by * bz) return ATVS_ERR_SHAPE;
  if (images != nullptr && channels < 3) return ATVS_ERR_SHAPE;
  if ((images == nullptr) != (color == nullptr)) return ATVS_ERR_NULL;
  if (count > 0 && (!coords || !masks || !tsdf || !weight || !any)) return ATVS_ERR_NULL;
  if (count == 0) return ATVS_OK;
  hipLaunchKernelGGL((tsdf_integrate_kernel<false, false>), dim3((unsigned)count), dim3(kVox), 0, as_stream(stream), depths, images, channels,
                     cams, rows, cols, B, trunc, pixel_centre, coords, static_cast<const unsigned long long*>(masks), (n + 63) / 64, tsdf,
                     weight, color, static_cast<unsigned*>(any), (const unsigned long long*)nullptr, 0.0, (float*)nullptr,
                     (const float*)nullptr);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_tsdf_free_views(const int* coords, long count, const double* cams, int n, int rows, int cols, double voxel,
                                    const double* origin, int bx, int by, int bz, double pixel_centre, void* masks,
                                    atvs_stream_t stream) {
  if (check_maps(n, rows, cols) != ATVS_OK) return ATVS_ERR_SHAPE;
  TsdfBox B;
  const int rc = check_box(origin, voxel, bx, by, bz, &B);
  if (rc != ATVS_OK) return rc;
  if (!finite_d(pixel_centre)) return ATVS_ERR_ARG;
  if (count < 0 || count > (long)bx * by * bz) return ATVS_ERR_SHAPE;
  if (!cams || (count > 0 && (!coords || !masks))) return ATVS_ERR_NULL;
  if (count == 0) return ATVS_OK;
  const int words = (n + 63) / 64;
  const long groups = (count * words + kFreeWaves - 1) / kFreeWaves;
  hipLaunchKernelGGL(tsdf_free_views_kernel, dim3((unsigned)(groups < kFreeMaxGroups ? groups : kFreeMaxGroups)), dim3(64 * kFreeWaves), 0,
                     as_stream(stream), coords, count, cams, n, rows, cols, B, pixel_centre, static_cast<unsigned long long*>(masks), words);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_tsdf_integrate_carve(const float* depths, const float* images, int channels, const double* cams, int n, int rows,
                                         int cols, double voxel, double trunc, const double* origin, int bx, int by, int bz,
                                         double pixel_centre, const int* coords, const void* masks, const void* free_masks,
                                         double carve_weight, long count, float* tsdf, float* weight, float* color, float* free_out,
                                         void* any, atvs_stream_t stream) {
  TsdfBox B;
  const int rc = tsdf_mark_args(depths, cams, n, rows, cols, voxel, trunc, origin, bx, by, bz, pixel_centre, &B);
  if (rc != ATVS_OK) return rc;
  if (!(carve_weight > 0.0) || !finite_d(carve_weight)) return ATVS_ERR_ARG;
  if (count < 0 || count > (long)bx * by * bz) return ATVS_ERR_SHAPE;
  if (images != nullptr && channels < 3) return ATVS_ERR_SHAPE;
  if ((images == nullptr) != (color == nullptr)) return ATVS_ERR_NULL;
  if (count > 0 && (!coords || !masks || !free_masks || !tsdf || !weight || !free_out || !any)) return ATVS_ERR_NULL;
  if (count == 0) return ATVS_OK;
  hipLaunchKernelGGL((tsdf_integrate_kernel<true, false>), dim3((unsigned)count), dim3(kVox), 0, as_stream(stream), depths, images, channels,
                     cams, rows, cols, B, trunc, pixel_centre, coords, static_cast<const unsigned long long*>(masks), (n + 63) / 64, tsdf,
                     weight, color, static_cast<unsigned*>(any), static_cast<const unsigned long long*>(free_masks), carve_weight, free_out,
                     (const float*)nullptr);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_tsdf_integrate_weighted(const float* depths, const float* weights, const float* images, int channels,
                                            const double* cams, int n, int rows, int cols, double voxel, double trunc,
                                            const double* origin, int bx, int by, int bz, double pixel_centre, const int* coords,
                                            const void* masks, const void* free_masks, double carve_weight, long count, float* tsdf,
                                            float* weight, float* color, float* free_out, void* any, atvs_stream_t stream) {
  TsdfBox B;
  const int rc = tsdf_mark_args(depths, cams, n, rows, cols, voxel, trunc, origin, bx, by, bz, pixel_centre, &B);
  if (rc != ATVS_OK) return rc;
  if (!weights) return ATVS_ERR_NULL;
  const bool carving = free_masks != nullptr || free_out != nullptr;      // both NULL: no carving, carve_weight is not read
  if (carving && (!(carve_weight > 0.0) || !finite_d(carve_weight))) return ATVS_ERR_ARG;
  if (count < 0 || count > (long)bx * by * bz) return ATVS_ERR_SHAPE;
  if (images != nullptr && channels < 3) return ATVS_ERR_SHAPE;
  if ((images == nullptr) != (color == nullptr)) return ATVS_ERR_NULL;
  if ((free_masks == nullptr) != (free_out == nullptr)) return ATVS_ERR_NULL;
  if (count > 0 && (!coords || !masks || !tsdf || !weight || !any)) return ATVS_ERR_NULL;
  if (count == 0) return ATVS_OK;
  hipLaunchKernelGGL((tsdf_integrate_kernel<true, true>), dim3((unsigned)count), dim3(kVox), 0, as_stream(stream), depths, images, channels,
                     cams, rows, cols, B, trunc, pixel_centre, coords, static_cast<const unsigned long long*>(masks), (n + 63) / 64, tsdf,
                     weight, color, static_cast<unsigned*>(any), static_cast<const unsigned long long*>(free_masks),
                     carving ? carve_weight : 0.0, free_out, weights);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_tsdf_gather(const int* coords, const float* tsdf, const float* weight, const float* color, const void* keep, long count,
                                long kept, int* coords_out, float* tsdf_out, float* weight_out, float* color_out, const float* free_in,
                                float* free_out, atvs_stream_t stream) {
  if (count < 0 || count > kMaxDirectory || kept < 0 || kept > count) return ATVS_ERR_SHAPE;
  if ((color == nullptr) != (color_out == nullptr) && kept > 0) return ATVS_ERR_NULL;
  if ((free_in == nullptr) != (free_out == nullptr) && kept > 0) return ATVS_ERR_NULL;
  if (kept > 0 && (!coords || !tsdf || !weight || !keep || !coords_out || !tsdf_out || !weight_out)) return ATVS_ERR_NULL;
  if (kept == 0) return ATVS_OK;
  hipLaunchKernelGGL(tsdf_gather_kernel, dim3((unsigned)count), dim3(kVox), 0, as_stream(stream), coords, tsdf, weight, color,
                     static_cast<const unsigned*>(keep), count, (unsigned)kept, coords_out, tsdf_out, weight_out, color_out, free_in,
                     free_out);
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_tsdf_mesh_count(const int* blocks, int nb, int bx, int by, int bz, const float* tsdf, const float* weight,
                                    float min_weight, void* cube_ok, void* emask, void* vcount, void* fcount, atvs_stream_t stream) {
  const int rc = check_blocks(nb, bx, by, bz);
  if (rc != ATVS_OK) return rc;
  if (min_weight != min_weight) return ATVS_ERR_ARG;
  if (nb > 0 && (!blocks || !tsdf || !weight || !cube_ok || !emask || !vcount || !fcount)) return ATVS_ERR_NULL;
  if (nb == 0) return ATVS_OK;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(tsdf_cubes_kernel, dim3((unsigned)nb), dim3(kVox), 0, st, blocks, nb, bx, by, bz, tsdf, weight, min_weight,
                     static_cast<unsigned char*>(cube_ok), static_cast<unsigned*>(fcount));
  ATVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsdf_edges_kernel, dim3((unsigned)nb), dim3(kVox), 0, st, blocks, nb, bx, by, bz, tsdf,
                     static_cast<const unsigned char*>(cube_ok), static_cast<unsigned char*>(emask), static_cast<unsigned*>(vcount));
  ATVS_LAUNCH_CHECK();
  return ATVS_OK;
}

extern "C" int atvs_tsdf_mesh_emit(const int* blocks, int nb, int bx, int by, int bz, double voxel, const double* origin, const float* tsdf,
                                   const float* color, const void* emask, const void* vstart, const void* fstart, long n_vertices,
                                   long n_faces, float* vertices, void* colors, int* faces, atvs_stream_t stream) {
  int rc = check_blocks(nb, bx, by, bz);
  if (rc != ATVS_OK) return rc;
  TsdfBox B;
  rc = check_box(origin, voxel, bx, by, bz, &B);
  if (rc != ATVS_OK) return rc;
  if (n_vertices < 0 || n_faces < 0 || n_vertices > 7L * kVox * nb || n_faces > 12L * kVox * nb) return ATVS_ERR_SHAPE;
  if ((color == nullptr) != (colors == nullptr) && n_vertices > 0) return ATVS_ERR_NULL;
  if (nb > 0 && (!blocks || !tsdf || !emask || !vstart || !fstart)) return ATVS_ERR_NULL;
  if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) return ATVS_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (n_vertices > 0) {
    hipLaunchKernelGGL(tsdf_vertices_kernel, dim3((unsigned)nb), dim3(kVox), 0, st, blocks, nb, bx, by, bz, B, tsdf, color,
                       static_cast<const unsigned char*>(emask), static_cast<const unsigned*>(vstart), vertices,
                       static_cast<unsigned char*>(colors));
    ATVS_LAUNCH_CHECK();
  }
  if (n_faces > 0) {
    hipLaunchKernelGGL(tsdf_faces_kernel, dim3((unsigned)nb), dim3(kVox), 0, st, blocks, nb, bx, by, bz, tsdf,
                       static_cast<const unsigned char*>(emask), static_cast<const unsigned*>(vstart), static_cast<const unsigned*>(fstart),
                       (long)nb * kVox, (unsigned)n_faces, faces);
    ATVS_LAUNCH_CHECK();
  }
  return ATVS_OK;
}
