// The cells of the sparse voxel table, ONE definition for cloud_register.hip (atvs_cloud_voxel_downsample, atvs_cloud_voxel_shares)
// and mesh_simplify.hip (the clusters of atvs_mesh_cluster): the cell and the 32-bit fraction of a coordinate, the packed key, the
// open-addressing slot of a cell.  include/atvsnet_hip.h states the rule; nothing here allocates or launches.
#pragma once
#include <math.h>

#include "common.h"
#include "cloud_common.h"

namespace {

constexpr unsigned long long kEmpty = ~0ull;
constexpr double kCellLimit = 2097152.0;               // 2^21 cells per axis

struct VoxelArgs {
  double origin[3];
  double voxel;
};

// cell c and fraction u of one coordinate; false when the cell leaves [0, 2^21)
__device__ __forceinline__ bool voxel_coord(float x, double origin, double voxel, unsigned long long* c, unsigned long long* u) {
  const double g = ((double)x - origin) / voxel;
  const double cf = floor(g);
  if (!(cf >= 0.0 && cf < kCellLimit)) return false;
  const double f = floor((g - cf) * 4294967296.0);
  *c = (unsigned long long)cf;
  *u = f >= 4294967295.0 ? 4294967295ull : (unsigned long long)f;
  return true;
}

// The slot of the voxel with cells c[] in the open-addressing table (ONE definition for the down-sampler, the shares and the mesh
// clusters): the key packs the cells 3 x 21 bits, probing is linear from a multiplicative hash, one 64-bit compare-and-swap per
// probe.  The table is at most half full, so the loop ends long before `slots`; -1 is never returned in practice.
__device__ __forceinline__ int voxel_find_slot(const unsigned long long* c, unsigned long long* __restrict__ keys, long slots, int shift) {
  const unsigned long long key = c[0] | (c[1] << 21) | (c[2] << 42);
  unsigned long long h = (key * 0x9E3779B97F4A7C15ull) >> shift;
  for (long probe = 0; probe < slots; ++probe) {
    const unsigned long long seen = atomicCAS(keys + h, kEmpty, key);
    if (seen == kEmpty || seen == key) return (int)h;
    h = (h + 1) & (unsigned long long)(slots - 1);
  }
  return -1;
}

// The table's front end for point i: the slot of its voxel and its fractions u[] inside it; -1 for a non-finite point, and for one
// whose cell leaves [0, 2^21), which raises *err.
__device__ __forceinline__ int voxel_slot_of(const float* __restrict__ pts, long i, const VoxelArgs& A, long slots, int shift,
                                             unsigned long long* __restrict__ keys, int* __restrict__ err, unsigned long long* u) {
  const float x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
  if (!finite3(x, y, z)) return -1;
  unsigned long long c[3];
  const bool ok = voxel_coord(x, A.origin[0], A.voxel, &c[0], &u[0]) & voxel_coord(y, A.origin[1], A.voxel, &c[1], &u[1]) &
                  voxel_coord(z, A.origin[2], A.voxel, &c[2], &u[2]);
  if (!ok) {
    atomicOr(err, 1);
    return -1;
  }
  return voxel_find_slot(c, keys, slots, shift);
}

// voxel and origin as the caller gave them -> A; false (voxel <= 0, or either not finite): ATVS_ERR_ARG
inline bool voxel_args(double voxel, const double* origin, VoxelArgs* A) {
  const double big = 1.7976931348623157e308;
  *A = VoxelArgs{{origin[0], origin[1], origin[2]}, voxel};
  return voxel > 0.0 && voxel <= big && fabs(origin[0]) <= big && fabs(origin[1]) <= big && fabs(origin[2]) <= big;
}

}  // namespace
