// voxel_key.hpp -- the per-point arithmetic that sicp_merge_clouds (merge_kernels.hip) and the voxel map (map_kernels.hip)
// share, so that the two cannot drift: the pose transform, the crop test and the voxel key of include/sicp.h, "registered
// scans into one cloud", steps 2 - 4.  Device code only; every operation is rounded on its own (no contraction).
#ifndef SICP_VOXEL_KEY_HPP_
#define SICP_VOXEL_KEY_HPP_

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace sicp {

constexpr unsigned long long kVoxelDropped = ~0ull;  // the key of a point that the crop (or the grid's range) drops

// pcl::transformPointCloud<PointT,double> as the search transforms its queries (knn_kernels.hip: xform_row):
// (((m0*x + m1*y) + m2*z) + m3) in double, no contraction, then one rounding to float
__device__ __forceinline__ float voxel_xform_row(const double* m, double x, double y, double z) {
#pragma clang fp contract(off)
  double a = __dmul_rn(m[0], x);
  a = __dadd_rn(a, __dmul_rn(m[1], y));
  a = __dadd_rn(a, __dmul_rn(m[2], z));
  a = __dadd_rn(a, m[3]);
  return __double2float_rn(a);
}

// exec/filter_range.h in f32 about a centre: d = p - c, d2 = (dx dx + dy dy) + dz dz, kept when (double)d2 <= range^2
__device__ __forceinline__ bool voxel_crop_keeps(float px, float py, float pz, float cx, float cy, float cz, double range_sq) {
#pragma clang fp contract(off)
  const float dx = __fsub_rn(px, cx), dy = __fsub_rn(py, cy), dz = __fsub_rn(pz, cz);
  float d2 = __fmul_rn(dx, dx);
  d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
  d2 = __fadd_rn(d2, __fmul_rn(dz, dz));
  return (double)d2 <= range_sq;
}

// v = floor(p * inv_leaf) per axis in float; three biased 21-bit voxel coordinates, z highest, so ascending keys are ascending
// (vz, vy, vx).  false (and nothing written) when a coordinate lies beyond the fields (a NaN fails too).
__device__ __forceinline__ bool voxel_key(float px, float py, float pz, float inv_leaf, unsigned long long* key) {
#pragma clang fp contract(off)
  typedef unsigned long long u64;
  const float v0 = floorf(__fmul_rn(px, inv_leaf)), v1 = floorf(__fmul_rn(py, inv_leaf)), v2 = floorf(__fmul_rn(pz, inv_leaf));
  const float lim = (float)kMergeBias;
  if (!(fabsf(v0) < lim && fabsf(v1) < lim && fabsf(v2) < lim)) return false;
  *key = ((u64)(unsigned)((int)v2 + kMergeBias) << 42) | ((u64)(unsigned)((int)v1 + kMergeBias) << 21) |
         (u64)(unsigned)((int)v0 + kMergeBias);
  return true;
}

}  // namespace sicp
#endif
