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

// the voxel coordinates a key holds
__device__ __forceinline__ void voxel_key_coords(unsigned long long key, int* vx, int* vy, int* vz) {
  *vx = (int)(key & 0x1fffffull) - kMergeBias;
  *vy = (int)((key >> 21) & 0x1fffffull) - kMergeBias;
  *vz = (int)((key >> 42) & 0x1fffffull) - kMergeBias;
}

// a histogram row's fullest bin, the label of a map row wherever one is asked for (extract, carve, raycast, elevation): ties to
// the smallest label, bin 0 can win
__device__ __forceinline__ uint32_t map_fullest_bin(const uint32_t* h, int stride) {
  uint32_t best = 0, best_n = h[0];
  for (int l = 1; l < stride; ++l) {
    const uint32_t m = h[l];
    if (m > best_n) { best_n = m; best = (uint32_t)l; }
  }
  return best;
}

// The voxel walk of sicp_map_carve (include/sicp.h, "free-space carving", rule 4): from the voxel of the origin o to the voxel
// of the return p in exactly n = |dvx| + |dvy| + |dvz| steps of one voxel along one axis.  Per axis u = (double)o * (double)
// inv_leaf and w = (double)p * (double)inv_leaf (exact products), du = w - u, and for an axis that has steps to take
// tmax = ((double)(vo + (step > 0)) - u) / du, tdelta = (double)step / du; a step goes along the axis with steps left whose tmax
// is the smallest (x before y before z among equals) and adds tdelta to it.  All in double, every operation rounded on its own;
// the trip count is an integer, so the walk ends in the return's voxel whatever the rounding.
struct VoxelRay {
  unsigned long long key;  // the voxel the walk stands in
  int n;                   // steps from the origin's voxel to the return's
  int rx, ry, rz;          // steps left per axis
  int sx, sy, sz;          // +1 / -1 (0: none to take)
  double mx, my, mz;       // tmax
  double dx, dy, dz;       // tdelta
};

__device__ __forceinline__ void voxel_ray_axis(float o, float p, float inv_leaf, int vo, int vp, int* rem, int* step, double* tmax,
                                               double* tdelta) {
#pragma clang fp contract(off)
  const int d = vp - vo;
  *rem = d < 0 ? -d : d;
  *step = d > 0 ? 1 : (d < 0 ? -1 : 0);
  *tmax = 0.0;
  *tdelta = 0.0;
  if (d == 0) return;
  const double u = __dmul_rn((double)o, (double)inv_leaf), w = __dmul_rn((double)p, (double)inv_leaf);
  const double du = __dsub_rn(w, u);  // (not 0: the two floors differ, so the products do)
  *tmax = __ddiv_rn(__dsub_rn((double)(vo + (d > 0 ? 1 : 0)), u), du);
  *tdelta = __ddiv_rn((double)*step, du);
}

// ko, kp: the keys of o and p (voxel_key)
__device__ __forceinline__ void voxel_ray_begin(float ox, float oy, float oz, unsigned long long ko, float px, float py, float pz,
                                                unsigned long long kp, float inv_leaf, VoxelRay* r) {
  int ax, ay, az, bx, by, bz;
  voxel_key_coords(ko, &ax, &ay, &az);
  voxel_key_coords(kp, &bx, &by, &bz);
  voxel_ray_axis(ox, px, inv_leaf, ax, bx, &r->rx, &r->sx, &r->mx, &r->dx);
  voxel_ray_axis(oy, py, inv_leaf, ay, by, &r->ry, &r->sy, &r->my, &r->dy);
  voxel_ray_axis(oz, pz, inv_leaf, az, bz, &r->rz, &r->sz, &r->mz, &r->dz);
  r->key = ko;
  r->n = r->rx + r->ry + r->rz;
}

// one step (the caller counts them: at most n); returns the axis taken, 0 / 1 / 2
__device__ __forceinline__ int voxel_ray_step(VoxelRay* r) {
#pragma clang fp contract(off)
  int axis = -1;
  double best = 0.0;
  if (r->rx > 0) { axis = 0; best = r->mx; }
  if (r->ry > 0 && (axis < 0 || r->my < best)) { axis = 1; best = r->my; }
  if (r->rz > 0 && (axis < 0 || r->mz < best)) axis = 2;
  // (selects, not branches: the three axes stay in registers)
  const bool tx = axis == 0, ty = axis == 1, tz = axis == 2;
  const long long dk = tx ? (long long)r->sx : (ty ? (long long)r->sy * (1ll << 21) : (tz ? (long long)r->sz * (1ll << 42) : 0ll));
  r->key += (unsigned long long)dk;
  r->rx -= tx ? 1 : 0;
  r->ry -= ty ? 1 : 0;
  r->rz -= tz ? 1 : 0;
  const double nx = __dadd_rn(r->mx, r->dx), ny = __dadd_rn(r->my, r->dy), nz = __dadd_rn(r->mz, r->dz);
  r->mx = tx ? nx : r->mx;
  r->my = ty ? ny : r->my;
  r->mz = tz ? nz : r->mz;
  return axis;
}

}  // namespace sicp
#endif
