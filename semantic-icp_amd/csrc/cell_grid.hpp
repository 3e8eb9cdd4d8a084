// cell_grid.hpp -- the sorted cell grid of sicp_cluster and sicp_filter (device code: included by cluster_kernels.hip and
// filter_kernels.hip only).  A point's cell is three integers; its key packs them, biased, into 21-bit fields with z highest,
// so that sorted keys list the cells row by row and every row of neighbouring cells is one run of consecutive positions.
#ifndef SICP_CELL_GRID_HPP_
#define SICP_CELL_GRID_HPP_

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace sicp {

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;
constexpr int kCellBias = 1 << 20;
constexpr u64 kCellRow = 1ull << 21, kCellPlane = 1ull << 42;  // the key of the next cell in y / in z

// The grid is an accelerator, not the definition: it must put every joined pair into cells that differ by at most one per axis.
//  (1) Rounding is monotone, so fl(dx dx) <= d2 (the two adds of non-negative terms never round below their first operand) and
//      d2 < t2 = fl(t t) gives dx dx < t t, |dx| < t with dx = fl(px - qx); t is a float, so |px - qx| >= t would give
//      |fl(px - qx)| >= t: hence |px - qx| < t in real numbers, with no rounding allowance left to make.
//  (2) The host picks the largest float inv with inv t <= 1, tested on the exact product (double)inv (double)t.  u = (double)p
//      (double)inv is exact too (24 x 24 bits), so |u_p - u_q| = inv |px - qx| < 1 holds in real numbers.
//  (3) |u_p - u_q| < 1 gives |floor(u_p) - floor(u_q)| <= 1.  The same on y and z.
// (floor(p * inv) in float, as voxel_key forms it, is off by up to |u| 2^-24 cells and would break (3) at large coordinates.)
__device__ __forceinline__ bool cluster_cell(float p, float inv, int* c) {
  const double v = floor(__dmul_rn((double)p, (double)inv));
  if (!(fabs(v) < (double)kClusterCellLimit)) return false;
  *c = (int)v;
  return true;
}

__device__ __forceinline__ u64 cell_key(int cx, int cy, int cz) {
  return ((u64)(unsigned)(cz + kCellBias) << 42) | ((u64)(unsigned)(cy + kCellBias) << 21) | (u64)(unsigned)(cx + kCellBias);
}

__device__ __forceinline__ int lower_bound_key(const u64* k, int lo, int hi, u64 v) {  // first position in [lo, hi) with k >= v
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (k[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace sicp

#endif
