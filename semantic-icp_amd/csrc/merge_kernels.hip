// merge_kernels.hip -- sicp_merge_clouds: several posed clouds into one voxel-grid cloud (driver: merge.cpp; the rules and
// their precisions: INTEGRATION.md, "Merging registered scans").  Transform, crop and voxel key per point in one launch over
// all parts; a stable radix sort by key; per voxel the f64 sum of its points in ascending global index and the most frequent
// label.  No floating-point atomics: every sum runs in a fixed order, so every output is run-to-run bit-reproducible.
#include <hip/hip_runtime.h>

#define SICP_HD __host__ __device__
#include "job_table.hpp"
#include "kernels.h"
#include "voxel_key.hpp"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;
constexpr u64 kDropped = kVoxelDropped;

// per point: transform, crop (exec/filter_range.h in f32 about a centre), voxel key -- the arithmetic of voxel_key.hpp, which the
// voxel map shares.  key = three biased 21-bit voxel coordinates, z highest, so ascending keys are ascending (vz, vy, vx); 0
// without a grid; ~0 for a cropped point.  A coordinate beyond the fields raises res[kMergeRange] (a plain store: every writer
// stores the same 1).
__global__ __launch_bounds__(256) void merge_key_kernel(MergeKeyArgs a) {
  int lb;
  const MergePart& P = a.parts[job_of(a.blk_end, a.n_parts, blockIdx.x, &lb)];
  const int i = lb * 256 + threadIdx.x;
  if (i >= P.n) return;
  const int g = P.off + i;
  const double x = P.x[i], y = P.y[i], z = P.z[i];
  const float px = voxel_xform_row(P.M + 0, x, y, z);
  const float py = voxel_xform_row(P.M + 4, x, y, z);
  const float pz = voxel_xform_row(P.M + 8, x, y, z);
  a.tx[g] = px; a.ty[g] = py; a.tz[g] = pz;
  if (a.tlabel) a.tlabel[g] = P.label[i];
  const bool keep = !a.crop || voxel_crop_keeps(px, py, pz, a.cx, a.cy, a.cz, a.range_sq);
  u64 k = kDropped;
  if (keep) {
    k = 0;
    if (a.voxel && !voxel_key(px, py, pz, a.inv_leaf, &k)) {
      k = kDropped;
      a.res[kMergeRange] = 1;
    }
  }
  a.key[g] = k;
  a.val[g] = g;
}

// sorted position j opens a voxel (without a grid every kept point is one)
__global__ __launch_bounds__(256) void merge_heads_kernel(MergeReduceArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const u64 k = a.skey[j];
  a.flag[j] = (k != kDropped && (j == 0 || !a.voxel || k != a.skey[j - 1])) ? 1 : 0;
}

// the transformed points (and rank << 32 | label) once into sorted order, so that the reductions read contiguous runs; the
// first position of every voxel; the counts of kept points and voxels
__global__ __launch_bounds__(256) void merge_gather_kernel(MergeReduceArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const u64 k = a.skey[j];
  const int f = a.flag[j], p = a.pos[j];
  if (k != kDropped) {
    const int g = a.sval[j];
    a.gx[j] = a.tx[g]; a.gy[j] = a.ty[g]; a.gz[j] = a.tz[g];
    if (a.labels) a.lkey[j] = ((u64)(unsigned)(p + f - 1) << 32) | (u64)a.tlabel[g];
    if (f) a.heads[p] = j;
    if (j == a.n - 1 || a.skey[j + 1] == kDropped) a.res[kMergeKept] = j + 1;
  } else if (a.labels) {
    a.lkey[j] = kDropped;
  }
  if (j == a.n - 1) a.res[kMergeOut] = p + f;
}

// one lane per voxel: the f64 sum of its points in ascending global index / count, rounded once to f32 (the rule of
// boot_centroid_kernel; the order is the specification, so a long voxel is not split across lanes)
__global__ __launch_bounds__(256) void merge_centroid_kernel(MergeReduceArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n_out = a.res[kMergeOut], n_kept = a.res[kMergeKept];
  int cnt = 0;
  if (k < a.n && k < n_out) {
    const int b = a.heads[k], e = k + 1 < n_out ? a.heads[k + 1] : n_kept;
    double sx = 0, sy = 0, sz = 0;
    for (int j = b; j < e; ++j) { sx += (double)a.gx[j]; sy += (double)a.gy[j]; sz += (double)a.gz[j]; }
    cnt = e - b;
    const double c = (double)cnt;
    a.ox[k] = (float)(sx / c); a.oy[k] = (float)(sy / c); a.oz[k] = (float)(sz / c);
    a.ocount[k] = (uint32_t)cnt;
  }
  int m = cnt;
  for (int w = 32; w > 0; w >>= 1) m = max(m, __shfl_xor(m, w, 64));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&a.res[kMergeMaxCount], m);
}

// one lane per voxel: the longest run of equal labels in the voxel's range of the (rank, label) sort; ascending labels, so
// the first of equal runs is the smallest label
__global__ __launch_bounds__(256) void merge_label_kernel(MergeReduceArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n_out = a.res[kMergeOut], n_kept = a.res[kMergeKept];
  if (k >= a.n || k >= n_out) return;
  const int b = a.heads[k], e = k + 1 < n_out ? a.heads[k + 1] : n_kept;
  uint32_t best = 0, cur = 0;
  int best_len = 0, len = 0;
  for (int j = b; j < e; ++j) {
    const uint32_t l = (uint32_t)(a.lsorted[j] & 0xffffffffull);
    if (len > 0 && l == cur) ++len; else { cur = l; len = 1; }
    if (len > best_len) { best_len = len; best = cur; }
  }
  a.olabel[k] = best;
}

inline dim3 merge_grid(int n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_merge_keys(const MergeKeyArgs& a, int blocks, hipStream_t st) {
  if (a.n_parts <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(merge_key_kernel, dim3(blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_merge_heads(const MergeReduceArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(merge_heads_kernel, merge_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_merge_gather(const MergeReduceArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(merge_gather_kernel, merge_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_merge_centroids(const MergeReduceArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(merge_centroid_kernel, merge_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_merge_labels(const MergeReduceArgs& a, hipStream_t st) {
  if (a.n <= 0 || !a.labels) return hipSuccess;
  hipLaunchKernelGGL(merge_label_kernel, merge_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sicp
