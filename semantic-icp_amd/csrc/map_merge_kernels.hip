// map_merge_kernels.hip -- sicp_map_merge: one voxel map added into another at a pose with its evidence intact (driver:
// map.cpp; the rules: include/sicp.h, "fusing maps").  The items are SRC's rows.  A lane moves its row's f64 sums by the pose,
// keys the float centroid of the MOVED sums on dst's grid (voxel_key.hpp), and the (key, row) pairs go through the stable radix
// sort, so rows ascend inside a run of equal keys.  The runs' heads are a sorted list of distinct keys: integrate's rank merge
// (map_kernels.hip: lookup, misses, scatter, move_hist) opens and moves dst's rows for them.  One lane per touched row then
// continues the row's sums with its run in ascending src row -- a lane owns its row: plain stores, no float atomics -- and a
// second launch, parallel over (touched row, bin), adds the run's histogram rows with integer adds.
#include <hip/hip_runtime.h>

#include <algorithm>

#define SICP_HD __host__ __device__
#include "kernels.h"
#include "voxel_key.hpp"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

// voxel_xform_row's order on a row's sums, the translation scaled by the count, no rounding to float:
// ((m0 sx + m1 sy) + m2 sz) + m3 c
__device__ __forceinline__ double merge_move_row(const double* m, double sx, double sy, double sz, double c) {
  double a = __dmul_rn(m[0], sx);
  a = __dadd_rn(a, __dmul_rn(m[1], sy));
  a = __dadd_rn(a, __dmul_rn(m[2], sz));
  return __dadd_rn(a, __dmul_rn(m[3], c));
}

constexpr int kMergeMaxBlocks = 1024;  // a workgroup loops over its rows and ends in ONE atomic: a thousand on one address, not one a wave

// per src row: the min_count test, the moved sums, the float centroid of them, the crop, dst's key (~0 for a row that takes
// no part); a coordinate beyond the key's fields raises its flag (a plain store: every writer stores the same 1).  The kept
// rows' counts: summed per lane over the workgroup's turns, per wave by shuffles, per workgroup through LDS, one integer atomic.
__global__ __launch_bounds__(256) void map_merge_key_kernel(MapMergeArgs a) {
  __shared__ u64 part[4];
  u64 kept = 0;
  const long long step = (long long)gridDim.x * 256;
  for (long long r0 = (long long)blockIdx.x * 256; r0 < a.n; r0 += step) {  // (the same trip count in every lane)
    const long long r = r0 + threadIdx.x;
    if (r >= a.n) continue;
    const uint32_t cnt = a.src.cnt[r];
    u64 k = kVoxelDropped;
    if ((long long)cnt >= a.min_count) {
      const double sx = a.src.sx[r], sy = a.src.sy[r], sz = a.src.sz[r], c = (double)cnt;
      const double tx = merge_move_row(a.M + 0, sx, sy, sz, c);
      const double ty = merge_move_row(a.M + 4, sx, sy, sz, c);
      const double tz = merge_move_row(a.M + 8, sx, sy, sz, c);
      a.mx[r] = tx; a.my[r] = ty; a.mz[r] = tz;
      const float px = __double2float_rn(__ddiv_rn(tx, c));
      const float py = __double2float_rn(__ddiv_rn(ty, c));
      const float pz = __double2float_rn(__ddiv_rn(tz, c));
      if (!a.crop || voxel_crop_keeps(px, py, pz, a.cx, a.cy, a.cz, a.range_sq)) {
        if (voxel_key(px, py, pz, a.inv_leaf, &k)) {
          kept += cnt;  // (at most 2^31 rows of counts below 2^32: no overflow)
        } else {
          k = kVoxelDropped;
          a.res[kMapRange] = 1;
        }
      }
    }
    a.key[r] = k;
    a.val[r] = (int)r;
  }
  for (int w = 32; w > 0; w >>= 1) kept += (u64)__shfl_xor((long long)kept, w, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 sum = part[0] + part[1] + part[2] + part[3];
    if (sum) atomicAdd(a.kept_points, sum);
  }
}

// the first sorted position of every run of equal keys; the numbers of kept rows and of runs
__global__ __launch_bounds__(256) void map_merge_runs_kernel(MapMergeArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const int f = a.flag[j], p = a.pos[j];
  if (a.skey[j] != kVoxelDropped) {
    if (f) a.heads[p] = j;
    if (j == a.n - 1 || a.skey[j + 1] == kVoxelDropped) a.res[kMapKept] = j + 1;
  }
  if (j == a.n - 1) a.res[kMapScanVoxels] = p + f;
}

// one lane per touched dst row: its sums continued from the stored value (0.0 for an opened row) with the run's moved sums in
// ascending src row, one add per axis and row -- the order is the specification, so a run is not split across lanes -- and its
// count.  The longest run: one integer atomic a workgroup, as the key kernel's sum.
__global__ __launch_bounds__(256) void map_merge_fold_sums_kernel(MapMergeArgs a) {
  __shared__ int part[4];
  int run = 0;
  const long long step = (long long)gridDim.x * 256;
  for (long long k0 = (long long)blockIdx.x * 256; k0 < a.n_runs; k0 += step) {
    const long long k = k0 + threadIdx.x;
    if (k >= a.n_runs) continue;
    const long long r = (long long)a.rank[k] + a.mpos[k];
    if (r >= (long long)a.n_map + a.n_new) continue;  // (never; a row beyond the buffers is not written)
    const int b = a.heads[k], e = k + 1 < a.n_runs ? a.heads[k + 1] : a.n_kept;
    double sx = a.to.sx[r], sy = a.to.sy[r], sz = a.to.sz[r];
    uint32_t c = a.to.cnt[r];
    for (int j = b; j < e; ++j) {
      const int s = a.sval[j];
      sx = __dadd_rn(sx, a.mx[s]); sy = __dadd_rn(sy, a.my[s]); sz = __dadd_rn(sz, a.mz[s]);
      c += a.src.cnt[s];  // (the host has checked the map's total: no count passes 2^32 - 1)
    }
    a.to.sx[r] = sx; a.to.sy[r] = sy; a.to.sz[r] = sz;
    a.to.cnt[r] = c;
    run = max(run, e - b);
  }
  for (int w = 32; w > 0; w >>= 1) run = max(run, __shfl_xor(run, w, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int m = max(max(part[0], part[1]), max(part[2], part[3]));
    if (m > 0) atomicMax(&a.res[kMapMaxCount], m);
  }
}

// one lane per (touched dst row, bin): consecutive lanes own consecutive bins, so every step of the run reads consecutive
// words of one src histogram row, whatever the stride.  Integer adds: their order is free.
__global__ __launch_bounds__(256) void map_merge_fold_hist_kernel(MapMergeArgs a) {
  const long long total = (long long)a.n_runs * a.stride;
  const long long step = (long long)gridDim.x * 256;
  const long long rows = (long long)a.n_map + a.n_new;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
    const int k = (int)(e / a.stride);
    const int bin = (int)(e - (long long)k * a.stride);
    const long long r = (long long)a.rank[k] + a.mpos[k];
    if (r >= rows) continue;
    const int b = a.heads[k], end = k + 1 < a.n_runs ? a.heads[k + 1] : a.n_kept;
    uint32_t acc = 0u;
    for (int j = b; j < end; ++j) acc += a.src.hist[(long long)a.sval[j] * a.stride + bin];
    a.to.hist[r * a.stride + bin] += acc;
  }
}

inline dim3 merge_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }
inline dim3 merge_looped_grid(long long n) { return dim3((unsigned)std::min<long long>((n + 255) / 256, kMergeMaxBlocks)); }

}  // namespace

hipError_t launch_map_merge_keys(const MapMergeArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_merge_key_kernel, merge_looped_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_merge_runs(const MapMergeArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_merge_runs_kernel, merge_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_merge_fold_sums(const MapMergeArgs& a, hipStream_t st) {
  if (a.n_runs <= 0) return hipSuccess;
  if (a.n_runs > a.n || a.n_kept < a.n_runs || a.n_kept > a.n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(map_merge_fold_sums_kernel, merge_looped_grid(a.n_runs), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_merge_fold_hist(const MapMergeArgs& a, hipStream_t st) {
  const long long total = (long long)a.n_runs * a.stride;
  if (total <= 0) return hipSuccess;
  if (a.n_runs > a.n || a.n_kept < a.n_runs || a.n_kept > a.n || !a.src.hist || !a.to.hist) return hipErrorInvalidValue;
  const long long blocks = std::min<long long>((total + 255) / 256, 1 << 16);  // (the rest by the kernel's stride loop)
  hipLaunchKernelGGL(map_merge_fold_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sicp
