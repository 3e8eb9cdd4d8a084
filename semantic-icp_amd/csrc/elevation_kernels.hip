// elevation_kernels.hip -- sicp_map_elevation (include/sicp.h, "elevation"; driver: elevation.cpp; the launches' order:
// kernels.h, MapElevationArgs).  The map's rows are keyed by (cell of the window, level), sorted once -- a stable radix sort, so
// the rows of one cell and level stay in ascending map row, the order in which rule 5 adds a level's sums -- and every occupied
// cell is then walked by the one lane that owns it: plain stores, no float atomics, every byte run-to-run reproducible and
// independent of the launch shape.  The map is only read.
#include <hip/hip_runtime.h>

#include <algorithm>

#define SICP_HD __host__ __device__
#include "kernels.h"
#include "voxel_key.hpp"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

constexpr unsigned kElevNaN = 0x7fc00000u;  // the quiet NaN of an EMPTY cell
constexpr u64 kElevLevelMask = (1ull << kElevLevelBits) - 1;

// the mathematical floor of a / b (b > 0)
__device__ __forceinline__ int elev_fdiv(int a, int b) {
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

__device__ __forceinline__ bool elev_listed(const uint32_t* list, int n, uint32_t l) {
  bool in = false;
  for (int j = 0; j < n; ++j) in = in || list[j] == l;
  return in;
}

// the window's cell of the voxel column (vx, vy), -1 outside
__device__ __forceinline__ int elev_cell_of(const MapElevationArgs& a, int vx, int vy) {
  const int i = elev_fdiv(vx, a.B) - a.x0, j = elev_fdiv(vy, a.B) - a.y0;
  if (i < 0 || i >= a.W || j < 0 || j >= a.H) return -1;
  return j * a.W + i;
}

// every cell EMPTY (rule 5), its neighbourhood outputs included (rule 6); every point "no cell" (rule 8)
__global__ __launch_bounds__(256) void elevation_init_kernel(MapElevationArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long cells = (long long)a.W * a.H;
  const float nan = __uint_as_float(kElevNaN);
  if (t < cells) {
    a.state[t] = 0;
    a.elevation[t] = nan; a.bottom[t] = nan; a.ceiling[t] = nan;
    a.label[t] = 0u; a.count[t] = 0u;
    a.level_top[t] = 0; a.level_bottom[t] = 0; a.n_levels[t] = 0;
  }
  if (t < a.n_caller) {
    a.point_cell[t] = -1;
    a.point_height[t] = nan;
  }
}

// rule 2, one lane per map row: (cell << 21) | (vz + bias) for a row that counts, all ones otherwise; the histogram is read only
// when labels are ignored
__global__ __launch_bounds__(256) void elevation_key_kernel(MapElevationArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n_map) return;
  u64 k = ~0ull;
  int vx, vy, vz;
  voxel_key_coords(a.rows.key[r], &vx, &vy, &vz);
  if ((long long)a.rows.cnt[r] >= a.min_count && vz >= a.lo && vz <= a.hi) {
    const int c = elev_cell_of(a, vx, vy);
    bool counts = c >= 0;
    if (counts && a.n_ignore > 0) {
      const uint32_t l = map_fullest_bin(a.rows.hist + (size_t)r * (size_t)a.stride, a.stride);
      counts = !elev_listed(a.ignore, a.n_ignore, l);
    }
    if (counts) k = ((u64)(unsigned)c << kElevLevelBits) | (u64)(unsigned)(vz + kMergeBias);
  }
  a.key[r] = k;
  a.val[r] = r;
}

// flag[i]: sorted row i counts and is the first of its cell; the rows that count are the first ctl[kElevValid] sorted rows (one
// lane stands on their end)
__global__ __launch_bounds__(256) void elevation_heads_kernel(MapElevationArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_map) return;
  const u64 k = a.skey[i];
  const bool valid = k != ~0ull;
  a.flag[i] = (valid && (i == 0 || (a.skey[i - 1] >> kElevLevelBits) != (k >> kElevLevelBits))) ? 1 : 0;
  if (valid && (i == a.n_map - 1 || a.skey[i + 1] == ~0ull)) a.ctl[kElevValid] = i + 1;
}

// the occupied cells, ascending, with their first sorted row; their number
__global__ __launch_bounds__(256) void elevation_segment_kernel(MapElevationArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_map) return;
  const int f = a.flag[i], p = a.pos[i];
  if (f) {
    a.occ_cell[p] = (int)(a.skey[i] >> kElevLevelBits);
    a.occ_begin[p] = i;
  }
  if (i == a.n_map - 1) a.ctl[kElevOccupied] = p + f;
}

__device__ __forceinline__ int elev_level(const MapElevationArgs& a, int j) { return (int)(a.skey[j] & kElevLevelMask) - kMergeBias; }

// rule 5's mean of the sorted rows from j on that share j's level (they end before `end`): S = S + sz[row] in ascending map row
__device__ __forceinline__ float elev_level_mean(const MapElevationArgs& a, int j, int end, uint32_t* n_out) {
  const u64 k = a.skey[j];
  double S = 0.0;
  uint32_t N = 0u;
  for (; j < end && a.skey[j] == k; ++j) {
    const int row = a.sval[j];
    S = S + a.rows.sz[row];
    N += a.rows.cnt[row];
  }
  *n_out = N;
  return (float)(S / (double)N);
}

// rules 3 - 5, one lane per occupied cell.  The first walk reads keys only and finds the chosen run -- where its bottom and its
// top level begin among the sorted rows -- and where the run after it begins; the means and the label are then formed from
// those three stretches.
__global__ __launch_bounds__(256) void elevation_cell_kernel(MapElevationArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n_occ = a.ctl[kElevOccupied], n_valid = a.ctl[kElevValid];
  if (k >= n_occ) return;
  const int c = a.occ_cell[k];
  const int begin = a.occ_begin[k], end = k + 1 < n_occ ? a.occ_begin[k + 1] : n_valid;
  if (c < 0 || c >= a.W * a.H || begin < 0 || end > a.n_map || begin >= end) return;  // (cannot happen; nothing beyond the buffers)
  int run_at = begin, top_at = begin, next_at = end;   // the chosen run's bottom and top levels, the following run
  int bottom = elev_level(a, begin), top = bottom, levels = 1, prev = bottom;
  for (int j = begin + 1; j < end; ++j) {
    const int l = elev_level(a, j);
    if (l == prev) continue;
    if (l - prev > a.clearance) {      // a run begins
      if (a.use_ref && l <= a.vref) {  // (bottoms ascend: the last one at or below vref stays)
        run_at = j; top_at = j; bottom = l; top = l; levels = 1;
      } else {
        next_at = j;
        break;
      }
    } else {
      top_at = j; top = l; levels += 1;
    }
    prev = l;
  }
  uint32_t n_top = 0u, n_any = 0u;
  const float elevation = elev_level_mean(a, top_at, next_at, &n_top);
  const float low = elev_level_mean(a, run_at, next_at, &n_any);
  float ceiling = __uint_as_float(0x7f800000u);
  if (next_at < end) ceiling = elev_level_mean(a, next_at, end, &n_any);
  uint32_t label = 0u;
  if (a.rows.hist) {  // the level's histograms added bin by bin; the fullest bin as map_fullest_bin picks it
    uint32_t best_n = 0u;
    for (int l = 0; l < a.stride; ++l) {
      uint32_t s = 0u;
      for (int j = top_at; j < next_at; ++j) s += a.rows.hist[(size_t)a.sval[j] * (size_t)a.stride + (size_t)l];
      if (l == 0 || s > best_n) { best_n = s; label = (uint32_t)l; }
    }
  }
  a.state[c] = 1;
  a.elevation[c] = elevation; a.bottom[c] = low; a.ceiling[c] = ceiling;
  a.label[c] = label; a.count[c] = n_top;
  a.level_top[c] = top; a.level_bottom[c] = bottom; a.n_levels[c] = levels;
}

// rules 6 and 7, one lane per cell of the window; the cells per class: one integer atomic per workgroup and class
__global__ __launch_bounds__(256) void elevation_stencil_kernel(MapElevationArgs a) {
  __shared__ int per_class[8];
  if (threadIdx.x < 8) per_class[threadIdx.x] = 0;
  __syncthreads();
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < (long long)a.W * a.H) {
    const int c = (int)t, i = c % a.W, j = c / a.W;
    int cls = 0, nb = 0;
    float step = __uint_as_float(kElevNaN);
    if (a.state[c]) {
      const float e = a.elevation[c];
      step = 0.0f;
      for (int dj = -1; dj <= 1; ++dj)
        for (int di = -1; di <= 1; ++di) {
          const int ni = i + di, nj = j + dj;
          if ((di == 0 && dj == 0) || ni < 0 || ni >= a.W || nj < 0 || nj >= a.H) continue;
          const int q = nj * a.W + ni;
          if (!a.state[q]) continue;
          const float d = fabsf(__fsub_rn(a.elevation[q], e));
          step = d > step ? d : step;
          nb += 1;
        }
      const uint32_t label = a.label[c];
      const float ceiling = a.ceiling[c];
      if ((a.n_blocked > 0 && elev_listed(a.blocked, a.n_blocked, label)) ||
          (a.n_drivable > 0 && !elev_listed(a.drivable, a.n_drivable, label)))
        cls = 2;
      else if (a.level_top[c] - a.level_bottom[c] > a.max_extent)
        cls = 3;
      else if (a.min_clearance > 0.0 && fabsf(ceiling) < __uint_as_float(0x7f800000u) && (double)__fsub_rn(ceiling, e) < a.min_clearance)
        cls = 4;
      else if ((double)step > a.max_step)
        cls = 5;
      else if (nb < a.min_neighbors)
        cls = 6;
      else
        cls = 1;
    }
    a.step[c] = step;
    a.neighbors[c] = (uint8_t)nb;
    a.cls[c] = (uint8_t)cls;
    atomicAdd(&per_class[cls], 1);
  }
  __syncthreads();
  if (threadIdx.x < 8 && per_class[threadIdx.x]) atomicAdd(&a.ctl[kElevClass + threadIdx.x], per_class[threadIdx.x]);
}

// rule 8, one lane per finite point: integrate's transform, the grid's key, the cell's elevation
__global__ __launch_bounds__(256) void elevation_point_kernel(MapElevationArgs a) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.n) return;
  const int at = a.keep ? a.keep[f] : f;
  if (at < 0 || at >= a.n_caller) return;  // (cannot happen; nothing beyond the buffers)
  const double x = a.px[f], y = a.py[f], z = a.pz[f];
  const float px = voxel_xform_row(a.M + 0, x, y, z);
  const float py = voxel_xform_row(a.M + 4, x, y, z);
  const float pz = voxel_xform_row(a.M + 8, x, y, z);
  u64 key;
  if (!voxel_key(px, py, pz, a.inv_leaf, &key)) return;
  int vx, vy, vz;
  voxel_key_coords(key, &vx, &vy, &vz);
  const int c = elev_cell_of(a, vx, vy);
  if (c < 0) return;
  a.point_cell[at] = c;
  if (a.state[c]) a.point_height[at] = __fsub_rn(pz, a.elevation[c]);
}

inline dim3 elev_grid(long long n) { return dim3((unsigned)((std::max(n, 1ll) + 255) / 256)); }

}  // namespace

hipError_t launch_elevation_init(const MapElevationArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(elevation_init_kernel, elev_grid(std::max((long long)a.W * a.H, (long long)a.n_caller)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_elevation_keys(const MapElevationArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  hipLaunchKernelGGL(elevation_key_kernel, elev_grid(a.n_map), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_elevation_heads(const MapElevationArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  hipLaunchKernelGGL(elevation_heads_kernel, elev_grid(a.n_map), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_elevation_segments(const MapElevationArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  hipLaunchKernelGGL(elevation_segment_kernel, elev_grid(a.n_map), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_elevation_cells(const MapElevationArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  // (the occupied cells' number is on the device: no more than the rows, no more than the window)
  hipLaunchKernelGGL(elevation_cell_kernel, elev_grid(std::min((long long)a.n_map, (long long)a.W * a.H)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_elevation_stencil(const MapElevationArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(elevation_stencil_kernel, elev_grid((long long)a.W * a.H), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_elevation_points(const MapElevationArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(elevation_point_kernel, elev_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sicp
