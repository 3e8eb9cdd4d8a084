// distance_kernels.hip -- sicp_map_distance (include/sicp.h, "distance"; driver: distance.cpp; the launches' order and the
// packed key: kernels.h, MapDistanceArgs).  The field is the lexicographic minimum of (d^2, map row) over the obstacles, and
// that minimum is separable: three windowed-minimum sweeps over the dense window, along x, y and z, each reading and writing
// one 8-byte key a cell between two buffers.  Integer arithmetic and plain stores throughout (one 64-bit atomicMin per row
// seeds a column in planar mode), so every byte is run-to-run reproducible and independent of the launch shape.  The map is
// only read.
#include <hip/hip_runtime.h>

#include <algorithm>

#define SICP_HD __host__ __device__
#include "kernels.h"
#include "voxel_key.hpp"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

constexpr unsigned kDistNaN = 0x7fc00000u;  // the quiet NaN of a point without a range

__device__ __forceinline__ bool dist_listed(const uint32_t* list, int n, uint32_t l) {
  bool in = false;
  for (int j = 0; j < n; ++j) in = in || list[j] == l;
  return in;
}

__device__ __forceinline__ long long dist_cells(const MapDistanceArgs& a) { return (long long)a.nx * a.ny * a.nz; }

// the window's cell of the voxel (vx, vy, vz), -1 outside (planar: the column's; vz is not looked at)
__device__ __forceinline__ int dist_cell_of(const MapDistanceArgs& a, int vx, int vy, int vz) {
  const int i = vx - a.x0, j = vy - a.y0, k = a.planar ? 0 : vz - a.z0;
  if (i < 0 || i >= a.nx || j < 0 || j >= a.ny || k < 0 || k >= a.nz) return -1;
  return (k * a.ny + j) * a.nx + i;
}

// every cell "none"; every point "no cell" (rule 5)
__global__ __launch_bounds__(256) void distance_init_kernel(MapDistanceArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < dist_cells(a)) a.key[t] = kDistNone;
  if (t < a.n_caller) {
    a.point_cell[t] = -1;
    a.point_dist_sq[t] = -1;
    a.point_nearest[t] = -1;
    a.point_range_sq[t] = __uint_as_float(kDistNaN);
  }
}

// rules 2 and 3, one lane per map row: a row that counts seeds its cell with (0, row) -- a plain store in 3-D, where a voxel
// has one row; a 64-bit atomicMin in planar mode, where the smallest row of a column stays.  The obstacle cells: one integer
// atomic per workgroup.
__global__ __launch_bounds__(256) void distance_seed_kernel(MapDistanceArgs a) {
  __shared__ int seeded;
  if (threadIdx.x == 0) seeded = 0;
  __syncthreads();
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < a.n_map) {
    int vx, vy, vz;
    voxel_key_coords(a.rows.key[r], &vx, &vy, &vz);
    const int c = dist_cell_of(a, vx, vy, vz);
    bool counts = c >= 0 && (long long)a.rows.cnt[r] >= a.min_count && (!a.planar || (vz >= a.lo && vz <= a.hi));
    if (counts && a.rows.hist) {
      const uint32_t l = map_fullest_bin(a.rows.hist + (size_t)r * (size_t)a.stride, a.stride);
      a.row_label[r] = l;
      if (a.n_ignore > 0 && dist_listed(a.ignore, a.n_ignore, l)) counts = false;
      if (a.n_only > 0 && !dist_listed(a.only, a.n_only, l)) counts = false;
    }
    if (counts) {
      if (a.planar) {
        if (atomicMin(&a.key[c], (u64)(unsigned)r) == kDistNone) atomicAdd(&seeded, 1);  // (the column's first arrival counts it)
      } else {
        a.key[c] = (u64)(unsigned)r;
        atomicAdd(&seeded, 1);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && seeded) atomicAdd(&a.ctl[kDistObstacles], seeded);
}

// the windowed minimum of one cell: keys[-R .. R] about `at`, `step` keys apart
__device__ __forceinline__ u64 dist_window_min(const u64* at, int step, int R) {
  u64 best = at[0];
  for (int s = 1; s <= R; ++s) {
    const u64 add = (u64)(unsigned)(s * s) << 32;
    const u64 lo = at[-s * step] + add, hi = at[s * step] + add;
    best = lo < best ? lo : best;
    best = hi < best ? hi : best;
  }
  return best;
}

// the sweep along x: a workgroup stages kDistLineTile cells of one line and R cells of halo on either side in LDS ("none" beyond
// the line's ends), a lane takes the windowed minimum of its cell.  The grid is flat: block b is piece b % pieces of line
// b / pieces.
__global__ __launch_bounds__(kDistLineTile) void distance_sweep_x_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int nx, long long lines,
                                                                        int pieces, int R) {
  __shared__ u64 tile[kDistLineTile + 2 * kDistMaxR];
  const long long line = (long long)blockIdx.x / pieces;
  const int first = (int)((long long)blockIdx.x % pieces) * kDistLineTile;
  if (line >= lines) return;
  const u64* row = src + (size_t)line * (size_t)nx;
  for (int t = threadIdx.x; t < kDistLineTile + 2 * R; t += kDistLineTile) {
    const int i = first - R + t;
    tile[t] = (i >= 0 && i < nx) ? row[i] : kDistNone;
  }
  __syncthreads();
  const int i = first + (int)threadIdx.x;
  if (i < nx) dst[(size_t)line * (size_t)nx + (size_t)i] = dist_window_min(tile + threadIdx.x + R, 1, R);
}

// the sweeps along y and z: lanes run along x, so every global access is kDistTileX keys = 256 contiguous bytes; a workgroup of
// kDistTileX x 8 lanes stages kDistTileX x (kDistTileA + 2 R) keys in LDS ("none" beyond the axis' ends and the line's) and
// every lane takes the windowed minimum of kDistTileA / 8 cells of its column.  A cell is base + outer * stride_outer + a *
// stride_axis + i; the grid is flat: block b is x tile b % xt, axis tile (b / xt) % at, outer index b / (xt * at).
__global__ __launch_bounds__(256) void distance_sweep_axis_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int nx, int n_axis,
                                                                  long long stride_axis, int n_outer, long long stride_outer, int xt, int at, int R) {
  extern __shared__ u64 tile_dyn[];
  const int tx = threadIdx.x % kDistTileX, ty = threadIdx.x / kDistTileX;  // ty: 0..7
  const long long b = blockIdx.x;
  const int bx = (int)(b % xt), ba = (int)((b / xt) % at);
  const long long outer = b / ((long long)xt * at);
  if (outer >= n_outer) return;
  const int i = bx * kDistTileX + tx;
  const int a0 = ba * kDistTileA;
  const size_t base = (size_t)outer * (size_t)stride_outer + (size_t)i;
  for (int t = ty; t < kDistTileA + 2 * R; t += 8) {
    const int a = a0 - R + t;
    tile_dyn[t * kDistTileX + tx] = (i < nx && a >= 0 && a < n_axis) ? src[base + (size_t)a * (size_t)stride_axis] : kDistNone;
  }
  __syncthreads();
  if (i >= nx) return;
  for (int q = 0; q < kDistTileA / 8; ++q) {
    const int r = ty + 8 * q, a = a0 + r;
    if (a < n_axis) dst[base + (size_t)a * (size_t)stride_axis] = dist_window_min(tile_dyn + (r + R) * kDistTileX + tx, kDistTileX, R);
  }
}

// rule 4, one lane per cell: the ball's test, the key unpacked, the row's label; the reached cells and the largest d^2: one
// integer atomic each per workgroup
__global__ __launch_bounds__(256) void distance_final_kernel(MapDistanceArgs a, const u64* __restrict__ src) {
  __shared__ int reached, largest;
  if (threadIdx.x == 0) { reached = 0; largest = 0; }
  __syncthreads();
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  bool in = false;
  int far = 0;  // d^2 + 1 of a reached cell
  if (t < dist_cells(a)) {
    const u64 k = src[t];
    const u64 d2 = k >> 32;
    const int row = (int)(unsigned)(k & 0xffffffffull);
    in = d2 <= (u64)(a.R * a.R) && row >= 0 && row < a.n_map;  // (a reached key's row is a map row)
    far = in ? (int)d2 + 1 : 0;
    a.dist_sq[t] = in ? (int)d2 : -1;
    a.nearest[t] = in ? row : -1;
    a.label[t] = (in && a.row_label) ? a.row_label[row] : 0u;
  }
  // a wave's count and maximum first (every lane of the wave takes part), then one LDS atomic each per wave
  const u64 hit = __ballot(in);
  for (int off = 32; off > 0; off >>= 1) far = max(far, __shfl_xor(far, off));
  if ((threadIdx.x & 63) == 0 && hit) {
    atomicAdd(&reached, __popcll(hit));
    atomicMax(&largest, far);
  }
  __syncthreads();
  if (threadIdx.x == 0 && reached) {
    atomicAdd(&a.ctl[kDistReached], reached);
    atomicMax(&a.ctl[kDistMaxPlus1], largest);
  }
}

// rule 5, one lane per finite point: integrate's transform, the grid's key arithmetic, the cell's values
__global__ __launch_bounds__(256) void distance_point_kernel(MapDistanceArgs a) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.n) return;
  const int at = a.keep ? a.keep[f] : f;
  if (at < 0 || at >= a.n_caller) return;  // (cannot happen; nothing beyond the buffers)
  const double x = a.px[f], y = a.py[f], z = a.pz[f];
  const float px = voxel_xform_row(a.M + 0, x, y, z);
  const float py = voxel_xform_row(a.M + 4, x, y, z);
  const float pz = voxel_xform_row(a.M + 8, x, y, z);
  const float v0 = floorf(__fmul_rn(px, a.inv_leaf)), v1 = floorf(__fmul_rn(py, a.inv_leaf)), v2 = floorf(__fmul_rn(pz, a.inv_leaf));
  const float lim = (float)kMergeBias;
  if (!(fabsf(v0) < lim && fabsf(v1) < lim && (a.planar || fabsf(v2) < lim))) return;
  const int c = dist_cell_of(a, (int)v0, (int)v1, a.planar ? 0 : (int)v2);
  if (c < 0) return;
  const int row = a.nearest[c];
  a.point_cell[at] = c;
  a.point_dist_sq[at] = a.dist_sq[c];
  a.point_nearest[at] = row;
  if (!a.planar && row >= 0 && row < a.n_map) {
    const double n = (double)a.rows.cnt[row];
    const float cx = (float)(a.rows.sx[row] / n), cy = (float)(a.rows.sy[row] / n), cz = (float)(a.rows.sz[row] / n);
    const float dx = __fsub_rn(px, cx), dy = __fsub_rn(py, cy), dz = __fsub_rn(pz, cz);
    float d2 = __fmul_rn(dx, dx);
    d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
    d2 = __fadd_rn(d2, __fmul_rn(dz, dz));
    a.point_range_sq[at] = d2;
  }
  atomicAdd(&a.ctl[kDistInside], 1);
}

inline dim3 dist_grid(long long n) { return dim3((unsigned)((std::max(n, 1ll) + 255) / 256)); }

}  // namespace

hipError_t launch_distance_init(const MapDistanceArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(distance_init_kernel, dist_grid(std::max((long long)a.nx * a.ny * a.nz, (long long)a.n_caller)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_distance_seed(const MapDistanceArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  hipLaunchKernelGGL(distance_seed_kernel, dist_grid(a.n_map), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_distance_sweep(const MapDistanceArgs& a, int axis, const unsigned long long* src, unsigned long long* dst, hipStream_t st) {
  if (a.R < 1 || a.R > kDistMaxR) return hipErrorInvalidValue;
  const long long plane = (long long)a.nx * a.ny;
  if (axis == 0) {
    const int pieces = (a.nx + kDistLineTile - 1) / kDistLineTile;
    const long long lines = (long long)a.ny * a.nz;
    hipLaunchKernelGGL(distance_sweep_x_kernel, dim3((unsigned)(lines * pieces)), dim3(kDistLineTile), 0, st, src, dst, a.nx, lines, pieces, a.R);
    return hipGetLastError();
  }
  const int n_axis = axis == 1 ? a.ny : a.nz, n_outer = axis == 1 ? a.nz : a.ny;
  const long long stride_axis = axis == 1 ? (long long)a.nx : plane, stride_outer = axis == 1 ? plane : (long long)a.nx;
  const int xt = (a.nx + kDistTileX - 1) / kDistTileX, at = (n_axis + kDistTileA - 1) / kDistTileA;
  const size_t lds = (size_t)(kDistTileA + 2 * a.R) * kDistTileX * sizeof(unsigned long long);
  hipLaunchKernelGGL(distance_sweep_axis_kernel, dim3((unsigned)((long long)xt * at * n_outer)), dim3(256), lds, st, src, dst, a.nx, n_axis,
                     stride_axis, n_outer, stride_outer, xt, at, a.R);
  return hipGetLastError();
}

hipError_t launch_distance_final(const MapDistanceArgs& a, const unsigned long long* src, hipStream_t st) {
  hipLaunchKernelGGL(distance_final_kernel, dist_grid((long long)a.nx * a.ny * a.nz), dim3(256), 0, st, a, src);
  return hipGetLastError();
}

hipError_t launch_distance_points(const MapDistanceArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(distance_point_kernel, dist_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sicp
