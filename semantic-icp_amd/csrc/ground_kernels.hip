// ground_kernels.hip -- sicp_segment_ground: piecewise-planar ground on a polar grid (driver: ground.cpp; the rules:
// include/sicp.h, "ground of a cloud").  A lane per point forms the cell and the sort key; one stable sort of (key, caller
// index) makes every cell one segment, lowest z first; a pass finds the segments and writes the sorted coordinates densely, so
// that the fit streams.  The fit kernel gives one wave a whole cell: the seeds, n_iter x (centroid pass, product pass with the
// membership predicate recomputed from the previous model), the Jacobi on every lane alike, the tests, one last counting
// pass, the row stored by lane 0.  Member j belongs to lane j mod 64 and the lanes combine by a butterfly, so a cell's sums are
// the same for every grid; the grid has a wave per cell, dispatched in cell order (the dense near cells first).  A lane per
// point then writes the flag and the height.  Counts are integers, no float atomics.
#include <hip/hip_runtime.h>

#include "device_geometry.hpp"
#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

__device__ __forceinline__ int finite_of(const GroundArgs& a, int i) { return a.finv ? a.finv[i] : i; }

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// rules 1 - 3: the cell, the candidate test and the key
__global__ __launch_bounds__(256) void ground_key_kernel(GroundArgs a) {
  __shared__ double tab[kGroundMaxRings + 1 + kGroundMaxSectors];
  const int R = a.R, S = a.S, half = S / 2;
  for (int t = threadIdx.x; t < R + 1 + S; t += 256) tab[t] = a.tables[t];
  __syncthreads();
  const double* edge2 = tab;
  const double* cos_half = tab + R + 1;
  const double* sin_half = cos_half + half;
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool cand = false, below = false;
  if (i < a.n_caller) {
    u64 key = (u64)(unsigned)(R * S) << 32;
    int cell = -1;
    const int f = finite_of(a, i);
    if (f >= 0) {
      const float zf = a.z[f];
      const double dx = __dsub_rn((double)a.x[f], a.org[0]), dy = __dsub_rn((double)a.y[f], a.org[1]), dz = __dsub_rn((double)zf, a.org[2]);
      const double r2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
      if (r2 >= edge2[0] && r2 < edge2[R]) {
        int ring = 0;
        for (int r = 1; r < R; ++r) ring += r2 >= edge2[r] ? 1 : 0;
        const bool lower = !(dy > 0.0 || (dy == 0.0 && dx > 0.0));
        const double xp = lower ? -dx : dx, yp = lower ? -dy : dy;
        int sector = lower ? half : 0;
        for (int j = 1; j < half; ++j) sector += __dsub_rn(__dmul_rn(cos_half[j], yp), __dmul_rn(sin_half[j], xp)) >= 0.0 ? 1 : 0;
        cell = ring * S + sector;
        bool ok = a.mask == nullptr || a.mask[i] != 0;
        if (ok && a.labels) {
          const uint32_t l = a.label[f];
          for (int k = 0; k < a.n_ignore; ++k) ok = ok && a.ignore[k] != l;
        }
        cand = ok && dz >= a.below;
        below = ok && !cand;
        if (cand) {
          const uint32_t b = __float_as_uint(zf);
          key = ((u64)(unsigned)cell << 32) | (u64)((b & 0x80000000u) ? ~b : (b ^ 0x80000000u));
        }
      }
    }
    a.key[i] = key;
    a.val[i] = i;
    a.cellv[i] = cell;
    a.cand[i] = cand ? 1 : 0;
  }
  const int nc = __syncthreads_count(cand ? 1 : 0), nb = __syncthreads_count(below ? 1 : 0);
  if (threadIdx.x == 0) {
    if (nc) atomicAdd(&a.ctl->n_candidates, nc);
    if (nb) atomicAdd(&a.ctl->n_below, nb);
  }
}

// the segments of the sorted keys (seg_begin / seg_end are zero for a cell without candidates) and the sorted coordinates
__global__ __launch_bounds__(256) void ground_segment_kernel(GroundArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n_caller) return;
  const int c = (int)(a.skey[j] >> 32), cp = j > 0 ? (int)(a.skey[j - 1] >> 32) : -1;
  if (c != cp) {
    a.seg_begin[c] = j;
    if (cp >= 0) a.seg_end[cp] = j;
  }
  if (j == a.n_caller - 1) a.seg_end[c] = a.n_caller;
  if (c < a.R * a.S) {
    const int f = finite_of(a, a.sval[j]);  // (a candidate is finite)
    a.sx[j] = a.x[f]; a.sy[j] = a.y[f]; a.sz[j] = a.z[f];
  }
}

// rule 5's combination of the 64 lane sums: pairs at distance 1, 2, 4, .. 32; every lane ends with T_6[0] (a + b == b + a)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v = __dadd_rn(v, __shfl_xor(v, off));
  return v;
}

// the set a pass runs over: the seeds (dz < ts) or the members a model selects ((u . (d - g)) < th)
struct GroundSet {
  bool seeds;
  double ts;
  double ux, uy, uz, gx, gy, gz, th;
  __device__ __forceinline__ bool has(double dx, double dy, double dz) const {
    if (seeds) return dz < ts;
    return dot3(ux, uy, uz, __dsub_rn(dx, gx), __dsub_rn(dy, gy), __dsub_rn(dz, gz)) < th;
  }
};

constexpr int kGroundUnroll = 4;  // members a lane has in flight; the order of a lane's additions is ascending j all the same

// MODE 0: count and the sums of d.  MODE 1: the six products of d - c.  MODE 2: count only.
template <int MODE>
__device__ __forceinline__ void ground_pass(const GroundArgs& a, const float* __restrict__ sx, const float* __restrict__ sy,
                                            const float* __restrict__ sz, int m, int lane, const GroundSet& set, double cx, double cy,
                                            double cz, int& count, double (&sum)[6]) {
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int cnt = 0;
  for (int base = 0; base < m; base += 64 * kGroundUnroll) {
    float x[kGroundUnroll], y[kGroundUnroll], z[kGroundUnroll];
#pragma unroll
    for (int k = 0; k < kGroundUnroll; ++k) {
      const int j = base + k * 64 + lane;
      const int jj = j < m ? j : 0;
      x[k] = sx[jj]; y[k] = sy[jj]; z[k] = sz[jj];
    }
#pragma unroll
    for (int k = 0; k < kGroundUnroll; ++k) {
      const int j = base + k * 64 + lane;
      const double dx = __dsub_rn((double)x[k], a.org[0]), dy = __dsub_rn((double)y[k], a.org[1]), dz = __dsub_rn((double)z[k], a.org[2]);
      const bool in = j < m && set.has(dx, dy, dz);
      cnt += __popcll(__ballot(in));  // (a scalar of the wave: every branch on a count is uniform)
      // (a sum that begins at +0.0 never becomes -0.0: adding +0.0 for a member outside the set leaves it as it is)
      if (MODE == 0) {
        s[0] = __dadd_rn(s[0], in ? dx : 0.0); s[1] = __dadd_rn(s[1], in ? dy : 0.0); s[2] = __dadd_rn(s[2], in ? dz : 0.0);
      } else if (MODE == 1) {
        const double ex = __dsub_rn(dx, cx), ey = __dsub_rn(dy, cy), ez = __dsub_rn(dz, cz);
        s[0] = __dadd_rn(s[0], in ? __dmul_rn(ex, ex) : 0.0); s[1] = __dadd_rn(s[1], in ? __dmul_rn(ey, ex) : 0.0);
        s[2] = __dadd_rn(s[2], in ? __dmul_rn(ey, ey) : 0.0); s[3] = __dadd_rn(s[3], in ? __dmul_rn(ez, ex) : 0.0);
        s[4] = __dadd_rn(s[4], in ? __dmul_rn(ez, ey) : 0.0); s[5] = __dadd_rn(s[5], in ? __dmul_rn(ez, ez) : 0.0);
      }
    }
  }
  if (MODE != 1) count = cnt;
  if (MODE == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) sum[k] = wave_sum(s[k]);
  } else if (MODE == 1) {
#pragma unroll
    for (int k = 0; k < 6; ++k) sum[k] = wave_sum(s[k]);
  }
}

// rules 4 - 6: one wave per cell, four cells a workgroup.  The cell index, the segment and every count are scalars of the wave,
// so every branch around a lane exchange is uniform (a work counter fetched by lane 0 inside a loop was compiled
// into a loop that lane 0 left on its own, and never ended); the dispatcher hands out the workgroups in cell order.
__global__ __launch_bounds__(256) void ground_fit_kernel(GroundArgs a) {
  const int lane = threadIdx.x & 63;
  const int cell = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (cell >= a.R * a.S) return;
  const int begin = __builtin_amdgcn_readfirstlane(a.seg_begin[cell]), m = __builtin_amdgcn_readfirstlane(a.seg_end[cell]) - begin;
  const double nan = quiet_nan();
  GroundCell row;
  row.normal[0] = row.normal[1] = row.normal[2] = nan;
  row.centroid[0] = row.centroid[1] = row.centroid[2] = nan;
  row.lambda_min = nan; row.lpr = nan;
  row.status = kGroundEmpty; row.n_members = m; row.n_ground = 0; row.n_fit = 0;
  if (m > 0) {
    const float *sx = a.sx + begin, *sy = a.sy + begin, *sz = a.sz + begin;
    // rule 4: the first L members' dz, one per lane, added in order
    const int L = min(a.n_lpr, m);
    const double mine = lane < L ? __dsub_rn((double)sz[lane], a.org[2]) : 0.0;
    double lpr = 0.0;
    for (int k = 0; k < L; ++k) lpr = __dadd_rn(lpr, __shfl(mine, k));
    lpr = __ddiv_rn(lpr, (double)L);
    row.lpr = lpr;
    GroundSet set;
    set.seeds = true;
    set.ts = __dadd_rn(lpr, a.th_seeds);
    set.ux = set.uy = set.uz = set.gx = set.gy = set.gz = 0.0;
    set.th = a.th_dist;
    double lam = 0.0;
    int n_fit = 0;
    bool few = false;
    for (int it = 0; it < a.n_iter; ++it) {
      int count = 0;
      double sum[6];
      ground_pass<0>(a, sx, sy, sz, m, lane, set, 0.0, 0.0, 0.0, count, sum);
      if (count < a.min_points) { few = true; break; }
      const double cnt = (double)count;
      const double gx = __ddiv_rn(sum[0], cnt), gy = __ddiv_rn(sum[1], cnt), gz = __ddiv_rn(sum[2], cnt);
      int unused = 0;
      ground_pass<1>(a, sx, sy, sz, m, lane, set, gx, gy, gz, unused, sum);
      // the cyclic Jacobi of the covariance kernel (plane_fit_kernel), on every lane alike
      double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
      A[0][0] = sum[0];
      A[1][0] = A[0][1] = sum[1];
      A[1][1] = sum[2];
      A[2][0] = A[0][2] = sum[3];
      A[2][1] = A[1][2] = sum[4];
      A[2][2] = sum[5];
      for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (off <= 1e-300 || off <= 1e-34 * dia) break;
        jacobi_rotate(A, V, 0, 1);
        jacobi_rotate(A, V, 0, 2);
        jacobi_rotate(A, V, 1, 2);
      }
      const double e0 = fabs(A[0][0]), e1 = fabs(A[1][1]), e2 = fabs(A[2][2]);
      int col = 0;
      double em = e0;
      if (e1 <= em) { em = e1; col = 1; }
      if (e2 <= em) { em = e2; col = 2; }
      double ux = col == 0 ? V[0][0] : (col == 1 ? V[0][1] : V[0][2]);
      double uy = col == 0 ? V[1][0] : (col == 1 ? V[1][1] : V[1][2]);
      double uz = col == 0 ? V[2][0] : (col == 1 ? V[2][1] : V[2][2]);
      lam = col == 0 ? A[0][0] : (col == 1 ? A[1][1] : A[2][2]);
      if (uz < 0.0) { ux = -ux; uy = -uy; uz = -uz; }
      set.seeds = false;
      set.ux = ux; set.uy = uy; set.uz = uz; set.gx = gx; set.gy = gy; set.gz = gz;
      n_fit = count;
    }
    // rule 6
    const int ring = cell / a.S;
    if (few) row.status = kGroundTooFew;
    else if (!(set.uz >= a.min_cos)) row.status = kGroundNotUpright;
    else if (ring < a.elevation_rings && set.gz >= a.elev) row.status = kGroundTooHigh;
    else if (a.thick2 > 0.0 && lam > __dmul_rn(a.thick2, (double)n_fit)) row.status = kGroundTooThick;
    else row.status = kGroundOk;
    if (row.status == kGroundOk) {
      double none[6];
      int ground = 0;
      ground_pass<2>(a, sx, sy, sz, m, lane, set, 0.0, 0.0, 0.0, ground, none);
      row.normal[0] = set.ux; row.normal[1] = set.uy; row.normal[2] = set.uz;
      row.centroid[0] = set.gx; row.centroid[1] = set.gy; row.centroid[2] = set.gz;
      row.lambda_min = lam;
      row.n_ground = ground; row.n_fit = n_fit;
    }
  }
  if (lane == 0) a.cells[cell] = row;
}

// rules 7 and 8: the flag, the height and, with select, who goes to dst
__global__ __launch_bounds__(256) void ground_point_kernel(GroundArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_caller) return;
  const int cell = a.cellv[i];
  const int f = finite_of(a, i);
  double h = quiet_nan();
  bool ground = false;
  if (cell >= 0) {
    const int ring = cell / a.S, sector = cell - ring * a.S;
    int mc = -1;
    for (int r = ring; r >= 0 && mc < 0; --r)
      if (a.cells[r * a.S + sector].status == kGroundOk) mc = r * a.S + sector;
    if (mc >= 0) {
      const GroundCell& M = a.cells[mc];
      const double dx = __dsub_rn((double)a.x[f], a.org[0]), dy = __dsub_rn((double)a.y[f], a.org[1]), dz = __dsub_rn((double)a.z[f], a.org[2]);
      h = dot3(M.normal[0], M.normal[1], M.normal[2], __dsub_rn(dx, M.centroid[0]), __dsub_rn(dy, M.centroid[1]), __dsub_rn(dz, M.centroid[2]));
      ground = mc == cell && a.cand[i] != 0 && h < a.th_dist;
    }
  }
  a.oground[i] = ground ? 1 : 0;
  a.oheight[i] = h;
  if (a.select) a.flag[i] = (f >= 0 && ground == (a.select == 2)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void ground_select_kernel(GroundArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_caller) return;
  const int fl = a.flag[i], p = a.pos[i];
  if (fl) {
    const int f = finite_of(a, i);
    a.gx[p] = a.x[f]; a.gy[p] = a.y[f]; a.gz[p] = a.z[f];
    if (a.gl) a.gl[p] = a.label[f];
  }
  if (i == a.n_caller - 1) a.ctl->n_selected = p + fl;
}

inline dim3 grid256(long long n) { return dim3((unsigned)((n + 255) / 256)); }

bool ground_shape_ok(const GroundArgs& a) {
  return a.R >= 1 && a.R <= kGroundMaxRings && a.S >= 4 && a.S <= kGroundMaxSectors && a.S % 2 == 0 && a.n_lpr >= 1 && a.n_lpr <= 64;
}

}  // namespace

#define SICP_GROUND_POINTS(fn, kernel)                                    \
  hipError_t fn(const GroundArgs& a, hipStream_t st) {                    \
    if (a.n_caller <= 0) return hipSuccess;                               \
    if (!ground_shape_ok(a)) return hipErrorInvalidValue;                 \
    hipLaunchKernelGGL(kernel, grid256(a.n_caller), dim3(256), 0, st, a); \
    return hipGetLastError();                                             \
  }
SICP_GROUND_POINTS(launch_ground_keys, ground_key_kernel)
SICP_GROUND_POINTS(launch_ground_segments, ground_segment_kernel)
SICP_GROUND_POINTS(launch_ground_points, ground_point_kernel)
SICP_GROUND_POINTS(launch_ground_select, ground_select_kernel)
#undef SICP_GROUND_POINTS

// four waves a workgroup, a wave per cell
hipError_t launch_ground_fit(const GroundArgs& a, hipStream_t st) {
  if (!ground_shape_ok(a)) return hipErrorInvalidValue;
  const int blocks = (a.R * a.S + 3) / 4;
  hipLaunchKernelGGL(ground_fit_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sicp
