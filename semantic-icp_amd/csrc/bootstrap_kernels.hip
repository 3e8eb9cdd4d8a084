// bootstrap_kernels.hip -- the initial alignment without a pose prior (exec/bootstrap.h): voxel-grid keypoints, radius
// neighbourhoods, normals, FPFH features, the 33-D feature k-NN and the truncated error of SAC-IA hypotheses.
// The host driver is bootstrap.cpp; orders and precisions are fixed in INTEGRATION.md ("Bootstrap").  No floating-point
// atomics: every sum runs in a fixed order, so every output is run-to-run bit-reproducible.
#include <hip/hip_runtime.h>

#define SICP_HD __host__ __device__
#include "device_geometry.hpp"
#include "job_table.hpp"
#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

__device__ __forceinline__ bool boot_kept(float x, float y, float z, double box_max) {
  return (double)x < box_max && (double)y < box_max && (double)z < box_max;  // signed, bootstrap.h:24-28
}

// (the job forms -- one launch over every cloud or pair of a batch -- find a block's job with job_of: job_table.hpp)

// ---- voxel grid ----------------------------------------------------------------------------------------------------
// per workgroup: min / max of the kept points and their count -> blk[b * 8 + (lo0 lo1 lo2 hi0 hi1 hi2 count)]
// (LAB: a point whose label is in the ignore list is not kept either)
__device__ __forceinline__ bool boot_ignored(const BootIgnore& ig, unsigned l) {
  bool hit = false;
  for (int k = 0; k < ig.n; ++k) hit = hit || ig.v[k] == l;
  return hit;
}

template <bool LAB>
__device__ __forceinline__ void boot_bounds_body(int n, const float* x, const float* y, const float* z, const unsigned* label,
                                                 const BootIgnore* ig, double box_max, float* blk) {
  __shared__ float s[7][256];
  const int t = threadIdx.x, i = blockIdx.x * 256 + t;
  const float inf = __builtin_inff();
  float v[7] = {inf, inf, inf, -inf, -inf, -inf, 0.f};
  if (i < n) {
    const float px = x[i], py = y[i], pz = z[i];
    bool kept = boot_kept(px, py, pz, box_max);
    if (LAB) kept = kept && !boot_ignored(*ig, label[i]);
    if (kept) { v[0] = v[3] = px; v[1] = v[4] = py; v[2] = v[5] = pz; v[6] = 1.f; }
  }
  for (int k = 0; k < 7; ++k) s[k][t] = v[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      for (int k = 0; k < 3; ++k) s[k][t] = fminf(s[k][t], s[k][t + w]);
      for (int k = 3; k < 6; ++k) s[k][t] = fmaxf(s[k][t], s[k][t + w]);
      s[6][t] = s[6][t] + s[6][t + w];  // (integers below 2^24: exact)
    }
    __syncthreads();
  }
  if (t < 7) blk[blockIdx.x * 8 + t] = s[t][0];
}
__global__ __launch_bounds__(256) void boot_bounds_kernel(int n, const float* x, const float* y, const float* z,
                                                          double box_max, float* blk) {
  boot_bounds_body<false>(n, x, y, z, nullptr, nullptr, box_max, blk);
}
__global__ __launch_bounds__(256) void boot_bounds_ignore_kernel(int n, const float* x, const float* y, const float* z,
                                                                 const unsigned* label, BootIgnore ig, double box_max, float* blk) {
  boot_bounds_body<true>(n, x, y, z, label, &ig, box_max, blk);
}

// key = voxel index << 32 | point index (kept points), ~0 otherwise: sorted, points of one voxel are adjacent and in
// ascending index order
template <bool LAB>
__device__ __forceinline__ void boot_voxel_key_body(int n, const float* x, const float* y, const float* z, const unsigned* label,
                                                    const BootIgnore* ig, double box_max, float inv_leaf, int mb0, int mb1, int mb2,
                                                    int dx, int dxy, u64* key) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float px = x[i], py = y[i], pz = z[i];
  u64 k = ~0ull;
  bool kept = boot_kept(px, py, pz, box_max);
  if (LAB) kept = kept && !boot_ignored(*ig, label[i]);
  if (kept) {
    const int i0 = (int)floorf(px * inv_leaf) - mb0;
    const int i1 = (int)floorf(py * inv_leaf) - mb1;
    const int i2 = (int)floorf(pz * inv_leaf) - mb2;
    const unsigned idx = (unsigned)(i0 + i1 * dx + i2 * dxy);
    k = ((u64)idx << 32) | (unsigned)i;
  }
  key[i] = k;
}
__global__ __launch_bounds__(256) void boot_voxel_key_kernel(int n, const float* x, const float* y, const float* z,
                                                             double box_max, float inv_leaf, int mb0, int mb1, int mb2,
                                                             int dx, int dxy, u64* key) {
  boot_voxel_key_body<false>(n, x, y, z, nullptr, nullptr, box_max, inv_leaf, mb0, mb1, mb2, dx, dxy, key);
}
__global__ __launch_bounds__(256) void boot_voxel_key_ignore_kernel(int n, const float* x, const float* y, const float* z,
                                                                    const unsigned* label, BootIgnore ig, double box_max,
                                                                    float inv_leaf, int mb0, int mb1, int mb2, int dx, int dxy,
                                                                    u64* key) {
  boot_voxel_key_body<true>(n, x, y, z, label, &ig, box_max, inv_leaf, mb0, mb1, mb2, dx, dxy, key);
}

__global__ __launch_bounds__(256) void boot_heads_kernel(int n_kept, const u64* key, int* flag) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_kept) return;
  flag[j] = (j == 0 || (key[j] >> 32) != (key[j - 1] >> 32)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void boot_compact_kernel(int n_kept, const int* flag, const int* pos, int* heads, int* n_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_kept) return;
  if (flag[j]) heads[pos[j]] = j;
  if (j == n_kept - 1) *n_out = pos[j] + flag[j];
}

// one keypoint per voxel: the f64 sum of its points in ascending index order / count, rounded once to f32
__global__ __launch_bounds__(256) void boot_centroid_kernel(int n_kp, int n_kept, const int* heads, const u64* key,
                                                            const float* x, const float* y, const float* z,
                                                            float* kx, float* ky, float* kz) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_kp) return;
  const int b = heads[k], e = k + 1 < n_kp ? heads[k + 1] : n_kept;
  double sx = 0, sy = 0, sz = 0;
  for (int j = b; j < e; ++j) {
    const unsigned i = (unsigned)(key[j] & 0xffffffffull);
    sx += (double)x[i]; sy += (double)y[i]; sz += (double)z[i];
  }
  const double c = (double)(e - b);
  kx[k] = (float)(sx / c); ky[k] = (float)(sy / c); kz[k] = (float)(sz / c);
}

// one wave per voxel: the most frequent label of its points, ties to the smallest label (the rule of sicp_merge_clouds).
// Integer counts only.  The wave walks the voxel's distinct labels in ascending order: every pass counts the points with
// the current label and finds the smallest label above it (lanes stride over the voxel's range of the sorted keys, then a
// butterfly over the wave), so a voxel of c points with d distinct labels costs (d + 1) * ceil(c / 64) loads per lane --
// two points or several hundred alike -- and `>` keeps the smallest label among equal counts.
__global__ __launch_bounds__(256) void boot_label_vote_kernel(int n_kp, int n_kept, const int* heads, const u64* key,
                                                              const unsigned* label, unsigned* klabel) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= n_kp) return;  // (a whole wave)
  const int b = heads[k], e = k + 1 < n_kp ? heads[k + 1] : n_kept;
  bool started = false;  // false: the first pass only looks for the smallest label
  unsigned cur = 0, best = 0;
  int best_cnt = 0;
  for (;;) {
    int cnt = 0;
    unsigned nxt = 0xffffffffu;
    bool more = false;
    for (int j = b + lane; j < e; j += 64) {
      const unsigned l = label[(unsigned)(key[j] & 0xffffffffull)];
      if (started && l == cur) ++cnt;
      else if (!started || l > cur) { more = true; nxt = l < nxt ? l : nxt; }
    }
    for (int w = 32; w > 0; w >>= 1) {
      cnt += __shfl_xor(cnt, w, 64);
      const unsigned o = __shfl_xor(nxt, w, 64);
      nxt = o < nxt ? o : nxt;
    }
    if (started && cnt > best_cnt) { best_cnt = cnt; best = cur; }
    if (__ballot(more) == 0ull) break;
    cur = nxt;
    started = true;
  }
  if (lane == 0) klabel[k] = best;
}

// ---- radius neighbourhoods: a uniform grid of cells a little larger than the radius ---------------------------------
constexpr int kCellBias = 1 << 20;
__device__ __forceinline__ int boot_cell(float p, float inv_cell) {
  float c = floorf(p * inv_cell);
  c = fminf(fmaxf(c, (float)(-kCellBias + 2)), (float)(kCellBias - 3));  // (non-expansive: neighbours stay in adjacent cells)
  return (int)c;
}
__device__ __forceinline__ u64 boot_cell_key(int c0, int c1, int c2) {
  return ((u64)(unsigned)(c0 + kCellBias) << 42) | ((u64)(unsigned)(c1 + kCellBias) << 21) | (u64)(unsigned)(c2 + kCellBias);
}

__global__ __launch_bounds__(256) void boot_cell_key_kernel(int m, const float* x, const float* y, const float* z, float inv_cell,
                                                            u64* key, int* val) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  key[i] = boot_cell_key(boot_cell(x[i], inv_cell), boot_cell(y[i], inv_cell), boot_cell(z[i], inv_cell));
  val[i] = i;
}

__device__ __forceinline__ int boot_lower_bound(const u64* a, int n, u64 v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// d^2 = (dx dx + dy dy) + dz dz in f32; a neighbour when d^2 < r^2.  FILL = 0: count, 1: write (d^2 bits << 32 | index)
template <int FILL>
__global__ __launch_bounds__(256) void boot_radius_kernel(const BootCloudJob* jobs, const int* blk_end, int nj) {
  int lb;
  const BootCloudJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &lb)];
  const int i = lb * 256 + threadIdx.x, m = J.m;
  if (i >= m) return;
  const float *x = J.x, *y = J.y, *z = J.z;
  const float inv_cell = J.inv_cell, r2 = J.r2;
  const u64* skey = J.skey;
  const int* sval = J.sval;
  const float px = x[i], py = y[i], pz = z[i];
  const int c0 = boot_cell(px, inv_cell), c1 = boot_cell(py, inv_cell), c2 = boot_cell(pz, inv_cell);
  long long w = FILL ? J.loff[i] : 0;
  for (int a = -1; a <= 1; ++a)
    for (int b = -1; b <= 1; ++b) {
      // the three cells (c0 + a, c1 + b, c2 - 1 .. c2 + 1) are adjacent keys: one range
      const u64 k_lo = boot_cell_key(c0 + a, c1 + b, c2 - 1), k_hi = boot_cell_key(c0 + a, c1 + b, c2 + 1);
      int j = boot_lower_bound(skey, m, k_lo);
      for (; j < m && skey[j] <= k_hi; ++j) {
        const int q = sval[j];
        const float ddx = x[q] - px, ddy = y[q] - py, ddz = z[q] - pz;
        const float d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
        if (d2 < r2) {
          if (FILL) J.list[w] = ((u64)__float_as_uint(d2) << 32) | (unsigned)q;
          ++w;
        }
      }
    }
  if (!FILL) J.count[i] = w;
}

__global__ __launch_bounds__(256) void boot_split_kernel(long long total, const u64* list, int* idx, float* d2) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= total) return;
  const u64 k = list[j];
  idx[j] = (int)(k & 0xffffffffull);
  d2[j] = __uint_as_float((unsigned)(k >> 32));
}

// ---- normals: f64 covariance of the neighbourhood, smallest-eigenvalue eigenvector, flipped towards (0, 0, 0) -------
// (the lists of the normal radius: noff / nidx)
__global__ __launch_bounds__(256) void boot_normal_kernel(const BootCloudJob* jobs, const int* blk_end, int nj) {
  int lb;
  const BootCloudJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &lb)];
  const int i = lb * 256 + threadIdx.x;
  if (i >= J.m) return;
  const float *x = J.x, *y = J.y, *z = J.z;
  const long long* off = J.noff;
  const int* idx = J.nidx;
  double* n3 = J.n3;
  const long long b = off[i], e = off[i + 1];
  const double nan = __builtin_nan("");
  if (e - b < 3) { n3[3 * i] = n3[3 * i + 1] = n3[3 * i + 2] = nan; return; }
  double m0 = 0, m1 = 0, m2 = 0;
  for (long long j = b; j < e; ++j) { const int q = idx[j]; m0 += (double)x[q]; m1 += (double)y[q]; m2 += (double)z[q]; }
  const double cnt = (double)(e - b);
  m0 /= cnt; m1 /= cnt; m2 /= cnt;
  double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
  for (long long j = b; j < e; ++j) {
    const int q = idx[j];
    const double d0 = (double)x[q] - m0, d1 = (double)y[q] - m1, d2 = (double)z[q] - m2;
    c00 += d0 * d0; c01 += d0 * d1; c02 += d0 * d2; c11 += d1 * d1; c12 += d1 * d2; c22 += d2 * d2;
  }
  double A[3][3] = {{c00 / cnt, c01 / cnt, c02 / cnt}, {c01 / cnt, c11 / cnt, c12 / cnt}, {c02 / cnt, c12 / cnt, c22 / cnt}};
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 30; ++sweep) {  // the sweep of cov_body (feature_kernels.hip)
    const double offd = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (offd <= 1e-300 || offd <= 1e-34 * dia) break;
    jacobi_rotate(A, V, 0, 1);
    jacobi_rotate(A, V, 0, 2);
    jacobi_rotate(A, V, 1, 2);
  }
  const double e0 = fabs(A[0][0]), e1 = fabs(A[1][1]), e2 = fabs(A[2][2]);
  int col = 0;
  double em = e0;
  if (e1 <= em) { em = e1; col = 1; }
  if (e2 <= em) { em = e2; col = 2; }
  double nx = V[0][col], ny = V[1][col], nz = V[2][col];
  const double px = x[i], py = y[i], pz = z[i];
  if ((-px) * nx + (-py) * ny + (-pz) * nz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
  n3[3 * i] = nx; n3[3 * i + 1] = ny; n3[3 * i + 2] = nz;
}

// ---- FPFH ----------------------------------------------------------------------------------------------------------
// pcl::computePairFeatures(p1, n1, p2, n2) in f64; false where PCL returns false (coincident points, parallel frame)
__device__ __forceinline__ bool boot_pair_features(double p1x, double p1y, double p1z, double n1x, double n1y, double n1z,
                                                   double p2x, double p2y, double p2z, double n2x, double n2y, double n2z,
                                                   double& f1, double& f2, double& f3) {
  double dx = p2x - p1x, dy = p2y - p1y, dz = p2z - p1z;
  const double f4 = sqrt((dx * dx + dy * dy) + dz * dz);
  if (f4 == 0.0) return false;
  const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / f4;
  const double a2 = ((n2x * dx + n2y * dy) + n2z * dz) / f4;
  double ux = n1x, uy = n1y, uz = n1z, mx = n2x, my = n2y, mz = n2z;
  if (fabs(a1) < fabs(a2)) {  // acos(|a1|) > acos(|a2|): the swap rule
    ux = n2x; uy = n2y; uz = n2z; mx = n1x; my = n1y; mz = n1z;
    dx = -dx; dy = -dy; dz = -dz;
    f3 = -a2;
  } else {
    f3 = a1;
  }
  double vx = dy * uz - dz * uy, vy = dz * ux - dx * uz, vz = dx * uy - dy * ux;  // v = dp x u
  const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
  if (vn == 0.0) return false;
  vx /= vn; vy /= vn; vz /= vn;
  const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;  // w = u x v
  f2 = (vx * mx + vy * my) + vz * mz;
  f1 = atan2((wx * mx + wy * my) + wz * mz, (ux * mx + uy * my) + uz * mz);
  return true;
}

__device__ __forceinline__ int boot_bin(double v) {
  const int b = (int)floor(v);
  return b < 0 ? 0 : (b > 10 ? 10 : b);
}

// one wave per point: SPFH counts in LDS (integer atomics: order-free), each pair adds 100 / (|neighbourhood| - 1)
// (block = point: blk_end is the prefix of the keypoint counts)
__global__ __launch_bounds__(64) void boot_spfh_kernel(const BootCloudJob* jobs, const int* blk_end, int nj) {
  __shared__ int h[33];
  int p;
  const BootCloudJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &p)];
  const int t = threadIdx.x;
  const float *x = J.x, *y = J.y, *z = J.z;
  const double* n3 = J.n3;
  const long long* off = J.off;
  const int* idx = J.idx;
  double* spfh = J.spfh;
  if (t < 33) h[t] = 0;
  __syncthreads();
  const double n1x = n3[3 * p], n1y = n3[3 * p + 1], n1z = n3[3 * p + 2];
  const bool valid = !isnan(n1x);
  const long long b = off[p], e = off[p + 1];
  if (valid) {
    const double px = x[p], py = y[p], pz = z[p];
    for (long long j = b + t; j < e; j += 64) {
      const int q = idx[j];
      if (q == p) continue;
      const double n2x = n3[3 * q], n2y = n3[3 * q + 1], n2z = n3[3 * q + 2];
      if (isnan(n2x)) continue;
      double f1, f2, f3;
      if (!boot_pair_features(px, py, pz, n1x, n1y, n1z, x[q], y[q], z[q], n2x, n2y, n2z, f1, f2, f3)) continue;
      atomicAdd(&h[boot_bin(11.0 * (f1 + M_PI) / (2.0 * M_PI))], 1);
      atomicAdd(&h[11 + boot_bin(11.0 * (f2 + 1.0) / 2.0)], 1);
      atomicAdd(&h[22 + boot_bin(11.0 * (f3 + 1.0) / 2.0)], 1);
    }
  }
  __syncthreads();
  if (t < 33) spfh[(size_t)p * 33 + t] = valid ? (double)h[t] * (100.0 / (double)(e - b - 1)) : __builtin_nan("");
}

// one wave per point, lane = bin: sum SPFH(q) / d^2 over the neighbours with d^2 > 0 in list order (f64), then each
// third scaled to a sum of 100 (its 11 bins summed in bin order)
__global__ __launch_bounds__(64) void boot_fpfh_kernel(const BootCloudJob* jobs, const int* blk_end, int nj) {
  __shared__ double acc[33];
  int p;
  const BootCloudJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &p)];
  const int t = threadIdx.x;
  const double* n3 = J.n3;
  const long long* off = J.off;
  const int* idx = J.idx;
  const float* d2 = J.d2;
  const double* spfh = J.spfh;
  float* fpfh = J.fpfh;
  if (isnan(n3[3 * p])) {
    if (t < 33) fpfh[(size_t)p * 33 + t] = __builtin_nanf("");
    return;
  }
  double a = 0.0;
  const long long b = off[p], e = off[p + 1];
  for (long long j = b; j < e; ++j) {
    const float dd = d2[j];
    if (!(dd > 0.f)) continue;
    const int q = idx[j];
    if (isnan(n3[3 * q])) continue;
    if (t < 33) a += spfh[(size_t)q * 33 + t] / (double)dd;
  }
  if (t < 33) acc[t] = a;
  __syncthreads();
  if (t < 33) {
    const int third = t / 11 * 11;
    double s = 0.0;
    for (int k = 0; k < 11; ++k) s += acc[third + k];
    fpfh[(size_t)p * 33 + t] = (float)(s != 0.0 ? a * (100.0 / s) : a);
  }
}

// ---- feature k-NN: f32 L2 over bins 0..32 in order, ties to the lower index; target features tiled through LDS --------
constexpr int kKnnTile = 64;
// (job = pair: n source features sf, nt target features tf -> out[n][k]).  A feature row is NaN in all 33 bins or in none
// (boot_fpfh_kernel), so the source's test of every bin and the target's of bin 0 are one rule: "has a feature".
// LAB: the label form -- the tile carries the target keypoints' labels beside ok[], and a row of another label than the
// source keypoint's is passed over like a row without a feature.
template <bool LAB>
__global__ __launch_bounds__(256) void boot_feature_knn_kernel(const BootPairJob* jobs, const int* blk_end, int nj, int k) {
  __shared__ float tile[kKnnTile][33];
  __shared__ int ok[kKnnTile];
  __shared__ unsigned tlab[LAB ? kKnnTile : 1];
  int lb;
  const BootPairJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &lb)];
  const int ns = J.n, nt = J.nt;
  const float *sf = J.sf, *tf = J.tf;
  int* out = J.out;
  const int i = lb * 256 + threadIdx.x;
  float qf[33];
  bool qvalid = false;
  unsigned ql = 0;
  if (LAB && i < ns) ql = J.sl[i];
  if (i < ns) {
    qvalid = true;
#pragma unroll
    for (int b = 0; b < 33; ++b) { qf[b] = sf[(size_t)i * 33 + b]; qvalid = qvalid && !isnan(qf[b]); }
  } else {
#pragma unroll
    for (int b = 0; b < 33; ++b) qf[b] = 0.f;
  }
  float bd[kBootMaxK];
  int bi[kBootMaxK];
#pragma unroll
  for (int r = 0; r < kBootMaxK; ++r) { bd[r] = __builtin_inff(); bi[r] = -1; }
  for (int t0 = 0; t0 < nt; t0 += kKnnTile) {
    __syncthreads();
    for (int e = threadIdx.x; e < kKnnTile * 33; e += 256) {
      const int r = e / 33, c = e % 33;
      tile[r][c] = t0 + r < nt ? tf[(size_t)(t0 + r) * 33 + c] : 0.f;
    }
    if (threadIdx.x < kKnnTile) ok[threadIdx.x] = t0 + (int)threadIdx.x < nt && !isnan(tf[(size_t)(t0 + threadIdx.x) * 33]);
    if (LAB && threadIdx.x < kKnnTile) tlab[threadIdx.x] = t0 + (int)threadIdx.x < nt ? J.tl[t0 + threadIdx.x] : 0u;
    __syncthreads();
    const int cnt = nt - t0 < kKnnTile ? nt - t0 : kKnnTile;
    if (!qvalid) continue;
    for (int r = 0; r < cnt; ++r) {
      if (!ok[r]) continue;
      if (LAB && tlab[r] != ql) continue;
      float d = 0.f;
#pragma unroll
      for (int b = 0; b < 33; ++b) { const float df = qf[b] - tile[r][b]; d = d + df * df; }
      if (!(d < bd[kBootMaxK - 1])) continue;  // (a later index never displaces an equal distance)
      // insert behind every entry at most as far, then move the rest down one place each.  (The rest moves whatever it
      // compares to: a displaced entry tested with `<` again would jump over an entry at its own distance, and two
      // target rows with the same distance would swap whenever a nearer row arrived after them.)
      float cd = d;
      int ci = t0 + r;
      bool moving = false;
#pragma unroll
      for (int s = 0; s < kBootMaxK; ++s) {
        moving = moving || cd < bd[s];
        if (moving) { const float td = bd[s]; const int ti = bi[s]; bd[s] = cd; bi[s] = ci; cd = td; ci = ti; }
      }
    }
  }
  if (i >= ns) return;
#pragma unroll
  for (int r = 0; r < kBootMaxK; ++r)
    if (r < k) out[(size_t)i * k + r] = qvalid ? bi[r] : -1;
}

// ---- truncated error of every hypothesis: one workgroup each, fixed-shape f64 sum of (e <= t ? e / t : 1) ------------
// (job = the hypotheses of one pair in a chunk, block = hypothesis: n hypotheses of nt squared distances each, d2 -> err)
// LAB: the label form -- a distance within t counts as e / t only when the neighbour the search found (nbr: its index in the
// target tree's device order, as the search writes it; rows in the source tree's device order) has the source keypoint's
// label, and as 1 otherwise.
template <bool LAB>
__global__ __launch_bounds__(256) void boot_error_kernel(const BootPairJob* jobs, const int* blk_end, int nj, double t) {
  __shared__ double s[256];
  int h;
  const BootPairJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &h)];
  const int l = threadIdx.x, nq = J.nt;
  double* err = J.err;
  const float* d = J.d2 + (size_t)h * nq;
  double a = 0.0;
  for (int q = l; q < nq; q += 256) {
    const double e = (double)d[q];
    bool in = e <= t;
    if (LAB && in) {
      const int j = J.nbr[(size_t)h * nq + q];
      in = j >= 0 && J.tl[j] == J.sl[q];
    }
    a += in ? e / t : 1.0;
  }
  s[l] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (l < w) s[l] = s[l] + s[l + w];
    __syncthreads();
  }
  if (l == 0) err[h] = s[0];
}

inline dim3 boot_grid(long long n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }

}  // namespace

int boot_bounds_blocks(int n) { return (n + 255) / 256; }

// (ig == nullptr: the label-blind kernels, as launched before the label forms existed)
hipError_t launch_boot_bounds(int n, const float* x, const float* y, const float* z, const unsigned* label, const BootIgnore* ig,
                              double box_max, float* blk, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (ig && (ig->n < 0 || ig->n > kBootMaxIgnore)) return hipErrorInvalidValue;
  if (ig) hipLaunchKernelGGL(boot_bounds_ignore_kernel, boot_grid(n), dim3(256), 0, st, n, x, y, z, label, *ig, box_max, blk);
  else hipLaunchKernelGGL(boot_bounds_kernel, boot_grid(n), dim3(256), 0, st, n, x, y, z, box_max, blk);
  return hipGetLastError();
}

hipError_t launch_boot_voxel_keys(int n, const float* x, const float* y, const float* z, const unsigned* label, const BootIgnore* ig,
                                  double box_max, float inv_leaf, const int* min_b, int dx, int dxy, unsigned long long* key,
                                  hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (ig && (ig->n < 0 || ig->n > kBootMaxIgnore)) return hipErrorInvalidValue;
  if (ig)
    hipLaunchKernelGGL(boot_voxel_key_ignore_kernel, boot_grid(n), dim3(256), 0, st, n, x, y, z, label, *ig, box_max, inv_leaf,
                       min_b[0], min_b[1], min_b[2], dx, dxy, key);
  else
    hipLaunchKernelGGL(boot_voxel_key_kernel, boot_grid(n), dim3(256), 0, st, n, x, y, z, box_max, inv_leaf, min_b[0], min_b[1],
                       min_b[2], dx, dxy, key);
  return hipGetLastError();
}

hipError_t launch_boot_label_vote(int n_kp, int n_kept, const int* heads, const unsigned long long* key, const unsigned* label,
                                  unsigned* klabel, hipStream_t st) {
  if (n_kp <= 0) return hipSuccess;
  hipLaunchKernelGGL(boot_label_vote_kernel, boot_grid(n_kp, 4), dim3(256), 0, st, n_kp, n_kept, heads, key, label, klabel);
  return hipGetLastError();
}

hipError_t launch_boot_voxel_compact(int n_kept, const unsigned long long* key, int* flag, int* pos, int* heads, int* n_out,
                                     void* temp, size_t temp_bytes, hipStream_t st) {
  if (n_kept <= 0) return hipSuccess;
  hipLaunchKernelGGL(boot_heads_kernel, boot_grid(n_kept), dim3(256), 0, st, n_kept, key, flag);
  hipError_t e = prim_scan_int(temp, temp_bytes, flag, pos, n_kept, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(boot_compact_kernel, boot_grid(n_kept), dim3(256), 0, st, n_kept, flag, pos, heads, n_out);
  return hipGetLastError();
}

hipError_t launch_boot_centroids(int n_kp, int n_kept, const int* heads, const unsigned long long* key, const float* x,
                                 const float* y, const float* z, float* kx, float* ky, float* kz, hipStream_t st) {
  if (n_kp <= 0) return hipSuccess;
  hipLaunchKernelGGL(boot_centroid_kernel, boot_grid(n_kp), dim3(256), 0, st, n_kp, n_kept, heads, key, x, y, z, kx, ky, kz);
  return hipGetLastError();
}

hipError_t launch_boot_cell_keys(int m, const float* x, const float* y, const float* z, float inv_cell, unsigned long long* key,
                                 int* val, hipStream_t st) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(boot_cell_key_kernel, boot_grid(m), dim3(256), 0, st, m, x, y, z, inv_cell, key, val);
  return hipGetLastError();
}

hipError_t launch_boot_radius_jobs(int fill, const BootCloudJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st) {
  if (nj <= 0 || blocks <= 0) return hipSuccess;
  if (fill) hipLaunchKernelGGL(boot_radius_kernel<1>, dim3(blocks), dim3(256), 0, st, jobs, blk_end, nj);
  else hipLaunchKernelGGL(boot_radius_kernel<0>, dim3(blocks), dim3(256), 0, st, jobs, blk_end, nj);
  return hipGetLastError();
}

hipError_t launch_boot_split(long long total, const unsigned long long* list, int* idx, float* d2, hipStream_t st) {
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(boot_split_kernel, boot_grid(total), dim3(256), 0, st, total, list, idx, d2);
  return hipGetLastError();
}

hipError_t launch_boot_normal_jobs(const BootCloudJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st) {
  if (nj <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(boot_normal_kernel, dim3(blocks), dim3(256), 0, st, jobs, blk_end, nj);
  return hipGetLastError();
}

hipError_t launch_boot_fpfh_jobs(const BootCloudJob* jobs, const int* pt_end, int nj, int points, hipStream_t st) {
  if (nj <= 0 || points <= 0) return hipSuccess;
  hipLaunchKernelGGL(boot_spfh_kernel, dim3(points), dim3(64), 0, st, jobs, pt_end, nj);
  hipLaunchKernelGGL(boot_fpfh_kernel, dim3(points), dim3(64), 0, st, jobs, pt_end, nj);
  return hipGetLastError();
}

hipError_t launch_boot_feature_knn_jobs(const BootPairJob* jobs, const int* blk_end, int nj, int blocks, int k, bool same_label,
                                        hipStream_t st) {
  if (nj <= 0 || blocks <= 0) return hipSuccess;
  if (k < 1 || k > kBootMaxK) return hipErrorInvalidValue;
  if (same_label) hipLaunchKernelGGL(boot_feature_knn_kernel<true>, dim3(blocks), dim3(256), 0, st, jobs, blk_end, nj, k);
  else hipLaunchKernelGGL(boot_feature_knn_kernel<false>, dim3(blocks), dim3(256), 0, st, jobs, blk_end, nj, k);
  return hipGetLastError();
}

hipError_t launch_boot_error_jobs(const BootPairJob* jobs, const int* hyp_end, int nj, int hypotheses, double t, bool same_label,
                                  hipStream_t st) {
  if (nj <= 0 || hypotheses <= 0) return hipSuccess;
  if (same_label) hipLaunchKernelGGL(boot_error_kernel<true>, dim3(hypotheses), dim3(256), 0, st, jobs, hyp_end, nj, t);
  else hipLaunchKernelGGL(boot_error_kernel<false>, dim3(hypotheses), dim3(256), 0, st, jobs, hyp_end, nj, t);
  return hipGetLastError();
}

}  // namespace sicp
