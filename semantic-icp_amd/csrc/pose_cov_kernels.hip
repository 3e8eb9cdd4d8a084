// pose_cov_kernels.hip -- the sums of sicp_pose_covariance (gfx950, wave64).
//
// Censi's estimate needs, per slot i of the current correspondences, the derivatives of the slot's gradient share
// g_i = rho'(r^2) r J with respect to its source point p and its target point q (6x3 each, everything else held fixed):
//     B^z = kappa J (dr/dz) + rho'(s) r dJ/dz,   s = r^2,   kappa = d(rho'(s) r) / dr = rho' + 2 s rho''
// summed per POINT: G_j = sum of B^p over source point j's slots, G_k = sum of B^q over the slots that hit target k, and
// S = sum G G^T over each cloud (include/sicp.h gives the formulas).
//
//   pose_cov_src_jobs       one lane per source point: its K slots (contiguous) -> G_j in registers, G_j G_j^T into a
//                           fixed-order column of partials; every active slot's B^q stored once (144 bytes) with its sort
//                           key job | target | slot
//   (ONE radix sort of the keys of all jobs, over the bits in use: every target's slots become one run, in slot
//   order, inside the job's own range of the array)
//   pose_cov_tile_jobs      one lane per tile of kPoseCovTile sorted slots: a run that lies inside the tile is summed and
//                           squared at once; a run that crosses a tile edge leaves its part as a piece
//   pose_cov_owner_jobs     one lane per tile whose last run starts a crossing list: adds the following tiles' pieces in
//                           tile order, then squares
//   pose_cov_finalize_jobs  the columns in a fixed order, one workgroup per output
// Every kernel is launched once for a whole group of pairs (kernels.h: PoseCovJob; a lone call is a group of one).  A job
// owns whole workgroups, and inside them everything is indexed from the job's own origin: its columns, tiles, pieces and
// flags are those of a launch of its own.  Every sum therefore has one fixed order that depends on the pair alone -- the
// butterfly per wave, the four waves in order, the job's columns in order -- and there are no float atomics: a pair gives
// the same bits alone, in any group and run after run.  A long target list costs its owner lane one 144-byte read per tile it spans instead of one
// per slot (the split rule of store-and-sum reductions with skewed destination counts).  Nothing here is GEMM shaped.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SICP_HD __host__ __device__
#include "job_table.hpp"
#include "kernels.h"

namespace sicp {
namespace {

constexpr double kDblEps = 2.220446049250313e-16;  // std::numeric_limits<double>::epsilon() (the SQLoss offset)

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 cross(const V3& a, const V3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// B^p and B^q of one slot, row-major 6x3.  A = C_t + R C_s R^T = 2 I - k (n n^T + m m^T) (k = 1 - eps, n = n_t, m = R n_s);
// its inverse M in the Woodbury form of corr_eval_src (solve_kernels.hip), formed explicitly here.
__device__ __forceinline__ void slot_derivatives(const Pose& P, double k, double gw, bool sqloss, double loss_b, double w, const V3& p,
                                                 const V3& ns, const V3& m, const V3& qs, const V3& q, const V3& nt, double (&Bp)[18],
                                                 double (&Bq)[18]) {
  const double* R = P.R;
  const V3 d{q.x - qs.x, q.y - qs.y, q.z - qs.z};
  const double dn = dot(nt, m);
  const double h = 1.0 / ((gw - dn) * (gw + dn));
  const double nv[3] = {nt.x, nt.y, nt.z}, mv[3] = {m.x, m.y, m.z};
  double M[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      M[a][b] = 0.5 * ((a == b ? 1.0 : 0.0) + h * (gw * (nv[a] * nv[b] + mv[a] * mv[b]) + dn * (nv[a] * mv[b] + mv[a] * nv[b])));
  const double dv[3] = {d.x, d.y, d.z};
  double a2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) a2[a] = 2.0 * (M[a][0] * dv[0] + M[a][1] * dv[1] + M[a][2] * dv[2]);
  const double r = 0.5 * (dv[0] * a2[0] + dv[1] * a2[1] + dv[2] * a2[2]);
  // b2 = R^T a2, c = p + 1/2 C_s b2, J = [-b2; b2 x c]
  const V3 b2{R[0] * a2[0] + R[3] * a2[1] + R[6] * a2[2], R[1] * a2[0] + R[4] * a2[1] + R[7] * a2[2], R[2] * a2[0] + R[5] * a2[1] + R[8] * a2[2]};
  const double nb = k * dot(ns, b2);
  const V3 c{p.x + 0.5 * (b2.x - nb * ns.x), p.y + 0.5 * (b2.y - nb * ns.y), p.z + 0.5 * (b2.z - nb * ns.z)};
  const V3 bc = cross(b2, c);
  const double J[6] = {-b2.x, -b2.y, -b2.z, bc.x, bc.y, bc.z};
  // rho'(s) and kappa in closed form (the SQLoss stacks: rho = w b log(1 + u / b), u = sqrt(s + eps); rho' and 2 s rho''
  // are both ~ 1 / (2 u) and would cancel)
  const double s = r * r;
  double rho1, kappa;
  if (sqloss) {
    const double u = sqrt(s + kDblEps), sum = 1.0 + u / loss_b;
    rho1 = w / (2.0 * u * sum);
    kappa = w * kDblEps / (2.0 * u * u * u * sum) - w * s / (2.0 * loss_b * u * u * sum * sum);
  } else {  // Cauchy: rho = b log(1 + s / b), the weight only carries the gate
    const double sum = 1.0 + s / loss_b;
    rho1 = w / sum;
    kappa = w * (1.0 - s / loss_b) / (sum * sum);
  }
  const double f = rho1 * r;
  // D = d b2 / d q = 2 R^T M;  d b2 / d p = -D R
  double D[3][3], DR[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) D[a][b] = 2.0 * (R[a] * M[0][b] + R[3 + a] * M[1][b] + R[6 + a] * M[2][b]);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) DR[a][b] = D[a][0] * R[b] + D[a][1] * R[3 + b] + D[a][2] * R[6 + b];
  // d c / d q = 1/2 C_s D,  d c / d p = I - 1/2 C_s D R,  C_s x = x - k (n_s . x) n_s
  const double nsv[3] = {ns.x, ns.y, ns.z};
#pragma unroll
  for (int col = 0; col < 3; ++col) {
    const V3 Dc{D[0][col], D[1][col], D[2][col]};
    const V3 DRc{DR[0][col], DR[1][col], DR[2][col]};
    const double kd = k * dot(ns, Dc), kdr = k * dot(ns, DRc);
    const V3 Eq{0.5 * (Dc.x - kd * nsv[0]), 0.5 * (Dc.y - kd * nsv[1]), 0.5 * (Dc.z - kd * nsv[2])};
    const V3 Ep{(col == 0 ? 1.0 : 0.0) - 0.5 * (DRc.x - kdr * nsv[0]), (col == 1 ? 1.0 : 0.0) - 0.5 * (DRc.y - kdr * nsv[1]),
                (col == 2 ? 1.0 : 0.0) - 0.5 * (DRc.z - kdr * nsv[2])};
    // dJ/dz = [-d b2/dz; [b2]x dc/dz - [c]x d b2/dz]
    const V3 xq1 = cross(b2, Eq), xq2 = cross(c, Dc);
    const V3 xp1 = cross(b2, Ep), xp2 = cross(c, DRc);
    const double dJq[6] = {-Dc.x, -Dc.y, -Dc.z, xq1.x - xq2.x, xq1.y - xq2.y, xq1.z - xq2.z};
    const double dJp[6] = {DRc.x, DRc.y, DRc.z, xp1.x + xp2.x, xp1.y + xp2.y, xp1.z + xp2.z};
    const double drq = a2[col], drp = -(col == 0 ? b2.x : (col == 1 ? b2.y : b2.z));
#pragma unroll
    for (int row = 0; row < 6; ++row) {
      Bq[3 * row + col] = kappa * J[row] * drq + f * dJq[row];
      Bp[3 * row + col] = kappa * J[row] * drp + f * dJp[row];
    }
  }
}

// the 21 upper-triangle entries of G G^T (G 6x3 row-major), in sicp_accumulate's order
__device__ __forceinline__ void add_outer(const double (&G)[18], double (&acc)[21]) {
  int o = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b, ++o) acc[o] += (G[3 * a] * G[3 * b] + G[3 * a + 1] * G[3 * b + 1]) + G[3 * a + 2] * G[3 * b + 2];
}

// 21 sums of a 256-lane workgroup into column `col` of part[21][cols]: a fixed butterfly per wave, the four waves in order
template <class PartPtr>
__device__ __forceinline__ void block_sum21(double (&acc)[21], PartPtr part, int cols, int col) {
  __shared__ double s_w[4][21];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 21; ++e) {
    double v = acc[e];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) s_w[wave][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < 21) part[(size_t)threadIdx.x * cols + col] = (s_w[0][threadIdx.x] + s_w[1][threadIdx.x]) + (s_w[2][threadIdx.x] + s_w[3][threadIdx.x]);
}

// A pointer read from a job record is a generic pointer to the compiler (flat loads and stores: 41 instead of 29 us for the
// tile kernel of a 100K-point pair); the records only ever hold device memory, and saying so gives global ones.
#if defined(__HIP_DEVICE_COMPILE__)
#define SICP_GLOBAL __attribute__((address_space(1)))
#else
#define SICP_GLOBAL  // (the host pass only parses the kernels)
#endif
template <class T>
__device__ __forceinline__ SICP_GLOBAL T* dev(T* p) {
  return (SICP_GLOBAL T*)p;
}

__global__ __launch_bounds__(256) void pose_cov_src_jobs_kernel(const PoseCovJob* __restrict__ jobs, const int* __restrict__ blk_end, int nj) {
  int lb;
  const PoseCovJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &lb)];
  const PoseCovArgs& a = J.a;
  const int n_s = a.n_s, K = a.K;
  const int i = lb * 256 + threadIdx.x;
  const int cols = pose_cov_blocks(n_s);
  double acc[21];
#pragma unroll
  for (int e = 0; e < 21; ++e) acc[e] = 0.0;
  int active = 0;
  if (i < n_s) {
    const Pose P = a.pose;
    const double* R = P.R;
    const double k = a.one_m_eps, gw = 2.0 / k - 1.0, loss_b = a.cauchy_a * a.cauchy_a;
    const bool sqloss = a.use_sqloss != 0;
    const auto idx = dev(a.idx);
    const auto wgt = dev(a.w);
    const auto trec = dev(a.trec);
    const auto keys = dev(a.key);
    const auto bq = dev(a.bq);
    const unsigned long long job_key = J.job_key, gated = job_key | ((unsigned long long)(unsigned)J.n_t << J.slot_bits);
    const int slot_bits = J.slot_bits;
    const PointRec sr = dev(a.srec)[i];
    const V3 p{(double)sr.x, (double)sr.y, (double)sr.z}, ns{sr.nx, sr.ny, sr.nz};
    const V3 m{R[0] * ns.x + R[1] * ns.y + R[2] * ns.z, R[3] * ns.x + R[4] * ns.y + R[5] * ns.z, R[6] * ns.x + R[7] * ns.y + R[8] * ns.z};
    const V3 qs{R[0] * p.x + R[1] * p.y + R[2] * p.z + P.t[0], R[3] * p.x + R[4] * p.y + R[5] * p.z + P.t[1],
                R[6] * p.x + R[7] * p.y + R[8] * p.z + P.t[2]};
    double G[18];
#pragma unroll
    for (int e = 0; e < 18; ++e) G[e] = 0.0;
    for (int c = 0; c < K; ++c) {
      const int s = i * K + c;
      const int j = idx[s];
      if (j < 0) {
        keys[s] = gated | (unsigned)s;
        continue;
      }
      ++active;
      keys[s] = job_key | ((unsigned long long)(unsigned)j << slot_bits) | (unsigned)s;
      const PointRec tr = trec[j];
      const V3 q{(double)tr.x, (double)tr.y, (double)tr.z}, nt{tr.nx, tr.ny, tr.nz};
      double Bp[18], Bq[18];
      slot_derivatives(P, k, gw, sqloss, loss_b, wgt ? wgt[s] : 1.0, p, ns, m, qs, q, nt, Bp, Bq);
#pragma unroll
      for (int e = 0; e < 18; ++e) G[e] += Bp[e];
      SICP_GLOBAL double2* o = (SICP_GLOBAL double2*)(bq + (size_t)s * 18);
#pragma unroll
      for (int e = 0; e < 9; ++e) o[e] = make_double2(Bq[2 * e], Bq[2 * e + 1]);
    }
    add_outer(G, acc);
  }
  __shared__ int s_act[4];
  int v = active;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) s_act[threadIdx.x >> 6] = v;
  block_sum21(acc, dev(a.part_src), cols, lb);  // (its barrier also orders s_act)
  if (threadIdx.x == 0) dev(a.part_active)[lb] = (long long)s_act[0] + s_act[1] + s_act[2] + s_act[3];
}

// flag bits of a tile: its first run continues the previous tile's list (piece 0), its last run starts a list that goes on
// into the next tile (piece 1: the tile owns that list), its only run comes from the previous tile AND goes on (pass-through)
constexpr int kFirstContinues = 1, kOwnsLast = 2, kPassThrough = 4;

__global__ __launch_bounds__(256) void pose_cov_tile_jobs_kernel(const PoseCovJob* __restrict__ jobs, const int* __restrict__ blk_end, int nj) {
  int lb;
  const PoseCovJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &lb)];
  const int total = J.a.n_s * J.a.K;
  const int t = lb * 256 + threadIdx.x;
  const int tiles = pose_cov_tiles(total), cols = 2 * pose_cov_blocks(tiles);
  double acc[21];
#pragma unroll
  for (int e = 0; e < 21; ++e) acc[e] = 0.0;
  if (t < tiles) {
    const auto skey = dev(J.skey);
    const auto bq = dev(J.a.bq);
    const auto piece = dev(J.piece);
    const int slot_bits = J.slot_bits;
    const unsigned long long slot_mask = (1ull << slot_bits) - 1ull, tgt_mask = (1ull << J.tgt_bits) - 1ull;
    const long long n_t = J.n_t;
    // target of a sorted key; -1 for a gated-out slot (those sort last within the job)
    auto key_target = [&](unsigned long long key) {
      const long long tg = (long long)((key >> slot_bits) & tgt_mask);
      return tg == n_t ? -1ll : tg;
    };
    const int b = t * kPoseCovTile, e = min(b + kPoseCovTile, total);
    const long long prev = b > 0 ? key_target(skey[b - 1]) : -2;
    const long long next = e < total ? key_target(skey[e]) : -2;
    int flag = 0;
    double sum[18];
#pragma unroll
    for (int x = 0; x < 18; ++x) sum[x] = 0.0;
    long long cur = -1;
    int start = b;
    auto finish = [&](int end) {
      const bool cin = start == b && cur == prev, cout = end == e && cur == next;
      if (!cin && !cout) {
        add_outer(sum, acc);
      } else {
        SICP_GLOBAL double2* o = (SICP_GLOBAL double2*)(piece + ((size_t)t * 2 + (cin ? 0 : 1)) * 18);
#pragma unroll
        for (int x = 0; x < 9; ++x) o[x] = make_double2(sum[2 * x], sum[2 * x + 1]);
        flag |= cin ? (kFirstContinues | (cout ? kPassThrough : 0)) : kOwnsLast;
      }
    };
    int pos = b;
    for (; pos < e; ++pos) {
      const unsigned long long key = skey[pos];
      const long long tg = key_target(key);
      if (tg < 0) break;
      if (tg != cur) {
        if (cur >= 0) finish(pos);
        cur = tg;
        start = pos;
#pragma unroll
        for (int x = 0; x < 18; ++x) sum[x] = 0.0;
      }
      const SICP_GLOBAL double2* r = (const SICP_GLOBAL double2*)(bq + (size_t)(key & slot_mask) * 18);
#pragma unroll
      for (int x = 0; x < 9; ++x) {
        const double2 v = r[x];
        sum[2 * x] += v.x;
        sum[2 * x + 1] += v.y;
      }
    }
    if (cur >= 0) finish(pos);
    dev(J.flag)[t] = flag;
  }
  block_sum21(acc, dev(J.part_tgt), cols, lb);
}

__global__ __launch_bounds__(256) void pose_cov_owner_jobs_kernel(const PoseCovJob* __restrict__ jobs, const int* __restrict__ blk_end, int nj) {
  int lb;
  const PoseCovJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &lb)];
  const int t = lb * 256 + threadIdx.x;
  const int tiles = pose_cov_tiles(J.a.n_s * J.a.K), tb = pose_cov_blocks(tiles), cols = 2 * tb;
  double acc[21];
#pragma unroll
  for (int e = 0; e < 21; ++e) acc[e] = 0.0;
  const auto flags = dev(J.flag);
  if (t < tiles && (flags[t] & kOwnsLast)) {
    const auto pieces = dev(J.piece);
    double sum[18];
    const auto p = pieces + ((size_t)t * 2 + 1) * 18;
#pragma unroll
    for (int x = 0; x < 18; ++x) sum[x] = p[x];
    for (int u = t + 1; u < tiles; ++u) {
      const int f = flags[u];
      if (!(f & kFirstContinues)) break;  // (cannot happen: the owner's list goes on into tile t + 1)
      const auto q = pieces + (size_t)u * 2 * 18;
#pragma unroll
      for (int x = 0; x < 18; ++x) sum[x] += q[x];
      if (!(f & kPassThrough)) break;
    }
    add_outer(sum, acc);
  }
  block_sum21(acc, dev(J.part_tgt), cols, tb + lb);
}

// 43 workgroups per job, one per output: rows 0..20 S_src, 21..41 S_tgt, 42 the active count.  Every lane sums the job's
// columns c = lane, lane + 256, ... in order, then the fixed butterfly and the four waves in order (a lane walking a whole
// row alone took 150 us at 100K points: one dependent load per column).
__global__ __launch_bounds__(256) void pose_cov_finalize_jobs_kernel(const PoseCovJob* __restrict__ jobs) {
  __shared__ double s_w[4];
  __shared__ long long s_a[4];
  const PoseCovJob& J = jobs[blockIdx.x / 43];
  const int e = blockIdx.x % 43, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int src_cols = pose_cov_blocks(J.a.n_s), tgt_cols = 2 * pose_cov_blocks(pose_cov_tiles(J.a.n_s * J.a.K));
  if (e < 42) {
    const int cols = e < 21 ? src_cols : tgt_cols;
    const SICP_GLOBAL double* row = e < 21 ? dev(J.a.part_src) + (size_t)e * src_cols : dev(J.part_tgt) + (size_t)(e - 21) * tgt_cols;
    double v = 0.0;
    for (int c = threadIdx.x; c < cols; c += 256) v += row[c];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) s_w[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) dev(J.out42)[e] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
  } else {
    const auto part_active = dev(J.a.part_active);
    long long v = 0;
    for (int c = threadIdx.x; c < src_cols; c += 256) v += part_active[c];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) s_a[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) *dev(J.active) = (s_a[0] + s_a[1]) + (s_a[2] + s_a[3]);
  }
}

}  // namespace

hipError_t launch_pose_cov_src_jobs(const PoseCovJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st) {
  if (nj <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(pose_cov_src_jobs_kernel, dim3(blocks), dim3(256), 0, st, jobs, blk_end, nj);
  return hipGetLastError();
}

hipError_t launch_pose_cov_tile_jobs(const PoseCovJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st) {
  if (nj <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(pose_cov_tile_jobs_kernel, dim3(blocks), dim3(256), 0, st, jobs, blk_end, nj);
  return hipGetLastError();
}

hipError_t launch_pose_cov_owner_jobs(const PoseCovJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st) {
  if (nj <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(pose_cov_owner_jobs_kernel, dim3(blocks), dim3(256), 0, st, jobs, blk_end, nj);
  return hipGetLastError();
}

hipError_t launch_pose_cov_finalize_jobs(const PoseCovJob* jobs, int nj, hipStream_t st) {
  if (nj <= 0) return hipSuccess;
  hipLaunchKernelGGL(pose_cov_finalize_jobs_kernel, dim3(43 * nj), dim3(256), 0, st, jobs);
  return hipGetLastError();
}

}  // namespace sicp
