// graph_kernels.hip -- sicp_graph_*: the pose graph's kernels (driver: graph.cpp; an edge's algebra: graph_edge.hpp; the rules:
// include/sicp.h and INTEGRATION.md, "Pose graph").
//   linearise   one edge per lane, 64 lanes a workgroup: residual, chi2, weight, the two (diagonal block, gradient) records and
//               the off-diagonal block; the cost-only form stops after the loss
//   prior       one prior per lane, 64 lanes a workgroup, both kinds in one launch: residual, chi2, weight and the prior's one
//               (diagonal block, gradient) record; the cost-only form stops after the loss
//   gather      one lane per (node, entry of the 42-entry record): the sum of the node's edge records in incidence order, then
//               of its prior records in prior order
//   CG          A = H + D on the free nodes, block-Jacobi preconditioner (6x6 Cholesky per node).  The SpMV takes one lane per
//               (node, row) and walks the node's incidence list; dots are per-workgroup partial sums that one workgroup adds;
//               alpha, beta and the norms live in GraphScalars and every kernel returns when its flag is set
//   candidates  T exp(delta) per node, and the sums of the step's acceptance test
// Plain launches on one stream; no float atomics and no grid-wide synchronisation.
#include <hip/hip_runtime.h>

#define SICP_HD __host__ __device__
#include "graph_prior.hpp"
#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

// the sum (or the maximum) of the 256 lanes' values, in one fixed order, in every lane
template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) sh[t] = MAX ? fmax(sh[t], sh[t + h]) : sh[t] + sh[t + h];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void graph_keys_kernel(GraphArgs a, u64* __restrict__ keys) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2ll * a.n_edges) return;
  const int e = (int)(t >> 1);
  if (a.een && !a.een[e]) {  // a disabled edge: behind every node's list, in no node's degree
    keys[t] = ((u64)(unsigned)a.n_nodes << 32) | (u64)(unsigned)t;
    return;
  }
  const int node = (t & 1) ? a.ej[e] : a.ei[e];
  keys[t] = ((u64)(unsigned)node << 32) | (u64)(unsigned)t;
  atomicAdd(&a.deg[node], 1);
}

template <bool FULL>
__global__ __launch_bounds__(kGraphLinLanes) void graph_linearise_kernel(GraphArgs a, const double* __restrict__ pose) {
  const long long e = (long long)blockIdx.x * kGraphLinLanes + threadIdx.x;
  if (e >= a.n_edges) return;
  double Ti[7], Tj[7], z[7], Om[36];
  const double* pi = pose + 7ll * a.ei[e];
  const double* pj = pose + 7ll * a.ej[e];
  SICP_UNROLL
  for (int k = 0; k < 7; ++k) { Ti[k] = pi[k]; Tj[k] = pj[k]; z[k] = a.z[7 * e + k]; }
  SICP_UNROLL
  for (int k = 0; k < 36; ++k) Om[k] = a.omega[36 * e + k];
  double r[6], Or[6], Tji[7], s, w, rho;
  graph::edge_error(Ti, Tj, z, Om, a.loss, a.cauchy_a, r, Or, &s, &w, &rho, Tji);
  a.ec[e] = (a.een && !a.een[e]) ? 0.0 : 0.5 * rho;
  if (!FULL) return;
  a.s[e] = s;
  a.w[e] = w;
  SICP_UNROLL
  for (int k = 0; k < 6; ++k) a.r[6 * e + k] = r[k];
  graph::edge_blocks(r, Or, Om, w, Tji, a.C + (2 * e) * kGraphRec, a.C + (2 * e + 1) * kGraphRec, a.B + 36 * e);
}

// One prior per lane.  A pose prior holds two 6x6 arrays beside Omega (an edge: five), a position prior two 3x3.
template <bool FULL>
__global__ __launch_bounds__(kGraphLinLanes) void graph_prior_linearise_kernel(GraphArgs a, const double* __restrict__ pose) {
  const long long p = (long long)blockIdx.x * kGraphLinLanes + threadIdx.x;
  if (p >= a.n_priors) return;
  double T[7], r[6], s, w, rho;
  const double* pk = pose + 7ll * a.pnode[p];
  SICP_UNROLL
  for (int k = 0; k < 7; ++k) T[k] = pk[k];
  double* ec = a.ec + a.n_edges;
  const bool on = a.pen[p] != 0;
  if (a.pkind[p] == graph::kPriorPosition) {
    double pt[3], Om[9], Or[3];
    SICP_UNROLL
    for (int k = 0; k < 3; ++k) pt[k] = a.pz[7 * p + k];
    SICP_UNROLL
    for (int k = 0; k < 9; ++k) Om[k] = a.pomega[36 * p + k];
    graph::prior_position_error(T, pt, Om, a.loss, a.cauchy_a, r, Or, &s, &w, &rho);
    ec[p] = on ? 0.5 * rho : 0.0;
    if (!FULL) return;
    graph::prior_position_blocks(T, Or, Om, w, a.PC + p * kGraphRec);
  } else {
    double z[7], Om[36], Or[6];
    SICP_UNROLL
    for (int k = 0; k < 7; ++k) z[k] = a.pz[7 * p + k];
    SICP_UNROLL
    for (int k = 0; k < 36; ++k) Om[k] = a.pomega[36 * p + k];
    graph::prior_pose_error(T, z, Om, a.loss, a.cauchy_a, r, Or, &s, &w, &rho);
    ec[p] = on ? 0.5 * rho : 0.0;
    if (!FULL) return;
    graph::prior_pose_blocks(r, Or, Om, w, a.PC + p * kGraphRec);
  }
  a.ps[p] = s;
  a.pw[p] = w;
  SICP_UNROLL
  for (int k = 0; k < 6; ++k) a.pr[6 * p + k] = r[k];
}

__global__ __launch_bounds__(256) void graph_gather_kernel(GraphArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)a.n_nodes * kGraphRec) return;
  const int n = (int)(t / kGraphRec), k = (int)(t % kGraphRec);
  double v = 0;
  if (a.fixed[n]) {
    v = (k < 36 && k / 6 == k % 6) ? 1.0 : 0.0;
  } else {
    const int end = a.off[n + 1];
    for (int q = a.off[n]; q < end; ++q) v += a.C[(long long)(unsigned)a.inc[q] * kGraphRec + k];
    if (a.n_priors > 0) {
      const int pend = a.poff[n + 1];
      for (int q = a.poff[n]; q < pend; ++q) v += a.PC[(long long)a.pinc[q] * kGraphRec + k];
    }
  }
  if (k < 36) a.H[36ll * n + k] = v; else a.g[6ll * n + (k - 36)] = v;
}

// partial sums of ec (MAX = false) or partial maxima of |g| (MAX = true) into column 0
template <bool MAX>
__global__ __launch_bounds__(256) void graph_sum_kernel(GraphArgs a, const double* __restrict__ v, long long n) {
  __shared__ double sh[256];
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  double x = 0;
  if (t < n) x = MAX ? fabs(v[t]) : v[t];
  if (MAX && !(x == x)) x = __builtin_huge_val();  // (a NaN gradient must not pass for a small one)
  const double s = block_reduce<MAX>(x, sh);
  if (threadIdx.x == 0) a.part[blockIdx.x] = s;
}

__device__ __forceinline__ double damping(const GraphArgs& a, int n, int k) {
  return fmin(fmax(a.H[36ll * n + 7 * k], a.lo), a.hi) / a.radius;
}

// z = (L L^T)^-1 r with the node's packed factor
__device__ __forceinline__ void chol_apply(const double* __restrict__ L, const double* r, double* z) {
  double y[6];
  SICP_UNROLL
  for (int i = 0; i < 6; ++i) {
    double s = r[i];
    SICP_UNROLL
    for (int k = 0; k < i; ++k) s -= L[i * (i + 1) / 2 + k] * y[k];
    y[i] = s * L[21 + i];
  }
  SICP_UNROLL
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    SICP_UNROLL
    for (int k = i + 1; k < 6; ++k) s -= L[k * (k + 1) / 2 + i] * z[k];
    z[i] = s * L[21 + i];
  }
}

// one lane per node: the factor of the damped diagonal block; x = 0, r = -g, z = M^-1 r, p = z; partials of r.z and r.r
__global__ __launch_bounds__(256) void graph_cg_begin_kernel(GraphArgs a) {
  __shared__ double sh[256];
  const int n = blockIdx.x * 256 + threadIdx.x;
  double rz = 0, rr = 0;
  if (n < a.n_nodes) {
    double A[kGraphChol];  // the factor's 21 entries, then the reciprocals of its diagonal
    double* inv = A + 21;
    bool ok = true;
    SICP_UNROLL
    for (int i = 0; i < 6; ++i)
      SICP_UNROLL
      for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] = a.H[36ll * n + 6 * i + j] + (i == j ? damping(a, n, i) : 0.0);
    SICP_UNROLL
    for (int i = 0; i < 6; ++i)
      SICP_UNROLL
      for (int j = 0; j <= i; ++j) {
        double s = A[i * (i + 1) / 2 + j];
        SICP_UNROLL
        for (int k = 0; k < j; ++k) s -= A[i * (i + 1) / 2 + k] * A[j * (j + 1) / 2 + k];
        if (i == j) {
          if (!(s > 0)) { ok = false; s = 1.0; }
          A[i * (i + 1) / 2 + i] = sqrt(s);
          inv[i] = 1.0 / A[i * (i + 1) / 2 + i];
        } else {
          A[i * (i + 1) / 2 + j] = s * inv[j];
        }
      }
    if (!ok) a.S->flag = kGraphBreakdown;
    double* L = a.L + (long long)kGraphChol * n;
    SICP_UNROLL
    for (int k = 0; k < kGraphChol; ++k) L[k] = A[k];
    double r[6], z[6];
    SICP_UNROLL
    for (int k = 0; k < 6; ++k) r[k] = -a.g[6ll * n + k];
    chol_apply(A, r, z);
    SICP_UNROLL
    for (int k = 0; k < 6; ++k) {
      a.x[6ll * n + k] = 0;
      a.rr[6ll * n + k] = r[k];
      a.zz[6ll * n + k] = z[k];
      a.p[6ll * n + k] = z[k];
      rz += r[k] * z[k];
      rr += r[k] * r[k];
    }
  }
  const double s0 = block_reduce<false>(rz, sh);
  const double s1 = block_reduce<false>(rr, sh);
  if (threadIdx.x == 0) { a.part[blockIdx.x] = s0; a.part[a.part_stride + blockIdx.x] = s1; }
}

// q = A v, one lane per (node, row); partials of v.q.  DAMPED: A = H + D (conjugate gradients); otherwise A = H (the model's
// decrease).  CG: returns when the flag is set.
template <bool DAMPED>
__global__ __launch_bounds__(256) void graph_spmv_kernel(GraphArgs a, const double* __restrict__ v, double* __restrict__ q) {
  __shared__ double sh[256];
  if (DAMPED && a.S->flag) return;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  double dot = 0;
  if (t < 6ll * a.n_nodes) {
    const int n = (int)(t / 6), row = (int)(t % 6);
    const double* vn = v + 6ll * n;
    const double* Hn = a.H + 36ll * n + 6 * row;
    double y = 0;
    SICP_UNROLL
    for (int b = 0; b < 6; ++b) y += Hn[b] * vn[b];
    if (DAMPED) y += damping(a, n, row) * vn[row];
    if (!a.fixed[n]) {
      const int end = a.off[n + 1];
      for (int k = a.off[n]; k < end; ++k) {
        const unsigned slot = (unsigned)a.inc[k];
        const unsigned e = slot >> 1;
        const int other = (slot & 1) ? a.ei[e] : a.ej[e];
        if (a.fixed[other]) continue;
        const double* B = a.B + 36ll * e;
        const double* vo = v + 6ll * other;
        double s = 0;
        if (slot & 1) {
          SICP_UNROLL
          for (int b = 0; b < 6; ++b) s += B[6 * b + row] * vo[b];  // B^T x_i
        } else {
          SICP_UNROLL
          for (int b = 0; b < 6; ++b) s += B[6 * row + b] * vo[b];  // B x_j
        }
        y += s;
      }
    }
    q[t] = y;
    dot = v[t] * y;
  }
  const double s = block_reduce<false>(dot, sh);
  if (threadIdx.x == 0) a.part[blockIdx.x] = s;
}

// one lane per node: x += alpha p, r -= alpha q, z = M^-1 r; partials of r.z and r.r
__global__ __launch_bounds__(256) void graph_cg_update_kernel(GraphArgs a) {
  __shared__ double sh[256];
  if (a.S->flag) return;
  const double alpha = a.S->alpha;
  const int n = blockIdx.x * 256 + threadIdx.x;
  double rz = 0, rr = 0;
  if (n < a.n_nodes) {
    double r[6], z[6], L[kGraphChol];
    SICP_UNROLL
    for (int k = 0; k < kGraphChol; ++k) L[k] = a.L[(long long)kGraphChol * n + k];
    SICP_UNROLL
    for (int k = 0; k < 6; ++k) {
      a.x[6ll * n + k] += alpha * a.p[6ll * n + k];
      r[k] = a.rr[6ll * n + k] - alpha * a.q[6ll * n + k];
      a.rr[6ll * n + k] = r[k];
    }
    chol_apply(L, r, z);
    SICP_UNROLL
    for (int k = 0; k < 6; ++k) {
      a.zz[6ll * n + k] = z[k];
      rz += r[k] * z[k];
      rr += r[k] * r[k];
    }
  }
  const double s0 = block_reduce<false>(rz, sh);
  const double s1 = block_reduce<false>(rr, sh);
  if (threadIdx.x == 0) { a.part[blockIdx.x] = s0; a.part[a.part_stride + blockIdx.x] = s1; }
}

__global__ __launch_bounds__(256) void graph_cg_direction_kernel(GraphArgs a) {
  if (a.S->flag) return;
  const double beta = a.S->beta;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < 6ll * a.n_nodes) a.p[t] = a.zz[t] + beta * a.p[t];
}

// one lane per node: the candidate pose, and partials of |poses|^2, |delta|^2 and g.delta.  A fixed node and a node whose step
// is zero keep their bytes.
__global__ __launch_bounds__(256) void graph_candidates_kernel(GraphArgs a) {
  __shared__ double sh[256];
  const int n = blockIdx.x * 256 + threadIdx.x;
  double p2 = 0, xx = 0, gx = 0;
  if (n < a.n_nodes) {
    double T[7], d[6], o[7];
    bool zero = true;
    SICP_UNROLL
    for (int k = 0; k < 7; ++k) { T[k] = a.pose[7ll * n + k]; p2 += T[k] * T[k]; }
    SICP_UNROLL
    for (int k = 0; k < 6; ++k) {
      d[k] = a.x[6ll * n + k];
      zero = zero && d[k] == 0.0;
      xx += d[k] * d[k];
      gx += a.g[6ll * n + k] * d[k];
    }
    if (a.fixed[n] || zero) {
      SICP_UNROLL
      for (int k = 0; k < 7; ++k) o[k] = T[k];
    } else {
      se3::plus(T, d, o);
    }
    SICP_UNROLL
    for (int k = 0; k < 7; ++k) a.cand[7ll * n + k] = o[k];
  }
  const double s0 = block_reduce<false>(p2, sh);
  const double s1 = block_reduce<false>(xx, sh);
  const double s2 = block_reduce<false>(gx, sh);
  if (threadIdx.x == 0) {
    a.part[blockIdx.x] = s0;
    a.part[a.part_stride + blockIdx.x] = s1;
    a.part[2 * a.part_stride + blockIdx.x] = s2;
  }
}

// One workgroup: every column's `count` partials added in index order (lane t takes a run of consecutive ones, the runs are
// added in lane order), then lane 0 takes the step of the scalars.
__device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }
template <int FIN>
__global__ __launch_bounds__(256) void graph_finish_kernel(GraphArgs a, int count) {
  __shared__ double sh[256];
  GraphScalars* S = a.S;
  constexpr bool CG = FIN == kGraphFinStart || FIN == kGraphFinPq || FIN == kGraphFinRz;
  if (CG && S->flag) return;
  constexpr int COLS = FIN == kGraphFinCand ? 3 : (FIN == kGraphFinStart || FIN == kGraphFinRz) ? 2 : 1;
  constexpr bool MAX = FIN == kGraphFinGmax;
  const int run = (count + 255) / 256;
  double c[3] = {0, 0, 0};
  SICP_UNROLL
  for (int col = 0; col < COLS; ++col) {
    double v = 0;
    const int lo = threadIdx.x * run, hi = min(lo + run, count);
    for (int k = lo; k < hi; ++k) v = MAX ? fmax(v, a.part[col * a.part_stride + k]) : v + a.part[col * a.part_stride + k];
    c[col] = block_reduce<MAX>(v, sh);
  }
  if (threadIdx.x != 0) return;
  if (FIN == kGraphFinStart) {
    S->rz = c[0]; S->rr = c[1]; S->bb = c[1];
    if (!finite(c[0]) || !finite(c[1])) S->flag = kGraphBreakdown;
    else if (c[1] == 0.0) S->flag = kGraphConverged;
  } else if (FIN == kGraphFinPq) {
    S->pq = c[0];
    if (!finite(c[0]) || !(c[0] > 0.0)) S->flag = kGraphBreakdown;
    else S->alpha = S->rz / c[0];
  } else if (FIN == kGraphFinRz) {
    S->rr = c[1];
    if (!finite(c[0]) || !finite(c[1])) {
      S->flag = kGraphBreakdown;
    } else {
      S->beta = c[0] / S->rz;
      S->rz = c[0];
      S->cg_iters += 1;
      if (sqrt(c[1]) <= a.eta * sqrt(S->bb)) S->flag = kGraphConverged;
    }
  } else if (FIN == kGraphFinCost) {
    S->cost = c[0];
  } else if (FIN == kGraphFinCandCost) {
    S->cand_cost = c[0];
  } else if (FIN == kGraphFinGmax) {
    S->gmax = c[0];
  } else if (FIN == kGraphFinCand) {
    S->pose2 = c[0]; S->xx = c[1]; S->gx = c[2];
  } else {
    S->xHx = c[0];
  }
}

__global__ void graph_cg_reset_kernel(GraphArgs a) {
  a.S->flag = kGraphRunning;
  a.S->cg_iters = 0;
  a.S->alpha = 0; a.S->beta = 0; a.S->pq = 0;
}

}  // namespace

hipError_t launch_graph_keys(const GraphArgs& a, unsigned long long* keys, hipStream_t st) {
  graph_keys_kernel<<<graph_blocks(2ll * a.n_edges), 256, 0, st>>>(a, keys);
  return hipGetLastError();
}

hipError_t launch_graph_linearise(const GraphArgs& a, const double* pose, bool full, hipStream_t st) {
  const int blocks = (a.n_edges + kGraphLinLanes - 1) / kGraphLinLanes;
  if (full) graph_linearise_kernel<true><<<blocks, kGraphLinLanes, 0, st>>>(a, pose);
  else graph_linearise_kernel<false><<<blocks, kGraphLinLanes, 0, st>>>(a, pose);
  return hipGetLastError();
}

hipError_t launch_graph_prior_linearise(const GraphArgs& a, const double* pose, bool full, hipStream_t st) {
  const int blocks = (a.n_priors + kGraphLinLanes - 1) / kGraphLinLanes;
  if (full) graph_prior_linearise_kernel<true><<<blocks, kGraphLinLanes, 0, st>>>(a, pose);
  else graph_prior_linearise_kernel<false><<<blocks, kGraphLinLanes, 0, st>>>(a, pose);
  return hipGetLastError();
}

hipError_t launch_graph_gather(const GraphArgs& a, hipStream_t st) {
  graph_gather_kernel<<<graph_blocks((long long)a.n_nodes * kGraphRec), 256, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_graph_sum(const GraphArgs& a, int fin, hipStream_t st) {
  if (fin == kGraphFinGmax) {
    const int b = graph_blocks(6ll * a.n_nodes);
    graph_sum_kernel<true><<<b, 256, 0, st>>>(a, a.g, 6ll * a.n_nodes);
    graph_finish_kernel<kGraphFinGmax><<<1, 256, 0, st>>>(a, b);
  } else {
    const long long entries = (long long)a.n_edges + a.n_priors;  // the edges' 1/2 rho, then the priors'
    const int b = graph_blocks(entries);
    graph_sum_kernel<false><<<b, 256, 0, st>>>(a, a.ec, entries);
    if (fin == kGraphFinCost) graph_finish_kernel<kGraphFinCost><<<1, 256, 0, st>>>(a, b);
    else graph_finish_kernel<kGraphFinCandCost><<<1, 256, 0, st>>>(a, b);
  }
  return hipGetLastError();
}

hipError_t launch_graph_cg_begin(const GraphArgs& a, hipStream_t st) {
  const int b = graph_blocks(a.n_nodes);
  graph_cg_reset_kernel<<<1, 1, 0, st>>>(a);
  graph_cg_begin_kernel<<<b, 256, 0, st>>>(a);
  graph_finish_kernel<kGraphFinStart><<<1, 256, 0, st>>>(a, b);
  return hipGetLastError();
}

hipError_t launch_graph_cg_iteration(const GraphArgs& a, hipStream_t st) {
  const int bn = graph_blocks(a.n_nodes), br = graph_blocks(6ll * a.n_nodes);
  graph_spmv_kernel<true><<<br, 256, 0, st>>>(a, a.p, a.q);
  graph_finish_kernel<kGraphFinPq><<<1, 256, 0, st>>>(a, br);
  graph_cg_update_kernel<<<bn, 256, 0, st>>>(a);
  graph_finish_kernel<kGraphFinRz><<<1, 256, 0, st>>>(a, bn);
  graph_cg_direction_kernel<<<br, 256, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_graph_candidates(const GraphArgs& a, hipStream_t st) {
  const int bn = graph_blocks(a.n_nodes), br = graph_blocks(6ll * a.n_nodes);
  graph_candidates_kernel<<<bn, 256, 0, st>>>(a);
  graph_finish_kernel<kGraphFinCand><<<1, 256, 0, st>>>(a, bn);
  graph_spmv_kernel<false><<<br, 256, 0, st>>>(a, a.x, a.q);
  graph_finish_kernel<kGraphFinModel><<<1, 256, 0, st>>>(a, br);
  return hipGetLastError();
}

}  // namespace sicp
