// graph_cov_kernels.hip -- sicp_graph_marginals / sicp_graph_relative_covariances: blocks of H^-1 by conjugate gradients on many
// right-hand sides in lock step (driver: graph.cpp; the layout and the rules of independence: kernels.h; the meaning:
// include/sicp.h, "pose-graph covariances").
//   factor     one lane per node: the Cholesky factor of the undamped diagonal block (the identity for a free node without edges)
//   begin      one lane per (node, column) of a query: the sparse J^T, x = 0, r = b, z = M^-1 r, p = z; partials of r.z and r.r
//   SpMM       q = H p for COLS columns at once: one lane per (node, row) as graph_spmv_kernel, with the same incidence walk; the
//              lane loads its six entries of H and of each B_e once and applies them to COLS accumulators; partials of p.q
//   update     x += alpha p, r -= alpha q, z = M^-1 r per (node, column); partials of r.z and r.r
//   direction  p = z + beta p
//   finish     one workgroup per column: the column's partials in graph_finish_kernel's order, then the step of its scalars
//   extract    per query, sym(J X) from the rows of X at its two nodes
// Plain launches on one stream; no float atomics and no grid-wide synchronisation.  A column whose flag is set is frozen.
#include <hip/hip_runtime.h>

#define SICP_HD __host__ __device__
#include "graph_cov.hpp"
#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

constexpr int kCovLanes = 6 * kGraphCovNodes;  // the begin / update workgroup: 64 nodes x the 6 columns of one query
enum { kCovFinStart, kCovFinPq, kCovFinRz };

__device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }

// the sum of the 256 lanes' values in graph_kernels.hip's order, in every lane
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) sh[t] = sh[t] + sh[t + h];
    __syncthreads();
  }
  return sh[0];
}

// z = (L L^T)^-1 r with the node's packed factor
__device__ __forceinline__ void chol_apply(const double* L, const double* r, double* z) {
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

// a free node without enabled edges and without an enabled pose prior: the identity block.  (A node that only position
// priors hold has a block of rank 3; it is never asked for -- UNANCHORED -- and couples to nothing.)
__device__ __forceinline__ bool lone(const GraphCovArgs& a, int n) {
  return !a.fixed[n] && a.off[n + 1] == a.off[n] && !(a.held && a.held[n]);
}

__global__ __launch_bounds__(256) void graph_cov_factor_kernel(GraphCovArgs a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.n_nodes) return;
  double A[kGraphChol];
  double* inv = A + 21;
  const bool unit = lone(a, n);
  bool ok = true;
  SICP_UNROLL
  for (int i = 0; i < 6; ++i)
    SICP_UNROLL
    for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] = unit ? (i == j ? 1.0 : 0.0) : a.H[36ll * n + 6 * i + j];
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
  if (!ok) *a.bad = 1;
  double* L = a.L + (long long)kGraphChol * n;
  SICP_UNROLL
  for (int k = 0; k < kGraphChol; ++k) L[k] = A[k];
}

// The two partial sums of a begin / update workgroup: lane (node nl, column k) holds its terms; per column the 64 nodes' terms are
// added pairwise in one fixed order.
__device__ __forceinline__ void node_block_sums(const GraphCovArgs& a, double rz, double rr, double* sh0, double* sh1, int slot) {
  const int t = threadIdx.x, nl = t / 6, k = t % 6;
  sh0[k * kGraphCovNodes + nl] = rz;
  sh1[k * kGraphCovNodes + nl] = rr;
  __syncthreads();
  for (int h = kGraphCovNodes / 2; h > 0; h >>= 1) {
    if (t < 6 * h) {
      const int c = t / h, j = t % h;
      sh0[c * kGraphCovNodes + j] = sh0[c * kGraphCovNodes + j] + sh0[c * kGraphCovNodes + j + h];
      sh1[c * kGraphCovNodes + j] = sh1[c * kGraphCovNodes + j] + sh1[c * kGraphCovNodes + j + h];
    }
    __syncthreads();
  }
  if (t < 6) {
    const long long col = 6ll * slot + t;
    a.part[col * a.part_stride + blockIdx.x] = sh0[t * kGraphCovNodes];
    a.part[((long long)a.cols + col) * a.part_stride + blockIdx.x] = sh1[t * kGraphCovNodes];
  }
}

// grid: (blocks of 64 nodes, queries).  Column 6 slot + k of b = J^T is row k of J_a at node qa and e_k at node qb.
__global__ __launch_bounds__(kCovLanes) void graph_cov_begin_kernel(GraphCovArgs a) {
  __shared__ double sh0[kCovLanes], sh1[kCovLanes];
  const int slot = blockIdx.y, t = threadIdx.x, k = t % 6;
  const int n = blockIdx.x * kGraphCovNodes + t / 6;
  double rz = 0, rr = 0;
  if (n < a.n_nodes) {
    const int qa = a.qa[slot], qb = a.qb[slot];
    double r[6] = {0, 0, 0, 0, 0, 0}, z[6] = {0, 0, 0, 0, 0, 0};
    bool any = false;
    if (n == qb && !a.fixed[n]) { r[k] = 1.0; any = true; }
    if (n == qa && !a.fixed[n]) {
      double Ta[7], Tb[7], Ja[36];
      SICP_UNROLL
      for (int d = 0; d < 7; ++d) { Ta[d] = a.pose[7ll * qa + d]; Tb[d] = a.pose[7ll * qb + d]; }
      graph::relative_jacobian_a(Ta, Tb, Ja);
      SICP_UNROLL
      for (int d = 0; d < 6; ++d) {
        SICP_UNROLL
        for (int kk = 0; kk < 6; ++kk)
          if (kk == k) r[d] = Ja[6 * kk + d];
      }
      SICP_UNROLL
      for (int d = 0; d < 6; ++d) {
        SICP_UNROLL
        for (int kk = 0; kk < 6; ++kk)
          if (kk == k) a.J[36ll * slot + 6 * kk + d] = Ja[6 * kk + d];
      }
      any = true;
    }
    if (any) {
      double L[kGraphChol];
      SICP_UNROLL
      for (int d = 0; d < kGraphChol; ++d) L[d] = a.L[(long long)kGraphChol * n + d];
      chol_apply(L, r, z);
    }
    const long long at = ((long long)n * a.cols + 6ll * slot + k) * 6;
    SICP_UNROLL
    for (int d = 0; d < 6; ++d) {
      a.x[at + d] = 0;
      a.r[at + d] = r[d];
      a.z[at + d] = z[d];
      a.p[at + d] = z[d];
      rz += r[d] * z[d];
      rr += r[d] * r[d];
    }
  }
  node_block_sums(a, rz, rr, sh0, sh1, slot);
}

// grid: (blocks of 256 (node, row) lanes, cols / COLS).  q = H p on the columns c0 .. c0 + COLS; partials of p.q per column.
template <int COLS>
__global__ __launch_bounds__(256) void graph_spmm_kernel(GraphCovArgs a) {
  __shared__ double sh[COLS * 256];
  const int c0 = blockIdx.y * COLS;
  {
    bool running = false;
    for (int c = 0; c < COLS; ++c) running = running || a.S[c0 + c].flag == kGraphCovRunning;
    if (!running) return;
  }
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  double y[COLS];
  SICP_UNROLL
  for (int c = 0; c < COLS; ++c) y[c] = 0;
  if (t < 6ll * a.n_nodes) {
    const int n = (int)(t / 6), row = (int)(t % 6);
    const double* vn = a.p + ((long long)n * a.cols + c0) * 6;
    if (lone(a, n)) {
      SICP_UNROLL
      for (int c = 0; c < COLS; ++c) y[c] = vn[6 * c + row];
    } else {
      double m[6];
      SICP_UNROLL
      for (int b = 0; b < 6; ++b) m[b] = a.H[36ll * n + 6 * row + b];
      SICP_UNROLL
      for (int c = 0; c < COLS; ++c) {
        double s = 0;
        SICP_UNROLL
        for (int b = 0; b < 6; ++b) s += m[b] * vn[6 * c + b];
        y[c] = s;
      }
      if (!a.fixed[n]) {
        const int end = a.off[n + 1];
        for (int k = a.off[n]; k < end; ++k) {
          const unsigned slot = (unsigned)a.inc[k];
          const unsigned e = slot >> 1;
          const int other = (slot & 1) ? a.ei[e] : a.ej[e];
          if (a.fixed[other]) continue;
          const double* B = a.B + 36ll * e;
          SICP_UNROLL
          for (int b = 0; b < 6; ++b) m[b] = (slot & 1) ? B[6 * b + row] : B[6 * row + b];  // B^T x_i / B x_j
          const double* vo = a.p + ((long long)other * a.cols + c0) * 6;
          SICP_UNROLL
          for (int c = 0; c < COLS; ++c) {
            double s = 0;
            SICP_UNROLL
            for (int b = 0; b < 6; ++b) s += m[b] * vo[6 * c + b];
            y[c] += s;
          }
        }
      }
    }
    double* qn = a.q + ((long long)n * a.cols + c0) * 6;
    SICP_UNROLL
    for (int c = 0; c < COLS; ++c) {
      qn[6 * c + row] = y[c];
      y[c] = vn[6 * c + row] * y[c];
    }
  }
  // every column's 256 terms added in block_sum's order, all columns in one pass of barriers
  SICP_UNROLL
  for (int c = 0; c < COLS; ++c) sh[c * 256 + threadIdx.x] = y[c];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      SICP_UNROLL
      for (int c = 0; c < COLS; ++c) sh[c * 256 + threadIdx.x] = sh[c * 256 + threadIdx.x] + sh[c * 256 + threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x < COLS) a.part[(long long)(c0 + threadIdx.x) * a.part_stride + blockIdx.x] = sh[threadIdx.x * 256];
}

// grid: (blocks of 64 nodes, queries)
__global__ __launch_bounds__(kCovLanes) void graph_cov_update_kernel(GraphCovArgs a) {
  __shared__ double sh0[kCovLanes], sh1[kCovLanes];
  const int slot = blockIdx.y, t = threadIdx.x, k = t % 6;
  {
    bool running = false;
    for (int c = 0; c < 6; ++c) running = running || a.S[6 * slot + c].flag == kGraphCovRunning;
    if (!running) return;
  }
  const int n = blockIdx.x * kGraphCovNodes + t / 6;
  const GraphCovColumn* S = a.S + 6 * slot + k;
  double rz = 0, rr = 0;
  if (n < a.n_nodes && S->flag == kGraphCovRunning) {
    const double alpha = S->alpha;
    double r[6], z[6], L[kGraphChol];
    SICP_UNROLL
    for (int d = 0; d < kGraphChol; ++d) L[d] = a.L[(long long)kGraphChol * n + d];
    const long long at = ((long long)n * a.cols + 6ll * slot + k) * 6;
    SICP_UNROLL
    for (int d = 0; d < 6; ++d) {
      a.x[at + d] += alpha * a.p[at + d];
      r[d] = a.r[at + d] - alpha * a.q[at + d];
      a.r[at + d] = r[d];
    }
    chol_apply(L, r, z);
    SICP_UNROLL
    for (int d = 0; d < 6; ++d) {
      a.z[at + d] = z[d];
      rz += r[d] * z[d];
      rr += r[d] * r[d];
    }
  }
  node_block_sums(a, rz, rr, sh0, sh1, slot);
}

__global__ __launch_bounds__(256) void graph_cov_direction_kernel(GraphCovArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 6ll * a.n_nodes * a.cols) return;
  const GraphCovColumn* S = a.S + (t / 6) % a.cols;
  if (S->flag != kGraphCovRunning) return;
  a.p[t] = a.z[t] + S->beta * a.p[t];
}

// One workgroup per column: the column's `count` partials added in index order (lane t takes a run of consecutive ones, the
// runs are added in lane order), then lane 0 takes the step of the column's scalars.
template <int FIN>
__global__ __launch_bounds__(256) void graph_cov_finish_kernel(GraphCovArgs a, int count) {
  __shared__ double sh[256];
  const int col = blockIdx.x;
  GraphCovColumn* S = a.S + col;
  if (FIN != kCovFinStart && S->flag != kGraphCovRunning) return;
  constexpr int SUMS = FIN == kCovFinPq ? 1 : 2;
  const int run = (count + 255) / 256;
  const int lo = min(threadIdx.x * run, count), hi = min(lo + run, count);
  double c[2] = {0, 0};
  SICP_UNROLL
  for (int s = 0; s < SUMS; ++s) {
    const double* part = a.part + ((long long)s * a.cols + col) * a.part_stride;
    double v = 0;
    for (int k = lo; k < hi; ++k) v = v + part[k];
    c[s] = block_sum(v, sh);
  }
  if (threadIdx.x != 0) return;
  if (FIN == kCovFinStart) {
    S->rz = c[0]; S->rr = c[1]; S->bb = c[1];
    S->pq = 0; S->alpha = 0; S->beta = 0;
    S->iters = 0;
    int flag = kGraphCovRunning;
    if (*a.bad || !finite(c[0]) || !finite(c[1])) flag = kGraphCovBreakdown;
    else if (c[1] == 0.0) flag = kGraphCovConverged;
    S->flag = flag;
  } else if (FIN == kCovFinPq) {
    S->pq = c[0];
    if (!finite(c[0]) || !(c[0] > 0.0)) S->flag = kGraphCovBreakdown;
    else S->alpha = S->rz / c[0];
  } else {
    S->rr = c[1];
    if (!finite(c[0]) || !finite(c[1])) {
      S->flag = kGraphCovBreakdown;
    } else {
      S->beta = c[0] / S->rz;
      S->rz = c[0];
      S->iters += 1;
      if (sqrt(c[1]) <= a.tolerance * sqrt(S->bb)) S->flag = kGraphCovConverged;
      else if (S->iters >= a.max_iters) S->flag = kGraphCovLimit;
    }
  }
}

// one lane per (query, i, k): S = J X, out = (S + S^T) / 2.  X's column 6 slot + k holds H^-1 (row k of J)^T.
__device__ __forceinline__ double jx_entry(const GraphCovArgs& a, int slot, bool afree, bool bfree, int qa, int qb, int i, int k) {
  const long long col = 6ll * slot + k;
  double s = 0;
  if (afree) {
    const double* xa = a.x + ((long long)qa * a.cols + col) * 6;
    const double* Ji = a.J + 36ll * slot + 6 * i;
    SICP_UNROLL
    for (int j = 0; j < 6; ++j) s += Ji[j] * xa[j];
  }
  if (bfree) s += a.x[((long long)qb * a.cols + col) * 6 + i];
  return s;
}
__global__ __launch_bounds__(256) void graph_cov_extract_kernel(GraphCovArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 6 * a.cols) return;
  const int slot = t / 36, i = (t % 36) / 6, k = t % 6;
  const int qa = a.qa[slot], qb = a.qb[slot];
  const bool afree = qa >= 0 && !a.fixed[qa], bfree = !a.fixed[qb];
  const double u = jx_entry(a, slot, afree, bfree, qa, qb, i, k), v = jx_entry(a, slot, afree, bfree, qa, qb, k, i);
  a.out[t] = i <= k ? 0.5 * (u + v) : 0.5 * (v + u);
}

}  // namespace

hipError_t launch_graph_cov_factor(const GraphCovArgs& a, hipStream_t st) {
  graph_cov_factor_kernel<<<graph_blocks(a.n_nodes), 256, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_graph_cov_begin(const GraphCovArgs& a, hipStream_t st) {
  const int bn = graph_cov_node_blocks(a.n_nodes);
  graph_cov_begin_kernel<<<dim3(bn, a.cols / 6), kCovLanes, 0, st>>>(a);
  graph_cov_finish_kernel<kCovFinStart><<<a.cols, 256, 0, st>>>(a, bn);
  return hipGetLastError();
}

hipError_t launch_graph_cov_iteration(const GraphCovArgs& a, hipStream_t st) {
  const int bn = graph_cov_node_blocks(a.n_nodes), br = graph_blocks(6ll * a.n_nodes);
  const int chunk = graph_cov_spmm_cols(a.cols);
  if (chunk == 24) graph_spmm_kernel<24><<<dim3(br, a.cols / 24), 256, 0, st>>>(a);
  else if (chunk == 12) graph_spmm_kernel<12><<<dim3(br, a.cols / 12), 256, 0, st>>>(a);
  else graph_spmm_kernel<6><<<dim3(br, a.cols / 6), 256, 0, st>>>(a);
  graph_cov_finish_kernel<kCovFinPq><<<a.cols, 256, 0, st>>>(a, br);
  graph_cov_update_kernel<<<dim3(bn, a.cols / 6), kCovLanes, 0, st>>>(a);
  graph_cov_finish_kernel<kCovFinRz><<<a.cols, 256, 0, st>>>(a, bn);
  graph_cov_direction_kernel<<<graph_blocks(6ll * a.n_nodes * a.cols), 256, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_graph_cov_extract(const GraphCovArgs& a, hipStream_t st) {
  graph_cov_extract_kernel<<<graph_blocks(6ll * a.cols), 256, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace sicp
