// graph.cpp -- sicp_graph_* (include/sicp.h): a pose graph that lives on the device between calls.  Nodes, edges and priors lie
// one after another in one of two sets of arena buffers each; growth doubles into the spare set and swaps last, and every check of a
// call comes before its first write, so a refused call leaves the graph as it was.  The outer Levenberg-Marquardt loop runs
// here with one read-back per iteration (and one per batch of conjugate-gradient steps); the kernels: graph_kernels.hip, the
// sort and the scan of prim_kernels.hip.  At the end: sicp_graph_marginals / sicp_graph_relative_covariances, blocks of H^-1 by
// lock-step conjugate gradients on many right-hand sides (graph_cov_kernels.hip).
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

#define GRAPHCHECK(expr)                                                                       \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      G->last_error = std::string(G->call) + ": " #expr ": " + hipGetErrorString(_e) +         \
                      "; the graph is unchanged";                                              \
      return _e == hipErrorOutOfMemory ? SICP_ERR_OUT_OF_MEMORY : SICP_ERR_HIP;                \
    }                                                                                          \
  } while (0)

bool in_range(double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi; }

bool params_ok(const sicp_graph_params& p) {
  if (p.loss != SICP_GRAPH_LOSS_NONE && p.loss != SICP_GRAPH_LOSS_CAUCHY) return false;
  if (p.max_iterations < 0) return false;
  if (!std::isfinite(p.cauchy_a) || !(p.cauchy_a > 0.0)) return false;
  const double big = std::numeric_limits<double>::max();
  if (!in_range(p.gradient_tolerance, 0, big) || !in_range(p.function_tolerance, 0, big) || !in_range(p.parameter_tolerance, 0, big)) return false;
  if (!std::isfinite(p.min_radius) || !(p.min_radius > 0.0) || !std::isfinite(p.max_radius)) return false;
  if (!in_range(p.initial_radius, p.min_radius, p.max_radius)) return false;
  if (!(p.min_relative_decrease >= 0.0) || !(p.min_relative_decrease < 1.0)) return false;
  if (!std::isfinite(p.min_lm_diagonal) || !(p.min_lm_diagonal > 0.0) || !in_range(p.max_lm_diagonal, p.min_lm_diagonal, big)) return false;
  if (p.max_consecutive_invalid_steps < 1 || p.max_cg_iterations < 1 || p.cg_check_every < 1) return false;
  return p.cg_eta > 0.0 && p.cg_eta < 1.0;
}

// the first bad pose of qt[7 n] with the reason, or -1
long long first_bad_pose(const double* qt, long long n, std::string& why) {
  for (long long k = 0; k < n; ++k) {
    const double* q = qt + 7 * k;
    for (int d = 0; d < 7; ++d)
      if (!std::isfinite(q[d])) { why = "is not finite"; return k; }
    const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(std::fabs(norm - 1.0) <= 1e-6)) { why = "has a quaternion of norm " + std::to_string(norm); return k; }
  }
  return -1;
}
void store_pose(const double* q, double* o) {
  const double inv = 1.0 / std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int d = 0; d < 4; ++d) o[d] = q[d] * inv;
  for (int d = 4; d < 7; ++d) o[d] = q[d];
}

// (Omega + Omega^T) / 2 of an n x n information matrix (6; 3: a position prior's) into out, or the reason it is refused
bool take_omega(const double* om, int n, double* out, std::string& why) {
  double big = 0;
  for (int k = 0; k < n * n; ++k) {
    if (!std::isfinite(om[k])) { why = "has an information matrix that is not finite"; return false; }
    big = std::max(big, std::fabs(om[k]));
  }
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < a; ++b)
      if (std::fabs(om[n * a + b] - om[n * b + a]) > 1e-9 * big) { why = "has an information matrix that is not symmetric"; return false; }
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) out[n * a + b] = 0.5 * (om[n * a + b] + om[n * b + a]);
  bool pd = true;
  if (n == 6) {
    double A[36], rhs[6] = {0, 0, 0, 0, 0, 0}, y[6];
    std::memcpy(A, out, sizeof A);
    pd = sicp::detail::chol6_solve(A, rhs, y);
  } else {  // 3 x 3 by hand: every pivot must be > 0
    double L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 3 && pd; ++i)
      for (int j = 0; j <= i && pd; ++j) {
        double t = out[3 * i + j];
        for (int k = 0; k < j; ++k) t -= L[3 * i + k] * L[3 * j + k];
        if (i == j) {
          pd = t > 0.0 && std::isfinite(t);
          L[3 * i + i] = std::sqrt(t);
        } else {
          L[3 * i + j] = t / L[3 * j + j];
        }
      }
  }
  if (!pd) why = "has an information matrix that is not positive definite";
  return pd;
}

int resolve_range(const sicp_graph_ctx* G, int32_t first, int32_t count, std::string& why) {
  if (first < 0 || count < 1) { why = "first must be >= 0 and count >= 1"; return SICP_ERR_INVALID_ARGUMENT; }
  if ((long long)first + count > G->n_nodes) {
    why = "the range " + std::to_string(first) + " + " + std::to_string(count) + " reaches beyond the " + std::to_string(G->n_nodes) + " nodes";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  return SICP_OK;
}

// Room for n more nodes / m more edges in the spare set at twice the capacity, the contents copied, the swap last.
int grow_nodes(sicp_graph_ctx* G, long long n) {
  const long long need = G->n_nodes + n;
  if (need <= G->cap_nodes) return SICP_OK;
  const long long want = std::max<long long>(std::max<long long>(need, 2 * G->cap_nodes), 64);
  auto& cur = G->nodes[G->ncur];
  auto& spare = G->nodes[G->ncur ^ 1];
  GRAPHCHECK(spare.pose.reserve((size_t)want * 7));
  GRAPHCHECK(spare.fixed.reserve((size_t)want));
  if (G->n_nodes > 0) {
    GRAPHCHECK(hipMemcpyAsync(spare.pose.p, cur.pose.p, sizeof(double) * 7 * (size_t)G->n_nodes, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipMemcpyAsync(spare.fixed.p, cur.fixed.p, (size_t)G->n_nodes, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipStreamSynchronize(G->stream));
  }
  G->ncur ^= 1;
  G->cap_nodes = want;
  DevArena::FreeScope idle(G->device);  // (nothing reads the old set any more)
  cur.pose.release();
  cur.fixed.release();
  return SICP_OK;
}

int grow_edges(sicp_graph_ctx* G, long long m) {
  const long long need = G->n_edges + m;
  if (need <= G->cap_edges) return SICP_OK;
  const long long want = std::max<long long>(std::max<long long>(need, 2 * G->cap_edges), 64);
  auto& cur = G->edges[G->ecur];
  auto& spare = G->edges[G->ecur ^ 1];
  GRAPHCHECK(spare.i.reserve((size_t)want));
  GRAPHCHECK(spare.j.reserve((size_t)want));
  GRAPHCHECK(spare.z.reserve((size_t)want * 7));
  GRAPHCHECK(spare.omega.reserve((size_t)want * 36));
  GRAPHCHECK(spare.enabled.reserve((size_t)want));
  if (G->n_edges > 0) {
    const size_t M = (size_t)G->n_edges;
    GRAPHCHECK(hipMemcpyAsync(spare.enabled.p, cur.enabled.p, M, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipMemcpyAsync(spare.i.p, cur.i.p, sizeof(int) * M, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipMemcpyAsync(spare.j.p, cur.j.p, sizeof(int) * M, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipMemcpyAsync(spare.z.p, cur.z.p, sizeof(double) * 7 * M, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipMemcpyAsync(spare.omega.p, cur.omega.p, sizeof(double) * 36 * M, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipStreamSynchronize(G->stream));
  }
  G->ecur ^= 1;
  G->cap_edges = want;
  DevArena::FreeScope idle(G->device);
  cur.i.release(); cur.j.release(); cur.z.release(); cur.omega.release(); cur.enabled.release();
  return SICP_OK;
}

int grow_priors(sicp_graph_ctx* G, long long m) {
  const long long need = G->n_priors + m;
  if (need <= G->cap_priors) return SICP_OK;
  const long long want = std::max<long long>(std::max<long long>(need, 2 * G->cap_priors), 64);
  auto& cur = G->priors[G->pcur];
  auto& spare = G->priors[G->pcur ^ 1];
  GRAPHCHECK(spare.node.reserve((size_t)want));
  GRAPHCHECK(spare.kind.reserve((size_t)want));
  GRAPHCHECK(spare.z.reserve((size_t)want * 7));
  GRAPHCHECK(spare.omega.reserve((size_t)want * 36));
  GRAPHCHECK(spare.enabled.reserve((size_t)want));
  if (G->n_priors > 0) {
    const size_t P = (size_t)G->n_priors;
    GRAPHCHECK(hipMemcpyAsync(spare.node.p, cur.node.p, sizeof(int) * P, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipMemcpyAsync(spare.kind.p, cur.kind.p, sizeof(int) * P, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipMemcpyAsync(spare.z.p, cur.z.p, sizeof(double) * 7 * P, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipMemcpyAsync(spare.omega.p, cur.omega.p, sizeof(double) * 36 * P, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipMemcpyAsync(spare.enabled.p, cur.enabled.p, P, hipMemcpyDeviceToDevice, G->stream));
    GRAPHCHECK(hipStreamSynchronize(G->stream));
  }
  G->pcur ^= 1;
  G->cap_priors = want;
  DevArena::FreeScope idle(G->device);
  cur.node.release(); cur.kind.release(); cur.z.release(); cur.omega.release(); cur.enabled.release();
  return SICP_OK;
}

// the work buffers at the graph's size, and the kernels' arguments
int prepare(sicp_graph_ctx* G, sicp::GraphArgs& A) {
  const size_t N = (size_t)std::max<long long>(G->n_nodes, 1), M = (size_t)std::max<long long>(G->n_edges, 1), P = (size_t)G->n_priors;
  const int stride = sicp::graph_blocks((long long)std::max(6 * N, M + P));
  GRAPHCHECK(G->C.reserve(2 * M * sicp::kGraphRec)); GRAPHCHECK(G->B.reserve(36 * M)); GRAPHCHECK(G->r.reserve(6 * M));
  GRAPHCHECK(G->s.reserve(M)); GRAPHCHECK(G->w.reserve(M)); GRAPHCHECK(G->ec.reserve(M + P));
  if (P > 0) {
    GRAPHCHECK(G->PC.reserve(P * sicp::kGraphRec)); GRAPHCHECK(G->pr.reserve(6 * P)); GRAPHCHECK(G->ps.reserve(P)); GRAPHCHECK(G->pw.reserve(P));
    GRAPHCHECK(G->pinc.reserve(P)); GRAPHCHECK(G->poff.reserve(N + 1)); GRAPHCHECK(G->pheld.reserve(N));
  }
  GRAPHCHECK(G->H.reserve(36 * N)); GRAPHCHECK(G->g.reserve(6 * N)); GRAPHCHECK(G->L.reserve(sicp::kGraphChol * N));
  GRAPHCHECK(G->x.reserve(6 * N)); GRAPHCHECK(G->rr.reserve(6 * N)); GRAPHCHECK(G->zz.reserve(6 * N));
  GRAPHCHECK(G->p.reserve(6 * N)); GRAPHCHECK(G->q.reserve(6 * N)); GRAPHCHECK(G->cand.reserve(7 * N));
  GRAPHCHECK(G->part.reserve(3 * (size_t)stride));
  GRAPHCHECK(G->inc.reserve(2 * M)); GRAPHCHECK(G->off.reserve(N + 1));
  GRAPHCHECK(G->scalars.reserve(1));
  GRAPHCHECK(G->rec.resize(1));
  std::memset(&A, 0, sizeof A);
  A.n_nodes = (int)G->n_nodes; A.n_edges = (int)G->n_edges; A.n_priors = (int)G->n_priors;
  A.pose = G->nodes[G->ncur].pose.p; A.fixed = G->nodes[G->ncur].fixed.p;
  const auto& E = G->edges[G->ecur];
  A.ei = E.i.p; A.ej = E.j.p; A.z = E.z.p; A.omega = E.omega.p;
  A.een = G->n_edges_enabled < G->n_edges ? E.enabled.p : nullptr;
  if (P > 0) {
    const auto& Q = G->priors[G->pcur];
    A.pnode = Q.node.p; A.pkind = Q.kind.p; A.pen = Q.enabled.p; A.pz = Q.z.p; A.pomega = Q.omega.p;
    A.PC = G->PC.p; A.pr = G->pr.p; A.ps = G->ps.p; A.pw = G->pw.p; A.pinc = G->pinc.p; A.poff = G->poff.p;
  }
  A.loss = G->params.loss; A.cauchy_a = G->params.cauchy_a;
  A.C = G->C.p; A.B = G->B.p; A.r = G->r.p; A.s = G->s.p; A.w = G->w.p; A.ec = G->ec.p;
  A.inc = G->inc.p; A.off = G->off.p;
  A.H = G->H.p; A.g = G->g.p; A.L = G->L.p;
  A.x = G->x.p; A.rr = G->rr.p; A.zz = G->zz.p; A.p = G->p.p; A.q = G->q.p; A.cand = G->cand.p;
  A.part = G->part.p; A.part_stride = stride;
  A.S = G->scalars.p;
  A.lo = G->params.min_lm_diagonal; A.hi = G->params.max_lm_diagonal; A.radius = G->params.initial_radius; A.eta = G->params.cg_eta;
  return SICP_OK;
}

// The incidence tables, rebuilt when nodes, edges or priors have been added or an enabled flag has flipped.  Edges: the slots
// 2 * edge + side sorted by node (a stable sort of the node bits: within a node the slots ascend; a disabled edge's slots carry
// the key n_nodes and land behind every list), the degrees' scan.  Priors: the enabled ones by node in ascending id, counted and
// placed on the host from its mirrors, and the per-node flag of an enabled pose prior.
int build_incidence(sicp_graph_ctx* G, sicp::GraphArgs& A) {
  if (!G->incidence_stale) return SICP_OK;
  const long long slots = 2 * G->n_edges, N = G->n_nodes;
  hipStream_t st = G->stream;
  if (G->n_edges_enabled == 0) {  // (every list is empty)
    GRAPHCHECK(hipMemsetAsync(A.off, 0, sizeof(int) * (size_t)(N + 1), st));
  } else {
    GRAPHCHECK(G->keys.reserve((size_t)slots));
    GRAPHCHECK(G->deg.reserve((size_t)N + 1));
    const long long top = A.een ? N + 1 : N;  // the keys' values: the nodes, and n_nodes itself where an edge is disabled
    int bits = 1;
    while (bits < 31 && (1ll << bits) < top) ++bits;
    size_t sort_bytes = 0, scan_bytes = 0;
    GRAPHCHECK(sicp::prim_sort_keys(nullptr, sort_bytes, G->keys.p, G->inc.p, slots, 32, 32 + bits, st));
    GRAPHCHECK(sicp::prim_scan_int(nullptr, scan_bytes, G->deg.p, G->off.p, N + 1, st));
    GRAPHCHECK(G->temp.reserve(std::max(sort_bytes, scan_bytes) + 256));
    A.deg = G->deg.p;
    GRAPHCHECK(hipMemsetAsync(G->deg.p, 0, sizeof(int) * (size_t)(N + 1), st));
    GRAPHCHECK(sicp::launch_graph_keys(A, G->keys.p, st));
    GRAPHCHECK(sicp::prim_sort_keys(G->temp.p, sort_bytes, G->keys.p, G->inc.p, slots, 32, 32 + bits, st));
    GRAPHCHECK(sicp::prim_scan_int(G->temp.p, scan_bytes, G->deg.p, G->off.p, N + 1, st));
  }
  if (G->n_priors > 0) {
    const size_t P = (size_t)G->n_priors, off_bytes = sizeof(int) * (size_t)(N + 1), inc_bytes = sizeof(int) * P;
    GRAPHCHECK(G->stage.resize(off_bytes + inc_bytes + (size_t)N));
    int* off = reinterpret_cast<int*>(G->stage.data());
    int* inc = off + (N + 1);
    uint8_t* held = G->stage.data() + off_bytes + inc_bytes;
    std::memset(G->stage.data(), 0, off_bytes + inc_bytes + (size_t)N);
    for (size_t p = 0; p < P; ++p)
      if (G->h_pen[p]) {
        off[G->h_pnode[p] + 1] += 1;
        if (G->h_pkind[p] == SICP_GRAPH_PRIOR_POSE) held[G->h_pnode[p]] = 1;
      }
    for (long long k = 0; k < N; ++k) off[k + 1] += off[k];
    std::vector<int> at(off, off + N);
    for (size_t p = 0; p < P; ++p)
      if (G->h_pen[p]) inc[at[(size_t)G->h_pnode[p]]++] = (int)p;
    GRAPHCHECK(hipMemcpyAsync(G->poff.p, off, off_bytes, hipMemcpyHostToDevice, st));
    GRAPHCHECK(hipMemcpyAsync(G->pinc.p, inc, inc_bytes, hipMemcpyHostToDevice, st));
    GRAPHCHECK(hipMemcpyAsync(G->pheld.p, held, (size_t)N, hipMemcpyHostToDevice, st));
  }
  GRAPHCHECK(hipStreamSynchronize(st));
  G->incidence_stale = false;
  return SICP_OK;
}

int read_scalars(sicp_graph_ctx* G, sicp::GraphScalars& S) {
  GRAPHCHECK(hipMemcpyAsync(G->rec.data(), G->scalars.p, sizeof(sicp::GraphScalars), hipMemcpyDeviceToHost, G->stream));
  GRAPHCHECK(hipStreamSynchronize(G->stream));
  S = G->rec[0];
  return SICP_OK;
}

int download(sicp_graph_ctx* G, double* dst, const double* src, size_t count) {
  if (!dst || count == 0) return SICP_OK;
  GRAPHCHECK(hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyDeviceToHost, G->stream));
  GRAPHCHECK(hipStreamSynchronize(G->stream));
  return SICP_OK;
}

// every edge and every prior at `pose`: ec, and the records when full; then the sum of ec into S->cost / S->cand_cost
int linearise_entries(sicp_graph_ctx* G, sicp::GraphArgs& A, const double* pose, bool full, int fin) {
  hipStream_t st = G->stream;
  if (G->n_edges > 0) GRAPHCHECK(sicp::launch_graph_linearise(A, pose, full, st));
  if (G->n_priors > 0) GRAPHCHECK(sicp::launch_graph_prior_linearise(A, pose, full, st));
  if (G->n_edges + G->n_priors > 0) GRAPHCHECK(sicp::launch_graph_sum(A, fin, st));
  return SICP_OK;
}

// full linearisation at the current poses: per-edge and per-prior records, H, g, S->cost, S->gmax
int linearise_full(sicp_graph_ctx* G, sicp::GraphArgs& A) {
  hipStream_t st = G->stream;
  const int rc = linearise_entries(G, A, A.pose, true, sicp::kGraphFinCost);
  if (rc != SICP_OK) return rc;
  GRAPHCHECK(sicp::launch_graph_gather(A, st));
  GRAPHCHECK(sicp::launch_graph_sum(A, sicp::kGraphFinGmax, st));
  return SICP_OK;
}

// sicp_graph_errors / sicp_graph_prior_errors: every edge and every prior at the current poses (a disabled one too), the
// graph's whole cost, and the edges' or the priors' chi2, residuals and weights
int entry_errors(sicp_graph_ctx* G, bool priors, double* chi2, double* residual, double* weight, double* cost) {
  if (G->n_edges + G->n_priors == 0) {
    *cost = 0.0;
    return SICP_OK;
  }
  GRAPHCHECK(hipSetDevice(G->device));
  sicp::GraphArgs A;
  int rc = prepare(G, A);
  if (rc != SICP_OK) return rc;
  if ((rc = linearise_entries(G, A, A.pose, true, sicp::kGraphFinCost)) != SICP_OK) return rc;
  sicp::GraphScalars S;
  rc = read_scalars(G, S);
  if (rc != SICP_OK) return rc;
  const size_t M = (size_t)(priors ? G->n_priors : G->n_edges);
  if ((rc = download(G, chi2, priors ? A.ps : A.s, M)) != SICP_OK) return rc;
  if ((rc = download(G, residual, priors ? A.pr : A.r, 6 * M)) != SICP_OK) return rc;
  if ((rc = download(G, weight, priors ? A.pw : A.w, M)) != SICP_OK) return rc;
  *cost = S.cost;
  return SICP_OK;
}

}  // namespace

void graph_default_params(sicp_graph_params* p) {
  std::memset(p, 0, sizeof *p);
  p->loss = SICP_GRAPH_LOSS_NONE;
  p->max_iterations = 100;
  p->cauchy_a = 1.0;
  p->gradient_tolerance = 1e-10;
  p->function_tolerance = 1e-12;
  p->parameter_tolerance = 1e-12;
  p->initial_radius = 1e4;
  p->min_radius = 1e-32;
  p->max_radius = 1e16;
  p->min_relative_decrease = 1e-3;
  p->min_lm_diagonal = 1e-6;
  p->max_lm_diagonal = 1e32;
  p->max_consecutive_invalid_steps = 5;
  p->max_cg_iterations = 500;
  p->cg_eta = 0.1;
  p->cg_check_every = 8;
}

int graph_create(int device_id, const sicp_graph_params* p, sicp_graph_ctx** out) {
  if (!out) return SICP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!p || !params_ok(*p)) return SICP_ERR_INVALID_ARGUMENT;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SICP_ERR_NO_DEVICE;
  if (device_id < 0 || device_id >= n) return SICP_ERR_INVALID_ARGUMENT;
  sicp_graph_ctx* G = new (std::nothrow) sicp_graph_ctx();
  if (!G) return SICP_ERR_OUT_OF_MEMORY;
  G->device = device_id;
  G->params = *p;
  G->params.reserved_ = 0;
  if (hipSetDevice(device_id) != hipSuccess || G->stream.create() != hipSuccess) {
    delete G;
    return SICP_ERR_NO_DEVICE;
  }
  *out = G;
  return SICP_OK;
}

int graph_destroy(sicp_graph_ctx* G) {
  if (!G) return SICP_OK;
  (void)hipSetDevice(G->device);
  if (G->stream) (void)hipStreamSynchronize(G->stream);
  {
    DevArena::FreeScope once(G->device);  // one wait for the device, not one per buffer
    delete G;
  }
  return SICP_OK;
}

int graph_clear(sicp_graph_ctx* G) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->n_nodes = G->n_edges = G->n_fixed = 0;
  G->n_priors = G->n_edges_enabled = G->n_priors_enabled = 0;
  G->h_fixed.clear();
  G->h_ei.clear();
  G->h_ej.clear();
  G->h_een.clear();
  G->h_pen.clear();
  G->h_pnode.clear();
  G->h_pkind.clear();
  G->incidence_stale = true;
  G->anchored_stale = true;
  G->last_error.clear();
  return SICP_OK;
}

int graph_size(sicp_graph_ctx* G, int64_t* n_nodes, int64_t* n_edges) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  if (!n_nodes || !n_edges) {
    G->last_error = "sicp_graph_size: an output is NULL";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  *n_nodes = G->n_nodes;
  *n_edges = G->n_edges;
  return SICP_OK;
}

int graph_add_nodes(sicp_graph_ctx* G, int32_t n, const double* qt, const uint8_t* fixed, int32_t* first_id) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_add_nodes";
  auto refuse = [&](const std::string& why) {
    G->last_error = "sicp_graph_add_nodes: " + why + "; the graph is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (n < 1) return refuse("n must be >= 1");
  if (!qt) return refuse("qt is NULL");
  if (G->n_nodes + (long long)n > 0x7fffffffll) return refuse("the graph would hold more than 2^31 - 1 nodes");
  std::string why;
  const long long bad = first_bad_pose(qt, n, why);
  if (bad >= 0) return refuse("pose " + std::to_string(bad) + " " + why);
  GRAPHCHECK(hipSetDevice(G->device));
  const size_t pose_bytes = sizeof(double) * 7 * (size_t)n;
  GRAPHCHECK(G->stage.resize(pose_bytes + (size_t)n));
  double* sp = reinterpret_cast<double*>(G->stage.data());
  uint8_t* sf = G->stage.data() + pose_bytes;
  long long add_fixed = 0;
  for (long long k = 0; k < n; ++k) {
    store_pose(qt + 7 * k, sp + 7 * k);
    sf[k] = fixed && fixed[k] ? 1 : 0;
    add_fixed += sf[k];
  }
  G->h_fixed.reserve((size_t)(G->n_nodes + n));  // (may throw: before anything changes)
  const int rc = grow_nodes(G, n);
  if (rc != SICP_OK) return rc;
  auto& cur = G->nodes[G->ncur];
  GRAPHCHECK(hipMemcpyAsync(cur.pose.p + 7 * (size_t)G->n_nodes, sp, pose_bytes, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipMemcpyAsync(cur.fixed.p + (size_t)G->n_nodes, sf, (size_t)n, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipStreamSynchronize(G->stream));
  if (first_id) *first_id = (int32_t)G->n_nodes;
  G->h_fixed.insert(G->h_fixed.end(), sf, sf + n);
  G->n_nodes += n;
  G->n_fixed += add_fixed;
  G->incidence_stale = true;  // (the offsets run over the nodes)
  G->anchored_stale = true;
  return SICP_OK;
}

int graph_add_edges(sicp_graph_ctx* G, int32_t m, const int32_t* i, const int32_t* j, const double* z, const double* omega, int32_t* first_id) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_add_edges";
  auto refuse = [&](const std::string& why) {
    G->last_error = "sicp_graph_add_edges: " + why + "; the graph is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (m < 1) return refuse("m must be >= 1");
  if (!i || !j || !z || !omega) return refuse("an array is NULL");
  if (G->n_edges + (long long)m > 0x7fffffffll) return refuse("the graph would hold more than 2^31 - 1 edges");
  for (long long e = 0; e < m; ++e) {
    if (i[e] < 0 || i[e] >= G->n_nodes || j[e] < 0 || j[e] >= G->n_nodes)
      return refuse("edge " + std::to_string(e) + " (" + std::to_string(i[e]) + ", " + std::to_string(j[e]) + ") has an end outside the " +
                    std::to_string(G->n_nodes) + " nodes");
    if (i[e] == j[e]) return refuse("edge " + std::to_string(e) + " joins node " + std::to_string(i[e]) + " to itself");
  }
  std::string why;
  const long long bad = first_bad_pose(z, m, why);
  if (bad >= 0) return refuse("the measurement of edge " + std::to_string(bad) + " " + why);
  GRAPHCHECK(hipSetDevice(G->device));
  const size_t M = (size_t)m, zb = sizeof(double) * 7 * M, ob = sizeof(double) * 36 * M, ib = sizeof(int) * M;
  GRAPHCHECK(G->stage.resize(ob + zb + 2 * ib));
  double* so = reinterpret_cast<double*>(G->stage.data());
  double* sz = so + 36 * M;
  int* si = reinterpret_cast<int*>(sz + 7 * M);
  int* sj = si + M;
  for (size_t e = 0; e < M; ++e) {
    if (!take_omega(omega + 36 * e, 6, so + 36 * e, why)) return refuse("edge " + std::to_string(e) + " " + why);
    store_pose(z + 7 * e, sz + 7 * e);
    si[e] = i[e];
    sj[e] = j[e];
  }
  G->h_ei.reserve((size_t)(G->n_edges + m));  // (may throw: before anything changes)
  G->h_ej.reserve((size_t)(G->n_edges + m));
  G->h_een.reserve((size_t)(G->n_edges + m));
  const int rc = grow_edges(G, m);
  if (rc != SICP_OK) return rc;
  auto& cur = G->edges[G->ecur];
  const size_t at = (size_t)G->n_edges;
  GRAPHCHECK(hipMemcpyAsync(cur.omega.p + 36 * at, so, ob, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipMemcpyAsync(cur.z.p + 7 * at, sz, zb, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipMemcpyAsync(cur.i.p + at, si, ib, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipMemcpyAsync(cur.j.p + at, sj, ib, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipMemsetAsync(cur.enabled.p + at, 1, M, G->stream));  // (every edge is created enabled)
  GRAPHCHECK(hipStreamSynchronize(G->stream));
  if (first_id) *first_id = (int32_t)G->n_edges;
  G->h_ei.insert(G->h_ei.end(), si, si + m);
  G->h_ej.insert(G->h_ej.end(), sj, sj + m);
  G->h_een.insert(G->h_een.end(), M, (uint8_t)1);
  G->n_edges += m;
  G->n_edges_enabled += m;
  G->incidence_stale = true;
  G->anchored_stale = true;
  return SICP_OK;
}

int graph_add_priors(sicp_graph_ctx* G, int32_t kind, int32_t m, const int32_t* node, const double* z, const double* omega, int32_t* first_id) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_add_priors";
  auto refuse = [&](const std::string& why) {
    G->last_error = "sicp_graph_add_priors: " + why + "; the graph is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (kind != SICP_GRAPH_PRIOR_POSE && kind != SICP_GRAPH_PRIOR_POSITION) return refuse("kind " + std::to_string(kind) + " is not a kind of prior");
  if (m < 1) return refuse("m must be >= 1");
  if (!node || !z || !omega) return refuse("an array is NULL");
  if (G->n_priors + (long long)m > 0x7fffffffll) return refuse("the graph would hold more than 2^31 - 1 priors");
  for (long long p = 0; p < m; ++p)
    if (node[p] < 0 || node[p] >= G->n_nodes)
      return refuse("prior " + std::to_string(p) + " names node " + std::to_string(node[p]) + " outside the " + std::to_string(G->n_nodes) + " nodes");
  const bool is_pose = kind == SICP_GRAPH_PRIOR_POSE;
  std::string why;
  if (is_pose) {
    const long long bad = first_bad_pose(z, m, why);
    if (bad >= 0) return refuse("the measurement of prior " + std::to_string(bad) + " " + why);
  } else {
    for (long long k = 0; k < 3ll * m; ++k)
      if (!std::isfinite(z[k])) return refuse("the measurement of prior " + std::to_string(k / 3) + " is not finite");
  }
  GRAPHCHECK(hipSetDevice(G->device));
  const size_t M = (size_t)m, zb = sizeof(double) * 7 * M, ob = sizeof(double) * 36 * M, ib = sizeof(int) * M;
  GRAPHCHECK(G->stage.resize(ob + zb + 2 * ib));
  double* so = reinterpret_cast<double*>(G->stage.data());
  double* sz = so + 36 * M;
  int* sn = reinterpret_cast<int*>(sz + 7 * M);
  int* sk = sn + M;
  std::memset(G->stage.data(), 0, ob + zb);  // (a position prior fills 3 of its 7 and 9 of its 36)
  for (size_t p = 0; p < M; ++p) {
    if (is_pose) {
      if (!take_omega(omega + 36 * p, 6, so + 36 * p, why)) return refuse("prior " + std::to_string(p) + " " + why);
      store_pose(z + 7 * p, sz + 7 * p);
    } else {
      if (!take_omega(omega + 9 * p, 3, so + 36 * p, why)) return refuse("prior " + std::to_string(p) + " " + why);
      for (int d = 0; d < 3; ++d) sz[7 * p + d] = z[3 * p + d];
    }
    sn[p] = node[p];
    sk[p] = kind;
  }
  G->h_pnode.reserve((size_t)(G->n_priors + m));  // (may throw: before anything changes)
  G->h_pkind.reserve((size_t)(G->n_priors + m));
  G->h_pen.reserve((size_t)(G->n_priors + m));
  const int rc = grow_priors(G, m);
  if (rc != SICP_OK) return rc;
  auto& cur = G->priors[G->pcur];
  const size_t at = (size_t)G->n_priors;
  GRAPHCHECK(hipMemcpyAsync(cur.omega.p + 36 * at, so, ob, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipMemcpyAsync(cur.z.p + 7 * at, sz, zb, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipMemcpyAsync(cur.node.p + at, sn, ib, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipMemcpyAsync(cur.kind.p + at, sk, ib, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipMemsetAsync(cur.enabled.p + at, 1, M, G->stream));  // (every prior is created enabled)
  GRAPHCHECK(hipStreamSynchronize(G->stream));
  if (first_id) *first_id = (int32_t)G->n_priors;
  G->h_pnode.insert(G->h_pnode.end(), sn, sn + m);
  G->h_pkind.insert(G->h_pkind.end(), sk, sk + m);
  G->h_pen.insert(G->h_pen.end(), M, (uint8_t)1);
  G->n_priors += m;
  G->n_priors_enabled += m;
  G->incidence_stale = true;
  G->anchored_stale = true;
  return SICP_OK;
}

int graph_set_enabled(sicp_graph_ctx* G, bool priors, int32_t first, int32_t count, const uint8_t* enabled) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = priors ? "sicp_graph_set_priors_enabled" : "sicp_graph_set_edges_enabled";
  auto refuse = [&](const std::string& why) {
    G->last_error = std::string(G->call) + ": " + why + "; the graph is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  const long long have = priors ? G->n_priors : G->n_edges;
  if (first < 0 || count < 1) return refuse("first must be >= 0 and count >= 1");
  if ((long long)first + count > have)
    return refuse("the range " + std::to_string(first) + " + " + std::to_string(count) + " reaches beyond the " + std::to_string(have) +
                  (priors ? " priors" : " edges"));
  if (!enabled) return refuse("enabled is NULL");
  std::vector<uint8_t>& mirror = priors ? G->h_pen : G->h_een;
  long long change = 0;
  bool same = true;
  for (long long k = 0; k < count; ++k) {
    const uint8_t v = enabled[k] ? 1 : 0;
    same = same && v == mirror[(size_t)(first + k)];
    change += (long long)v - (long long)mirror[(size_t)(first + k)];
  }
  if (same) return SICP_OK;  // (the flags have these values: the tables stay)
  GRAPHCHECK(hipSetDevice(G->device));
  GRAPHCHECK(G->stage.resize((size_t)count));
  for (long long k = 0; k < count; ++k) G->stage[(size_t)k] = enabled[k] ? 1 : 0;
  uint8_t* dev = priors ? G->priors[G->pcur].enabled.p : G->edges[G->ecur].enabled.p;
  GRAPHCHECK(hipMemcpyAsync(dev + (size_t)first, G->stage.data(), (size_t)count, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipStreamSynchronize(G->stream));
  for (long long k = 0; k < count; ++k) mirror[(size_t)(first + k)] = G->stage[(size_t)k];
  (priors ? G->n_priors_enabled : G->n_edges_enabled) += change;
  G->incidence_stale = true;
  G->anchored_stale = true;
  return SICP_OK;
}

int graph_get_enabled(sicp_graph_ctx* G, bool priors, int32_t first, int32_t count, uint8_t* enabled) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = priors ? "sicp_graph_get_priors_enabled" : "sicp_graph_get_edges_enabled";
  auto refuse = [&](const std::string& why) {
    G->last_error = std::string(G->call) + ": " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  const long long have = priors ? G->n_priors : G->n_edges;
  if (first < 0 || count < 1) return refuse("first must be >= 0 and count >= 1");
  if ((long long)first + count > have)
    return refuse("the range " + std::to_string(first) + " + " + std::to_string(count) + " reaches beyond the " + std::to_string(have) +
                  (priors ? " priors" : " edges"));
  if (!enabled) return refuse("enabled is NULL");
  const std::vector<uint8_t>& mirror = priors ? G->h_pen : G->h_een;  // (the host's copy is the device's, flag for flag)
  std::memcpy(enabled, mirror.data() + (size_t)first, (size_t)count);
  return SICP_OK;
}

int graph_counts(sicp_graph_ctx* G, int64_t* n_nodes, int64_t* n_edges, int64_t* n_edges_enabled, int64_t* n_priors, int64_t* n_priors_enabled) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  if (n_nodes) *n_nodes = G->n_nodes;
  if (n_edges) *n_edges = G->n_edges;
  if (n_edges_enabled) *n_edges_enabled = G->n_edges_enabled;
  if (n_priors) *n_priors = G->n_priors;
  if (n_priors_enabled) *n_priors_enabled = G->n_priors_enabled;
  return SICP_OK;
}

int graph_set_poses(sicp_graph_ctx* G, int32_t first, int32_t count, const double* qt) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_set_poses";
  auto refuse = [&](const std::string& why) {
    G->last_error = "sicp_graph_set_poses: " + why + "; the graph is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  std::string why;
  if (resolve_range(G, first, count, why) != SICP_OK) return refuse(why);
  if (!qt) return refuse("qt is NULL");
  const long long bad = first_bad_pose(qt, count, why);
  if (bad >= 0) return refuse("pose " + std::to_string(bad) + " " + why);
  GRAPHCHECK(hipSetDevice(G->device));
  const size_t bytes = sizeof(double) * 7 * (size_t)count;
  GRAPHCHECK(G->stage.resize(bytes));
  double* sp = reinterpret_cast<double*>(G->stage.data());
  for (long long k = 0; k < count; ++k) store_pose(qt + 7 * k, sp + 7 * k);
  GRAPHCHECK(hipMemcpyAsync(G->nodes[G->ncur].pose.p + 7 * (size_t)first, sp, bytes, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipStreamSynchronize(G->stream));
  return SICP_OK;
}

int graph_get_poses(sicp_graph_ctx* G, int32_t first, int32_t count, double* qt) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_get_poses";
  auto refuse = [&](const std::string& why) {
    G->last_error = "sicp_graph_get_poses: " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  std::string why;
  if (resolve_range(G, first, count, why) != SICP_OK) return refuse(why);
  if (!qt) return refuse("qt is NULL");
  GRAPHCHECK(hipSetDevice(G->device));
  return download(G, qt, G->nodes[G->ncur].pose.p + 7 * (size_t)first, 7 * (size_t)count);
}

int graph_set_fixed(sicp_graph_ctx* G, int32_t first, int32_t count, const uint8_t* fixed) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_set_fixed";
  auto refuse = [&](const std::string& why) {
    G->last_error = "sicp_graph_set_fixed: " + why + "; the graph is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  std::string why;
  if (resolve_range(G, first, count, why) != SICP_OK) return refuse(why);
  if (!fixed) return refuse("fixed is NULL");
  GRAPHCHECK(hipSetDevice(G->device));
  GRAPHCHECK(G->stage.resize((size_t)count));
  for (long long k = 0; k < count; ++k) G->stage[(size_t)k] = fixed[k] ? 1 : 0;
  GRAPHCHECK(hipMemcpyAsync(G->nodes[G->ncur].fixed.p + (size_t)first, G->stage.data(), (size_t)count, hipMemcpyHostToDevice, G->stream));
  GRAPHCHECK(hipStreamSynchronize(G->stream));
  for (long long k = 0; k < count; ++k) {
    G->n_fixed += (long long)G->stage[(size_t)k] - (long long)G->h_fixed[(size_t)(first + k)];
    G->h_fixed[(size_t)(first + k)] = G->stage[(size_t)k];
  }
  G->anchored_stale = true;
  return SICP_OK;
}

int graph_errors(sicp_graph_ctx* G, double* chi2, double* residual, double* weight, double* cost) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_errors";
  if (!cost) {
    G->last_error = "sicp_graph_errors: cost is NULL; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  return entry_errors(G, false, chi2, residual, weight, cost);
}

int graph_prior_errors(sicp_graph_ctx* G, double* chi2, double* residual, double* weight, double* cost) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_prior_errors";
  if (!cost) {
    G->last_error = "sicp_graph_prior_errors: cost is NULL; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  return entry_errors(G, true, chi2, residual, weight, cost);
}

int graph_linearize(sicp_graph_ctx* G, double* gradient, double* diag_blocks, double* cost) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_linearize";
  if (!cost) {
    G->last_error = "sicp_graph_linearize: cost is NULL; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  if (G->n_nodes == 0) {
    *cost = 0.0;
    return SICP_OK;
  }
  GRAPHCHECK(hipSetDevice(G->device));
  sicp::GraphArgs A;
  int rc = prepare(G, A);
  if (rc != SICP_OK) return rc;
  if ((rc = build_incidence(G, A)) != SICP_OK) return rc;
  const bool entries = G->n_edges + G->n_priors > 0;
  if (!entries) GRAPHCHECK(hipMemsetAsync(A.S, 0, sizeof(sicp::GraphScalars), G->stream));  // (no cost is summed)
  if ((rc = linearise_full(G, A)) != SICP_OK) return rc;
  sicp::GraphScalars S;
  if ((rc = read_scalars(G, S)) != SICP_OK) return rc;
  if ((rc = download(G, gradient, A.g, 6 * (size_t)G->n_nodes)) != SICP_OK) return rc;
  if ((rc = download(G, diag_blocks, A.H, 36 * (size_t)G->n_nodes)) != SICP_OK) return rc;
  *cost = entries ? S.cost : 0.0;
  return SICP_OK;
}

int graph_optimize(sicp_graph_ctx* G, sicp_graph_info* info) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = "sicp_graph_optimize";
  if (!info) {
    G->last_error = "sicp_graph_optimize: info is NULL; the graph is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  const bool nothing = G->n_edges_enabled + G->n_priors_enabled == 0;
  if (nothing || (G->n_fixed == 0 && G->n_priors_enabled == 0)) {
    G->last_error = std::string("sicp_graph_optimize: the graph has no ") +
                    (nothing ? "edge or prior that is enabled" : "fixed node and no enabled prior") + "; the graph is unchanged";
    return SICP_ERR_NOT_READY;
  }
  const sicp_graph_params& P = G->params;
  GRAPHCHECK(hipSetDevice(G->device));
  hipStream_t st = G->stream;
  sicp::GraphArgs A;
  int rc = prepare(G, A);
  if (rc != SICP_OK) return rc;
  if ((rc = build_incidence(G, A)) != SICP_OK) return rc;
  if ((rc = linearise_full(G, A)) != SICP_OK) return rc;
  sicp::GraphScalars S;
  if ((rc = read_scalars(G, S)) != SICP_OK) return rc;
  sicp_graph_info I;
  std::memset(&I, 0, sizeof I);
  double cost = S.cost, gmax = S.gmax, radius = P.initial_radius, decrease_factor = 2.0;
  I.initial_cost = cost;
  int invalid = 0;
  const size_t pose_bytes = sizeof(double) * 7 * (size_t)G->n_nodes;
  double* pose = G->nodes[G->ncur].pose.p;
  for (;;) {
    if (!(gmax > P.gradient_tolerance)) { I.termination = SICP_GRAPH_GRADIENT_TOLERANCE; break; }
    if (I.iterations >= P.max_iterations) { I.termination = SICP_GRAPH_MAX_ITERATIONS; break; }
    if (radius < P.min_radius) { I.termination = SICP_GRAPH_MIN_RADIUS; break; }
    I.iterations++;
    A.radius = radius;
    GRAPHCHECK(sicp::launch_graph_cg_begin(A, st));
    int done = 0;
    for (;;) {  // batches of conjugate-gradient steps, one small record read per batch
      const int batch = std::min(P.cg_check_every, P.max_cg_iterations - done);
      for (int k = 0; k < batch; ++k) GRAPHCHECK(sicp::launch_graph_cg_iteration(A, st));
      if ((rc = read_scalars(G, S)) != SICP_OK) return rc;
      done = S.cg_iters;
      if (S.flag != sicp::kGraphRunning || done >= P.max_cg_iterations || batch <= 0) break;
    }
    I.cg_iterations += S.cg_iters;
    bool valid = S.flag != sicp::kGraphBreakdown;
    double cand_cost = 0, model = 0;
    if (valid) {
      GRAPHCHECK(sicp::launch_graph_candidates(A, st));
      if ((rc = linearise_entries(G, A, A.cand, false, sicp::kGraphFinCandCost)) != SICP_OK) return rc;
      if ((rc = read_scalars(G, S)) != SICP_OK) return rc;
      cand_cost = S.cand_cost;
      model = -S.gx - 0.5 * S.xHx;
      valid = std::isfinite(cand_cost) && std::isfinite(model) && model > 0.0;
      if (valid && std::sqrt(S.xx) <= P.parameter_tolerance * (std::sqrt(S.pose2) + P.parameter_tolerance)) {
        I.termination = SICP_GRAPH_PARAMETER_TOLERANCE;
        break;
      }
    }
    if (!valid) {
      I.invalid_steps++;
      if (++invalid >= P.max_consecutive_invalid_steps) { I.termination = SICP_GRAPH_INVALID_STEPS; break; }
      radius /= decrease_factor;
      decrease_factor *= 2.0;
      continue;
    }
    invalid = 0;
    const double change = cost - cand_cost, rho = change / model;
    if (rho > P.min_relative_decrease) {
      // the candidates become the poses (a copy inside the set that holds them: nothing can refuse between)
      GRAPHCHECK(hipMemcpyAsync(pose, A.cand, pose_bytes, hipMemcpyDeviceToDevice, st));
      if ((rc = linearise_full(G, A)) != SICP_OK) return rc;
      if ((rc = read_scalars(G, S)) != SICP_OK) return rc;
      I.accepted_steps++;
      const double before = cost;
      cost = S.cost;
      gmax = S.gmax;
      const double t = 2.0 * rho - 1.0;
      radius = std::min(P.max_radius, radius / std::max(1.0 / 3.0, 1.0 - t * t * t));
      decrease_factor = 2.0;
      if (std::fabs(change) <= P.function_tolerance * before) { I.termination = SICP_GRAPH_FUNCTION_TOLERANCE; break; }
    } else {
      I.rejected_steps++;
      radius /= decrease_factor;
      decrease_factor *= 2.0;
    }
  }
  I.final_cost = cost;
  I.gradient_max_norm = gmax;
  I.radius = radius;
  *info = I;
  return SICP_OK;
}

// ---- blocks of H^-1: sicp_graph_marginals / sicp_graph_relative_covariances ------------------------------------------------------
namespace {

constexpr int kCovAutoColumns = 24;    // the widest SpMM instantiation: where the time per column stops falling
constexpr int kCovMaxColumns = 1536;   // what one pass takes at the most, whatever max_columns asks for (grid.y of the launches)

bool cov_params_ok(const sicp_graph_cov_params& p) {
  if (!std::isfinite(p.tolerance) || !(p.tolerance > 0.0) || !(p.tolerance < 1.0)) return false;
  if (p.max_cg_iterations < 0 || p.check_every < 1) return false;
  return p.max_columns >= 0 && p.max_columns % 6 == 0;
}

// per node: does its connected component hold a fixed node or a node with an enabled pose prior?  Union-find over the ends of
// the enabled edges, redone when the graph has changed.  (A position prior anchors nothing: one or two leave a rotation free.)
void refresh_anchored(sicp_graph_ctx* G) {
  if (!G->anchored_stale) return;
  const size_t N = (size_t)G->n_nodes;
  std::vector<int32_t> parent(N);
  for (size_t k = 0; k < N; ++k) parent[k] = (int32_t)k;
  auto find = [&](int32_t v) {
    while (parent[(size_t)v] != v) {
      parent[(size_t)v] = parent[(size_t)parent[(size_t)v]];
      v = parent[(size_t)v];
    }
    return v;
  };
  for (size_t e = 0; e < (size_t)G->n_edges; ++e) {
    if (!G->h_een[e]) continue;
    const int32_t a = find(G->h_ei[e]), b = find(G->h_ej[e]);
    if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
  }
  std::vector<uint8_t> root_fixed(N, 0);
  for (size_t k = 0; k < N; ++k)
    if (G->h_fixed[k]) root_fixed[(size_t)find((int32_t)k)] = 1;
  for (size_t p = 0; p < (size_t)G->n_priors; ++p)
    if (G->h_pen[p] && G->h_pkind[p] == SICP_GRAPH_PRIOR_POSE) root_fixed[(size_t)find(G->h_pnode[p])] = 1;
  G->anchored.assign(N, 0);
  for (size_t k = 0; k < N; ++k) G->anchored[k] = root_fixed[(size_t)find((int32_t)k)];
  G->anchored_stale = false;
}

// what the arena takes for `count` elements of T (DevBuf::reserve's request)
template <class T>
size_t arena_bytes(size_t count) { return DevArena::size_class((count + count / 8 + 64) * sizeof(T)); }

size_t cov_part_stride(long long n_nodes) {
  return (size_t)std::max(sicp::graph_cov_node_blocks(n_nodes), sicp::graph_blocks(6 * n_nodes));
}

// the work buffers of a pass of `cols` columns that are not there yet, in bytes of the arena
size_t cov_bytes_missing(const sicp_graph_ctx* G, int cols) {
  const size_t N = (size_t)G->n_nodes, vec = 6 * N * (size_t)cols, part = 2 * (size_t)cols * cov_part_stride(G->n_nodes);
  size_t need = 0;
  const size_t C = (size_t)cols;
  for (const DevBuf<double>* b : {&G->cov_x, &G->cov_r, &G->cov_z, &G->cov_p, &G->cov_q})
    if (b->cap < vec) need += arena_bytes<double>(vec);
  if (G->cov_part.cap < part) need += arena_bytes<double>(part);
  if (G->cov_J.cap < 6 * C) need += arena_bytes<double>(6 * C);
  if (G->cov_out.cap < 6 * C) need += arena_bytes<double>(6 * C);
  if (G->cov_query.cap < C) need += arena_bytes<int>(C);
  if (G->cov_bad.cap < 1) need += arena_bytes<int>(1);
  if (G->cov_cols.cap < C) need += arena_bytes<sicp::GraphCovColumn>(C);
  return need;
}

hipError_t cov_reserve(sicp_graph_ctx* G, int cols) {
  const size_t N = (size_t)G->n_nodes, vec = 6 * N * (size_t)cols, C = (size_t)cols;
  hipError_t e = hipSuccess;
  for (DevBuf<double>* b : {&G->cov_x, &G->cov_r, &G->cov_z, &G->cov_p, &G->cov_q})
    if ((e = b->reserve(vec)) != hipSuccess) return e;
  if ((e = G->cov_part.reserve(2 * C * cov_part_stride(G->n_nodes))) != hipSuccess) return e;
  if ((e = G->cov_J.reserve(6 * C)) != hipSuccess) return e;
  if ((e = G->cov_out.reserve(6 * C)) != hipSuccess) return e;
  if ((e = G->cov_query.reserve(C)) != hipSuccess) return e;  // (2 per query)
  if ((e = G->cov_bad.reserve(1)) != hipSuccess) return e;
  if ((e = G->cov_cols.reserve(C)) != hipSuccess) return e;
  if ((e = G->cov_rec.resize(C)) != hipSuccess) return e;
  if ((e = G->cov_hquery.resize(C)) != hipSuccess) return e;
  return G->cov_hout.resize(6 * C);
}

}  // namespace

void graph_default_cov_params(sicp_graph_cov_params* p) {
  std::memset(p, 0, sizeof *p);
  p->tolerance = 1e-10;
  p->max_cg_iterations = 0;
  p->check_every = 32;
  p->max_columns = 0;
}

int graph_covariances(sicp_graph_ctx* G, bool marginals, const sicp_graph_cov_params* params, int32_t n, const int32_t* a, const int32_t* b,
                      double* cov, int32_t* status, sicp_graph_cov_info* info) {
  if (!G) return SICP_ERR_INVALID_ARGUMENT;
  G->call = marginals ? "sicp_graph_marginals" : "sicp_graph_relative_covariances";
  auto refuse = [&](const std::string& why) {
    G->last_error = std::string(G->call) + ": " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  sicp_graph_cov_params P;
  if (params) P = *params; else graph_default_cov_params(&P);
  if (!cov_params_ok(P))
    return refuse("the parameters are outside their ranges (tolerance in (0, 1), max_cg_iterations >= 0, check_every >= 1, max_columns 0 "
                  "or a multiple of 6)");
  if (n < 1) return refuse("n must be >= 1");
  if (!b || (!marginals && !a) || !cov) return refuse("an array is NULL");
  for (long long q = 0; q < n; ++q) {
    if (b[q] < 0 || b[q] >= G->n_nodes || (!marginals && (a[q] < 0 || a[q] >= G->n_nodes)))
      return refuse("query " + std::to_string(q) + " names a node outside the " + std::to_string(G->n_nodes) + " nodes");
    if (!marginals && a[q] == b[q]) return refuse("query " + std::to_string(q) + " asks for node " + std::to_string(a[q]) + " relative to itself");
  }
  // Every answer is formed in host vectors and copied out at the end: a call that fails on the way has written nothing.
  refresh_anchored(G);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> C36(36 * (size_t)n, 0.0);
  std::vector<int32_t> stat((size_t)n, SICP_GRAPH_COV_OK);
  std::vector<int32_t> solve;  // the queries that need columns
  for (int32_t q = 0; q < n; ++q) {
    const bool afree = !marginals && !G->h_fixed[(size_t)a[q]], bfree = !G->h_fixed[(size_t)b[q]];
    if ((afree && !G->anchored[(size_t)a[q]]) || (bfree && !G->anchored[(size_t)b[q]])) {
      stat[(size_t)q] = SICP_GRAPH_COV_UNANCHORED;
      std::fill(C36.begin() + 36 * (size_t)q, C36.begin() + 36 * (size_t)(q + 1), nan);
    } else if (afree || bfree) {
      solve.push_back(q);
    }  // (otherwise: every end is fixed, the zeros stand)
  }
  sicp_graph_cov_info I;
  std::memset(&I, 0, sizeof I);
  if (!solve.empty()) {
    GRAPHCHECK(hipSetDevice(G->device));
    hipStream_t st = G->stream;
    sicp::GraphArgs A;
    int rc = prepare(G, A);
    if (rc != SICP_OK) return rc;
    if ((rc = build_incidence(G, A)) != SICP_OK) return rc;
    if ((rc = linearise_full(G, A)) != SICP_OK) return rc;  // (a query to solve has an anchored free node: there are edges or pose priors)
    // the columns of a pass: what is asked for, no more than the queries need, and what the arena's limit leaves room for
    int cols = (int)std::min<long long>(std::min(P.max_columns > 0 ? P.max_columns : kCovAutoColumns, kCovMaxColumns), 6ll * (long long)solve.size());
    for (;;) {
      auto& D = dev_arena().dev[G->device % kArenaDevices];
      size_t limit, reserved;
      {
        std::lock_guard<std::mutex> lock(dev_arena().m);
        limit = D.limit; reserved = D.reserved;
      }
      const bool fits = limit == 0 || reserved + cov_bytes_missing(G, cols) <= limit;
      if (fits || cols == 6) {  // (the estimate counts no free room inside the slabs: six columns are tried in any case)
        const hipError_t e = cov_reserve(G, cols);
        if (e == hipSuccess) break;
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory || cols == 6) {
          G->last_error = std::string(G->call) + ": the work buffers of a pass of " + std::to_string(cols) + " columns: " + hipGetErrorString(e) +
                          "; nothing was written and the graph is unchanged";
          return e == hipErrorOutOfMemory ? SICP_ERR_OUT_OF_MEMORY : SICP_ERR_HIP;
        }
      }
      cols = std::max(6, cols / 12 * 6);  // half, in whole queries
    }
    sicp::GraphCovArgs V;
    std::memset(&V, 0, sizeof V);
    V.n_nodes = (int)G->n_nodes;
    V.pose = A.pose; V.fixed = A.fixed; V.ei = A.ei; V.ej = A.ej; V.B = A.B; V.inc = A.inc; V.off = A.off; V.H = A.H; V.L = A.L;
    V.held = G->n_priors > 0 ? G->pheld.p : nullptr;
    V.J = G->cov_J.p; V.x = G->cov_x.p; V.r = G->cov_r.p; V.z = G->cov_z.p; V.p = G->cov_p.p; V.q = G->cov_q.p;
    V.part = G->cov_part.p; V.part_stride = (int)cov_part_stride(G->n_nodes);
    V.S = G->cov_cols.p; V.bad = G->cov_bad.p; V.out = G->cov_out.p;
    V.tolerance = P.tolerance;
    V.max_iters = P.max_cg_iterations > 0 ? P.max_cg_iterations
                                          : (int)std::min<long long>(std::max<long long>(20 * G->n_nodes, 200), 0x7fffffffll);
    GRAPHCHECK(hipMemsetAsync(V.bad, 0, sizeof(int), st));
    V.cols = 6;
    GRAPHCHECK(sicp::launch_graph_cov_factor(V, st));
    const size_t per_pass = (size_t)cols / 6;
    for (size_t first = 0; first < solve.size(); first += per_pass) {
      const size_t slots = std::min(per_pass, solve.size() - first);
      V.cols = 6 * (int)slots;
      int* hq = G->cov_hquery.data();
      for (size_t k = 0; k < slots; ++k) {
        const int32_t q = solve[first + k];
        hq[k] = marginals ? -1 : a[q];
        hq[slots + k] = b[q];
      }
      GRAPHCHECK(hipMemcpyAsync(G->cov_query.p, hq, sizeof(int) * 2 * slots, hipMemcpyHostToDevice, st));
      V.qa = G->cov_query.p; V.qb = G->cov_query.p + slots;
      GRAPHCHECK(sicp::launch_graph_cov_begin(V, st));
      const sicp::GraphCovColumn* S = G->cov_rec.data();
      long long enqueued = 0;
      for (;;) {  // batches of iterations, one read of the columns' records per batch; the device itself stops every column
        GRAPHCHECK(hipMemcpyAsync(G->cov_rec.data(), V.S, sizeof(sicp::GraphCovColumn) * (size_t)V.cols, hipMemcpyDeviceToHost, st));
        GRAPHCHECK(hipStreamSynchronize(st));
        bool running = false;
        for (int c = 0; c < V.cols; ++c) running = running || S[c].flag == sicp::kGraphCovRunning;
        if (!running || enqueued >= (long long)V.max_iters) break;
        const int batch = (int)std::min<long long>(P.check_every, (long long)V.max_iters - enqueued);
        for (int k = 0; k < batch; ++k) GRAPHCHECK(sicp::launch_graph_cov_iteration(V, st));
        enqueued += batch;
      }
      GRAPHCHECK(sicp::launch_graph_cov_extract(V, st));
      GRAPHCHECK(hipMemcpyAsync(G->cov_hout.data(), V.out, sizeof(double) * 36 * slots, hipMemcpyDeviceToHost, st));
      GRAPHCHECK(hipStreamSynchronize(st));
      int pass_iters = 0;
      for (size_t k = 0; k < slots; ++k) {
        const int32_t q = solve[first + k];
        int32_t s = SICP_GRAPH_COV_OK;
        for (int c = 6 * (int)k; c < 6 * (int)k + 6; ++c) {
          pass_iters = std::max(pass_iters, S[c].iters);
          if (S[c].flag == sicp::kGraphCovBreakdown) s = SICP_GRAPH_COV_BREAKDOWN;
          else if (S[c].flag != sicp::kGraphCovConverged && s == SICP_GRAPH_COV_OK) s = SICP_GRAPH_COV_NOT_CONVERGED;
          if (S[c].flag != sicp::kGraphCovBreakdown && S[c].bb > 0.0)
            I.worst_relative_residual = std::max(I.worst_relative_residual, std::sqrt(S[c].rr) / std::sqrt(S[c].bb));
        }
        stat[(size_t)q] = s;
        const double* got = G->cov_hout.data() + 36 * k;
        for (int d = 0; d < 36; ++d) C36[36 * (size_t)q + d] = s == SICP_GRAPH_COV_BREAKDOWN ? nan : got[d];
      }
      I.passes += 1;
      I.cg_iterations += pass_iters;
    }
  }
  for (int32_t q = 0; q < n; ++q) (stat[(size_t)q] == SICP_GRAPH_COV_OK ? I.n_ok : I.n_failed) += 1;
  std::memcpy(cov, C36.data(), sizeof(double) * C36.size());
  if (status) std::memcpy(status, stat.data(), sizeof(int32_t) * stat.size());
  if (info) *info = I;
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
