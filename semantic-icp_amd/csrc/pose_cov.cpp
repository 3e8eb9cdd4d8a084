// pose_cov.cpp -- sicp_pose_covariance / sicp_pose_covariance_batch (include/sicp.h): the search and the accumulate sweep at
// the pose (the same calls as sicp_correspondences + sicp_accumulate, hence the same bits), the cross sums S_src / S_tgt of
// pose_cov_kernels.hip, and the 6x6 algebra on the host.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

bool sigma_ok(double s) { return std::isfinite(s) && s >= 0.0; }

// The call's device scratch (~152 bytes per slot: B^q, the keys, the sorted keys, the sort's storage).  It lives for one
// call, shared by the pairs of a batch, and goes back to the arena at the end instead of staying with a handle (or with a
// parked one after sicp_destroy).  When every launch that used it has completed (`idle`: the stream was synchronised
// behind them) the arena's device-wide wait is skipped, as inside a DevArena::FreeScope; after an error it is not.
struct PoseCovScratch {
  DevBuf<double> bq, piece, part_src, part_tgt, out42;
  DevBuf<unsigned long long> key, key_sorted;
  DevBuf<int> flag;
  DevBuf<long long> part_active, active;
  DevBuf<unsigned char> sort_temp;
  int device = -1;
  bool idle = true;
  PoseCovScratch() = default;
  PoseCovScratch(const PoseCovScratch&) = delete;
  PoseCovScratch& operator=(const PoseCovScratch&) = delete;
  ~PoseCovScratch() {
    int& scope = DevArena::scope_device();
    const int prev = scope;
    if (idle && device >= 0) scope = device;
    bq.release(); piece.release(); part_src.release(); part_tgt.release(); out42.release();
    key.release(); key_sorted.release(); flag.release(); part_active.release(); active.release(); sort_temp.release();
    scope = prev;
  }
};

// S_src (out42[0:21]), S_tgt (out42[21:42]) and the active slot count of the current correspondences at qt
int pose_cov_sums(sicp_context* h, PoseCovScratch& X, const double* qt, double* out42, long long* active) {
  const sicp_params& P = h->params;
  const int n_s = h->corr_n, K = h->corr_K;
  const int total = n_s * K;
  std::fill(out42, out42 + 42, 0.0);
  *active = 0;
  if (total == 0) return SICP_OK;
  const int sb = sicp::pose_cov_blocks(n_s), tiles = sicp::pose_cov_tiles(total), tb = sicp::pose_cov_blocks(tiles);
  HIPCHECK(X.bq.reserve((size_t)total * 18));
  HIPCHECK(X.key.reserve((size_t)total));
  HIPCHECK(X.key_sorted.reserve((size_t)total));
  HIPCHECK(X.piece.reserve((size_t)tiles * 36));
  HIPCHECK(X.flag.reserve((size_t)tiles));
  HIPCHECK(X.part_src.reserve((size_t)sb * 21));
  HIPCHECK(X.part_active.reserve((size_t)sb));
  HIPCHECK(X.part_tgt.reserve((size_t)tb * 42));
  HIPCHECK(X.out42.reserve(42));
  HIPCHECK(X.active.reserve(1));
  size_t sort_bytes = 0;
  HIPCHECK(sicp::boot_sort_keys(nullptr, sort_bytes, X.key.p, X.key_sorted.p, total, h->stream));
  HIPCHECK(X.sort_temp.reserve(sort_bytes));
  X.device = h->device;
  X.idle = false;

  sicp::PoseCovArgs a{};
  a.n_s = n_s; a.K = K;
  a.idx = h->idx.p;
  a.w = h->corr_weighted ? h->w.p : nullptr;
  a.srec = h->cloud(0).rec.p; a.trec = h->cloud(1).rec.p;
  fill_pose(qt, a.pose);
  a.one_m_eps = 1.0 - P.epsilon;
  a.cauchy_a = P.cauchy_a;
  a.use_sqloss = P.use_sqloss;
  a.bq = X.bq.p; a.key = X.key.p;
  a.part_src = X.part_src.p; a.part_active = X.part_active.p;
  HIPCHECK(sicp::launch_pose_cov_src(a, h->stream));
  HIPCHECK(sicp::boot_sort_keys(X.sort_temp.p, sort_bytes, X.key.p, X.key_sorted.p, total, h->stream));
  sicp::PoseCovTgtArgs t{};
  t.total = total;
  t.key = X.key_sorted.p;
  t.bq = X.bq.p;
  t.piece = X.piece.p; t.flag = X.flag.p;
  t.part_tgt = X.part_tgt.p;
  HIPCHECK(sicp::launch_pose_cov_tgt(t, h->stream));
  HIPCHECK(sicp::launch_pose_cov_finalize(X.part_src.p, X.part_active.p, sb, X.part_tgt.p, 2 * tb, X.out42.p, X.active.p, h->stream));
  HIPCHECK(hipMemcpyAsync(out42, X.out42.p, sizeof(double) * 42, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipMemcpyAsync(active, X.active.p, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  X.idle = true;
  return SICP_OK;
}

void full6(const double* u21, double (&F)[6][6]) {
  int o = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b, ++o) F[a][b] = F[b][a] = u21[o];
}

// covariance_gn = H^-1 through the Cholesky factor (H^-1 = L^-T L^-1), covariance = H^-1 X H^-1; both written as their upper
// triangle and mirrored, so they are bit-symmetric.  Returns false (nothing written) when H is not positive definite.
bool combine(const double* H21, const double* Ss21, const double* St21, double sigma_source, double sigma_target, double* cov,
             double* cov_gn) {
  double H[6][6], L[6][6] = {}, Li[6][6] = {}, Hi[6][6], Xs[6][6], Xt[6][6];
  full6(H21, H);
  for (int j = 0; j < 6; ++j) {
    double d = H[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    L[j][j] = std::sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double v = H[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  for (int c = 0; c < 6; ++c) {  // L^-1 by forward substitution, column by column
    Li[c][c] = 1.0 / L[c][c];
    for (int i = c + 1; i < 6; ++i) {
      double v = 0.0;
      for (int k = c; k < i; ++k) v -= L[i][k] * Li[k][c];
      Li[i][c] = v / L[i][i];
    }
  }
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      double v = 0.0;
      for (int k = b; k < 6; ++k) v += Li[k][a] * Li[k][b];
      Hi[a][b] = Hi[b][a] = v;
    }
  full6(Ss21, Xs);
  full6(St21, Xt);
  const double vs = sigma_source * sigma_source, vt = sigma_target * sigma_target;
  double Y[6][6];  // X H^-1
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) {
      double v = 0.0;
      for (int k = 0; k < 6; ++k) v += (vs * Xs[a][k] + vt * Xt[a][k]) * Hi[k][b];
      Y[a][b] = v;
    }
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      double v = 0.0;
      for (int k = 0; k < 6; ++k) v += Hi[a][k] * Y[k][b];
      cov[6 * a + b] = cov[6 * b + a] = v;
      cov_gn[6 * a + b] = cov_gn[6 * b + a] = Hi[a][b];
    }
  bool finite = true;
  for (int e = 0; e < 36; ++e) finite = finite && std::isfinite(cov[e]) && std::isfinite(cov_gn[e]);
  return finite;
}

// one pair; sigmas already checked
int covariance_one(sicp_context* h, PoseCovScratch& X, const double* qt, double sigma_source, double sigma_target,
                   sicp_pose_covariance_result* out) {
  if (general_covariances(h)) {
    h->last_error = "sicp_pose_covariance: a cloud holds caller covariances of general form (sicp_set_covariances); the pose covariance is "
                    "defined for covariances I - (1 - epsilon) n n^T only";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  SICPCHECK(set_device(h));
  SICPCHECK(check_ready(h, false));
  SICPCHECK(search_at(h, qt));
  sicp_pose_covariance_result r;
  std::memset(&r, 0, sizeof r);
  double out28[28], sums[42];
  long long active = 0;
  SICPCHECK(eval28(h, qt, out28));
  SICPCHECK(pose_cov_sums(h, X, qt, sums, &active));
  std::memcpy(r.hessian, out28, sizeof r.hessian);
  std::memcpy(r.gradient, out28 + 21, sizeof r.gradient);
  r.cost = out28[27];
  std::memcpy(r.cross_source, sums, sizeof r.cross_source);
  std::memcpy(r.cross_target, sums + 21, sizeof r.cross_target);
  r.active = active;
  r.positive_definite = combine(r.hessian, r.cross_source, r.cross_target, sigma_source, sigma_target, r.covariance, r.covariance_gn) ? 1 : 0;
  if (!r.positive_definite) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::fill(r.covariance, r.covariance + 36, nan);
    std::fill(r.covariance_gn, r.covariance_gn + 36, nan);
  }
  *out = r;
  return SICP_OK;
}

}  // namespace

int pose_covariance(sicp_context* h, const double* qt, double sigma_source, double sigma_target, sicp_pose_covariance_result* out) {
  if (!h || !qt || !out) return SICP_ERR_INVALID_ARGUMENT;
  if (!sigma_ok(sigma_source) || !sigma_ok(sigma_target)) {
    h->last_error = "sicp_pose_covariance: sigma_source and sigma_target must be finite and >= 0";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  PoseCovScratch X;
  return covariance_one(h, X, qt, sigma_source, sigma_target, out);
}

int pose_covariance_batch(sicp_handle* hs, int32_t n, const double* qt, double sigma_source, double sigma_target,
                          sicp_pose_covariance_result* out, int32_t* status) {
  if (!hs || n < 1) return SICP_ERR_INVALID_ARGUMENT;
  sicp_context* h0 = hs[0];
  auto refuse = [&](const std::string& why) {
    if (h0) h0->last_error = "sicp_pose_covariance_batch: " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  for (int i = 0; i < n; ++i)
    if (!hs[i]) return refuse("handle " + std::to_string(i) + " is NULL");
  if (!qt) return refuse("qt is NULL");
  if (!out) return refuse("out is NULL");
  if (!sigma_ok(sigma_source) || !sigma_ok(sigma_target)) return refuse("sigma_source and sigma_target must be finite and >= 0");
  for (int i = 1; i < n; ++i)
    if (hs[i]->device != h0->device)
      return refuse("handle " + std::to_string(i) + " is on device " + std::to_string(hs[i]->device) + ", handle 0 on " + std::to_string(h0->device));
  // Pairs run one after another through the lone path (its own search, sweep, sort and read-back per pair), sharing one
  // scratch: every row has the bits of its lone call.  Launches are not shared across pairs.
  PoseCovScratch X;
  int first = SICP_OK;
  for (int i = 0; i < n; ++i) {
    sicp_pose_covariance_result r;
    int s;
    try {
      s = covariance_one(hs[i], X, qt + 7 * (size_t)i, sigma_source, sigma_target, &r);
    } catch (const std::bad_alloc&) {
      s = SICP_ERR_OUT_OF_MEMORY;
    }
    if (s == SICP_OK) out[i] = r;
    else if (first == SICP_OK) {
      first = s;
      if (h0 != hs[i]) h0->last_error = "sicp_pose_covariance_batch: pair " + std::to_string(i) + ": " + hs[i]->last_error;
    }
    if (s != SICP_OK) hs[i]->last_error = "sicp_pose_covariance_batch: pair " + std::to_string(i) + ": " + hs[i]->last_error;
    if (status) status[i] = s;
  }
  return first;
}

}  // namespace host
}  // namespace sicp
