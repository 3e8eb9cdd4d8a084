// pose_cov.cpp -- sicp_pose_covariance / sicp_pose_covariance_batch / a stream's covariance pass (include/sicp.h): the search
// at the pose (the same calls as sicp_correspondences, hence the same bits), then ONE sweep for a whole group of pairs -- the
// batched accumulate kernel on argument buffers of its own, the job-table kernels of pose_cov_kernels.hip with one sort,
// one read-back -- and the 6x6 algebra on the host.  A lone call is a group of one pair.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

bool sigma_ok(double s) { return std::isfinite(s) && s >= 0.0; }

// What bounds a group: its device scratch (~152 bytes per slot: B^q, the keys, the sorted keys, the sort's
// storage -- at most 1 GiB, and whatever a pair needs that is larger on its own), the 64 bits of a sort key
// (job | target | slot), and the pairs one accumulate launch holds.
constexpr long long kGroupSlots = (1ll << 30) / 152;
int bits_of(unsigned long long v) {
  int b = 0;
  while (v) { ++b; v >>= 1; }
  return b;
}
int slot_bits_of(long long max_total) { return std::max(1, bits_of((unsigned long long)std::max<long long>(max_total - 1, 0))); }
int tgt_bits_of(int max_nt) { return std::max(1, bits_of((unsigned long long)std::max(max_nt, 0))); }
int job_bits_of(int jobs) { return jobs > 1 ? bits_of((unsigned long long)(jobs - 1)) : 0; }
struct GroupBound {
  int jobs = 0, max_nt = 0;
  long long slots = 0, max_total = 0;
  // whether a pair of `total` slots onto `nt` target points may join (an empty group takes any pair)
  bool admits(long long total, int nt) const {
    if (jobs == 0) return true;
    if (jobs + 1 > kMaxActivePairs || slots + total > kGroupSlots) return false;
    return job_bits_of(jobs + 1) + tgt_bits_of(std::max(max_nt, nt)) + slot_bits_of(std::max(max_total, total)) <= 64;
  }
  void add(long long total, int nt) {
    ++jobs; slots += total; max_total = std::max(max_total, total); max_nt = std::max(max_nt, nt);
  }
};

// A sweep's device scratch.  Of a call: it lives for the call, shared by its groups, and goes back to the arena at the end
// instead of staying with a handle (or with a parked one after sicp_destroy).  Of a stream: it stays with the stream.
// (`idle`: DevArena::release_scratch)
struct PoseCovScratch {
  DevBuf<double> bq, piece, part_src, part_tgt, out;
  DevBuf<unsigned long long> key, key_sorted;
  DevBuf<int> flag;
  DevBuf<long long> part_active;
  DevBuf<unsigned char> sort_temp, args;
  int device = -1;
  bool idle = true;
  ~PoseCovScratch() {
    DevArena::release_scratch(device, idle, bq, piece, part_src, part_tgt, out, key, key_sorted, flag, part_active, sort_temp, args);
  }
};

// where a sweep's results arrive (pinned, valid once the stream has passed the read-back): pair i of the call is row pos[i]
struct SweepOut {
  const double* out28 = nullptr;     // [n][28] hessian 21 | gradient 6 | cost
  const double* out42 = nullptr;     // [n][42] S_src 21 | S_tgt 21
  const long long* active = nullptr; // [n]
  std::vector<int> pos;
  void get(int i, PoseCovSums* r) const {
    std::memcpy(r->out28, out28 + 28 * (size_t)pos[i], sizeof r->out28);
    std::memcpy(r->sums, out42 + 42 * (size_t)pos[i], sizeof r->sums);
    r->active = active[pos[i]];
  }
};

// The sweep of a group: n pairs (distinct handles, one device, within a GroupBound) whose current correspondences are those
// at qts[i], complete or queued on `st`.  Everything is queued on `st`, nothing is waited for: the accumulate kernel once per
// run of pairs of equal K and loss (argument array and headers in X.args -- never a handle's tick sets, which the ticks and
// eval28 use), the covariance kernels once each, one sort, one read-back into `pin`.  `h` leads: it takes the error text.
int pose_cov_sweep(sicp_context* h, PoseCovScratch& X, HostBuf<unsigned char>& pin, sicp_context* const* hs, const double* const* qts,
                   int n, hipStream_t st, SweepOut* o) {
  if (n < 1 || n > kMaxActivePairs) return SICP_ERR_INTERNAL;
  // pairs of equal (K, loss) next to each other
  std::vector<int> ord((size_t)n);
  for (int i = 0; i < n; ++i) ord[(size_t)i] = i;
  auto kind = [&](int i) { return hs[i]->corr_K * 2 + (hs[i]->params.use_sqloss ? 1 : 0); };
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return kind(a) < kind(b); });
  o->pos.assign((size_t)n, 0);
  for (int k = 0; k < n; ++k) o->pos[(size_t)ord[(size_t)k]] = k;
  // geometry of the group
  GroupBound gb;
  size_t tiles_all = 0, sb_all = 0, tb_all = 0;
  for (int k = 0; k < n; ++k) {
    sicp_context* g = hs[ord[(size_t)k]];
    const long long total = (long long)g->corr_n * g->corr_K;
    if (total > 0x7fffffffll) return SICP_ERR_INVALID_ARGUMENT;
    gb.add(total, g->cloud(1).n);
    const int tiles = sicp::pose_cov_tiles((int)total);
    tiles_all += (size_t)tiles; sb_all += (size_t)sicp::pose_cov_blocks(g->corr_n); tb_all += (size_t)sicp::pose_cov_blocks(tiles);
  }
  const int slot_bits = slot_bits_of(gb.max_total), tgt_bits = tgt_bits_of(gb.max_nt), end_bit = slot_bits + tgt_bits + job_bits_of(n);
  if (end_bit > 64 || gb.slots > 0x7fffffffll) return SICP_ERR_INTERNAL;
  const size_t slots = (size_t)gb.slots;
  HIPCHECK(X.bq.reserve(std::max<size_t>(slots, 1) * 18));
  HIPCHECK(X.key.reserve(std::max<size_t>(slots, 1)));
  HIPCHECK(X.key_sorted.reserve(std::max<size_t>(slots, 1)));
  HIPCHECK(X.piece.reserve(std::max<size_t>(tiles_all, 1) * 36));
  HIPCHECK(X.flag.reserve(std::max<size_t>(tiles_all, 1)));
  HIPCHECK(X.part_src.reserve(std::max<size_t>(sb_all, 1) * 21));
  HIPCHECK(X.part_active.reserve(std::max<size_t>(sb_all, 1)));
  HIPCHECK(X.part_tgt.reserve(std::max<size_t>(tb_all, 1) * 42));
  HIPCHECK(X.out.reserve((size_t)n * 71));
  size_t sort_bytes = 0;
  if (slots > 0) {
    HIPCHECK(sicp::prim_sort_keys(nullptr, sort_bytes, X.key.p, X.key_sorted.p, (long long)slots, 0, end_bit, st));
    HIPCHECK(X.sort_temp.reserve(sort_bytes + 256));
  }
  // the argument block: headers | accumulate arguments | jobs | the two workgroup prefixes; behind it the results
  // (one job array under two prefixes -- the source kernel's workgroups and the tile / owner kernels')
  typedef sicp::ArgBlock AB;
  AB block;
  const AB::Section s_hdr = block.add<sicp::BatchHeader>((size_t)n), s_batch = block.add<sicp::BatchArgs>((size_t)n),
                    s_jobs = block.add<sicp::PoseCovJob>((size_t)n), s_send = block.add<int>((size_t)n), s_tend = block.add<int>((size_t)n);
  const size_t arg_bytes = block.bytes(), res_bytes = sizeof(double) * 71 * (size_t)n;
  HIPCHECK(X.args.reserve(arg_bytes));
  HIPCHECK(pin.resize(arg_bytes + res_bytes));
  std::memset(pin.data(), 0, arg_bytes);
  sicp::BatchHeader* hdr = AB::host<sicp::BatchHeader>(s_hdr, pin.data());
  sicp::BatchArgs* batch = AB::host<sicp::BatchArgs>(s_batch, pin.data());
  sicp::PoseCovJob* jobs = AB::host<sicp::PoseCovJob>(s_jobs, pin.data());
  int* src_end = AB::host<int>(s_send, pin.data());
  int* tgt_end = AB::host<int>(s_tend, pin.data());
  sicp::BatchHeader* d_hdr = AB::dev<sicp::BatchHeader>(s_hdr, X.args.p);
  sicp::BatchArgs* d_batch = AB::dev<sicp::BatchArgs>(s_batch, X.args.p);
  const sicp::PoseCovJob* d_jobs = AB::dev<sicp::PoseCovJob>(s_jobs, X.args.p);
  const int* d_src_end = AB::dev<int>(s_send, X.args.p);
  const int* d_tgt_end = AB::dev<int>(s_tend, X.args.p);
  double* d_out28 = X.out.p;
  double* d_out42 = X.out.p + 28 * (size_t)n;
  long long* d_active = reinterpret_cast<long long*>(X.out.p + 70 * (size_t)n);
  X.device = h->device;
  X.idle = false;
  size_t off = 0, tile_off = 0, sb_off = 0, tb_off = 0;
  int src_blocks = 0, tgt_blocks = 0;
  for (int k = 0; k < n; ++k) {
    sicp_context* g = hs[ord[(size_t)k]];
    const double* qt = qts[ord[(size_t)k]];
    const sicp_params& P = g->params;
    const int n_s = g->corr_n, K = g->corr_K, total = n_s * K;
    const int nb = sicp::accumulate_blocks(total, K);
    if (g->partials.reserve((size_t)nb * 28) != hipSuccess) { h->last_error = "pose covariance: the accumulate partials"; return SICP_ERR_OUT_OF_MEMORY; }
    fill_acc(g, batch[k].a);
    fill_pose(qt, batch[k].a.pose);
    batch[k].nb = nb;
    const int tiles = sicp::pose_cov_tiles(total), sb = sicp::pose_cov_blocks(n_s), tb = sicp::pose_cov_blocks(tiles);
    sicp::PoseCovJob& J = jobs[k];
    sicp::PoseCovArgs& a = J.a;
    a.n_s = n_s; a.K = K;
    a.idx = g->idx.p;
    a.w = batch[k].a.w;  // the weights of the accumulate launch whose H this covariance is built on (fill_acc)
    a.srec = g->cloud(0).rec.p; a.trec = g->cloud(1).rec.p;
    fill_pose(qt, a.pose);
    a.one_m_eps = 1.0 - P.epsilon;
    a.cauchy_a = P.cauchy_a;
    a.use_sqloss = P.use_sqloss;
    a.bq = X.bq.p + off * 18; a.key = X.key.p + off;
    a.part_src = X.part_src.p + sb_off * 21; a.part_active = X.part_active.p + sb_off;
    J.skey = X.key_sorted.p + off;
    J.piece = X.piece.p + tile_off * 36; J.flag = X.flag.p + tile_off;
    J.part_tgt = X.part_tgt.p + tb_off * 42;
    J.out42 = d_out42 + 42 * (size_t)k; J.active = d_active + k;
    J.job_key = n > 1 ? (unsigned long long)k << (slot_bits + tgt_bits) : 0ull;
    J.n_t = g->cloud(1).n; J.slot_bits = slot_bits; J.tgt_bits = tgt_bits;
    off += (size_t)total; tile_off += (size_t)tiles; sb_off += (size_t)sb; tb_off += (size_t)tb;
    src_blocks += sb; tgt_blocks += tb;
    src_end[k] = src_blocks; tgt_end[k] = tgt_blocks;
  }
  for (int k0 = 0; k0 < n;) {  // one header per accumulate launch: its pairs and the launch's work-split counters
    int k1 = k0 + 1;
    while (k1 < n && kind(ord[(size_t)k1]) == kind(ord[(size_t)k0])) ++k1;
    hdr[k0] = sicp::BatchHeader{k1 - k0, 0u, 0u, 0};
    k0 = k1;
  }
  HIPCHECK(hipMemcpyAsync(X.args.p, pin.data(), arg_bytes, hipMemcpyHostToDevice, st));
  for (int k0 = 0; k0 < n;) {
    const int cnt = hdr[k0].n_pairs;
    sicp_context* g = hs[ord[(size_t)k0]];
    HIPCHECK(sicp::launch_accumulate_batch(g->corr_K, g->params.use_sqloss, d_hdr + k0, d_batch + k0, cnt, st));
    k0 += cnt;
  }
  HIPCHECK(sicp::launch_finalize_batch(d_batch, n, d_out28, st));
  HIPCHECK(sicp::launch_pose_cov_src_jobs(d_jobs, d_src_end, n, src_blocks, st));
  if (slots > 0) HIPCHECK(sicp::prim_sort_keys(X.sort_temp.p, sort_bytes, X.key.p, X.key_sorted.p, (long long)slots, 0, end_bit, st));
  HIPCHECK(sicp::launch_pose_cov_tile_jobs(d_jobs, d_tgt_end, n, tgt_blocks, st));
  HIPCHECK(sicp::launch_pose_cov_owner_jobs(d_jobs, d_tgt_end, n, tgt_blocks, st));
  HIPCHECK(sicp::launch_pose_cov_finalize_jobs(d_jobs, n, st));
  unsigned char* res = pin.data() + arg_bytes;
  HIPCHECK(hipMemcpyAsync(res, X.out.p, res_bytes, hipMemcpyDeviceToHost, st));
  o->out28 = reinterpret_cast<const double*>(res);
  o->out42 = o->out28 + 28 * (size_t)n;
  o->active = reinterpret_cast<const long long*>(o->out28 + 70 * (size_t)n);
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

// the caller's result from a pair's raw sums: the host algebra with the caller's sigmas
void fill_result(const PoseCovSums& u, double sigma_source, double sigma_target, sicp_pose_covariance_result* out) {
  sicp_pose_covariance_result r;
  std::memset(&r, 0, sizeof r);
  std::memcpy(r.hessian, u.out28, sizeof r.hessian);
  std::memcpy(r.gradient, u.out28 + 21, sizeof r.gradient);
  r.cost = u.out28[27];
  std::memcpy(r.cross_source, u.sums, sizeof r.cross_source);
  std::memcpy(r.cross_target, u.sums + 21, sizeof r.cross_target);
  r.active = u.active;
  r.positive_definite = combine(r.hessian, r.cross_source, r.cross_target, sigma_source, sigma_target, r.covariance, r.covariance_gn) ? 1 : 0;
  if (!r.positive_definite) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::fill(r.covariance, r.covariance + 36, nan);
    std::fill(r.covariance_gn, r.covariance_gn + 36, nan);
  }
  *out = r;
}

// what a pair must pass before anything is queued for it
int covariance_ready(sicp_context* h) {
  if (general_covariances(h)) {
    h->last_error = "sicp_pose_covariance: a cloud holds caller covariances of general form (sicp_set_covariances); the pose covariance is "
                    "defined for covariances I - (1 - epsilon) n n^T only";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  SICPCHECK(set_device(h));
  return check_ready(h, false);
}

// one pair, a group of its own; sigmas already checked
int covariance_one(sicp_context* h, const double* qt, double sigma_source, double sigma_target, sicp_pose_covariance_result* out) {
  SICPCHECK(covariance_ready(h));
  SICPCHECK(search_at(h, qt));
  PoseCovScratch X;
  SweepOut o;
  SICPCHECK(pose_cov_sweep(h, X, h->pc_stage, &h, &qt, 1, h->stream, &o));
  HIPCHECK(hipStreamSynchronize(h->stream));
  X.idle = true;
  h->st.total_evals++;
  h->st.acc_launches += 1;
  PoseCovSums u;
  o.get(0, &u);
  fill_result(u, sigma_source, sigma_target, out);
  return SICP_OK;
}

// the slice of a job flush that takes searches of list length L: one slice per length (1, 4, 20, 32), so that pairs of
// different modes, knn and k_cov share one flush
int slice_of_list(int L) { return L <= 1 ? 0 : (L <= 4 ? 1 : (L <= 20 ? 2 : 3)); }

// One group of a batch call: pairs[0 .. m) index the call's arrays, distinct handles, all past covariance_ready.  Features
// that are not current, then the searches, each through ONE job flush on the first handle's stream; the sweep; one wait.
// status[i] of a pair that fails on the way is set; the others go on.  Returns the status of the shared part.
int covariance_group(sicp_handle* hs, const double* qt, const std::vector<int>& pairs, PoseCovScratch& X, double sigma_source,
                     double sigma_target, sicp_pose_covariance_result* out, std::vector<int>& status) {
  sicp_context* L = hs[pairs[0]];
  std::vector<sicp_context*> gh;
  for (int i : pairs) gh.push_back(hs[i]);
  JobCollector jc;
  std::vector<int> live;  // positions in `pairs` still on their way
  {
    BatchGuard guard(gh.data(), (int)gh.size(), &jc, L->stream);
    auto staged = [&](int k, int rc) {
      if (rc != SICP_OK) status[(size_t)pairs[(size_t)k]] = rc;
      return rc == SICP_OK;
    };
    auto features = [&](sicp_context* h) -> int {  // (search_at's first half)
      const sicp_params& P = h->params;
      const bool em = P.mode == SICP_MODE_EM;
      Cloud &S = h->cloud(0), &T = h->cloud(1);
      jc.slice = slice_of_list(sicp::nn_list_len(P.k_cov));
      SICPCHECK(prepare_cloud(h, S));
      SICPCHECK(prepare_cloud(h, T));
      if (!features_current(h, S, em)) SICPCHECK(compute_features(h, S, em));
      if (!features_current(h, T, em)) SICPCHECK(compute_features(h, T, em));
      if (em && !weights_from_histograms(P, P.knn)) {
        SICPCHECK(ensure_proj(h, S));
        SICPCHECK(ensure_proj(h, T));
      }
      return SICP_OK;
    };
    for (int k = 0; k < (int)pairs.size(); ++k)
      if (staged(k, features(gh[(size_t)k]))) live.push_back(k);
    int rc = flush_jobs(L, jc, L->stream);
    if (rc != SICP_OK) return rc;
    std::vector<int> searched;
    for (int k : live) {
      sicp_context* h = gh[(size_t)k];
      jc.slice = slice_of_list(sicp::nn_list_len(h->params.knn));
      if (staged(k, run_correspondences(h, qt + 7 * (size_t)pairs[(size_t)k], h->params.knn, true))) searched.push_back(k);
    }
    live.swap(searched);
    rc = flush_jobs(L, jc, L->stream);
    if (rc != SICP_OK) return rc;
  }
  if (live.empty()) return SICP_OK;
  std::vector<sicp_context*> sh;
  std::vector<const double*> sq;
  for (int k : live) { sh.push_back(gh[(size_t)k]); sq.push_back(qt + 7 * (size_t)pairs[(size_t)k]); }
  SweepOut o;
  sicp_context* h = L;
  SICPCHECK(pose_cov_sweep(L, X, L->pc_stage, sh.data(), sq.data(), (int)sh.size(), L->stream, &o));
  HIPCHECK(hipStreamSynchronize(L->stream));
  X.idle = true;
  for (size_t k = 0; k < live.size(); ++k) {
    sh[k]->st.total_evals++;
    sh[k]->st.acc_launches += 1;
    PoseCovSums u;
    o.get((int)k, &u);
    fill_result(u, sigma_source, sigma_target, &out[pairs[(size_t)live[k]]]);
  }
  return SICP_OK;
}

}  // namespace

int pose_covariance(sicp_context* h, const double* qt, double sigma_source, double sigma_target, sicp_pose_covariance_result* out) {
  if (!h || !qt || !out) return SICP_ERR_INVALID_ARGUMENT;
  if (!sigma_ok(sigma_source) || !sigma_ok(sigma_target)) {
    h->last_error = "sicp_pose_covariance: sigma_source and sigma_target must be finite and >= 0";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  return covariance_one(h, qt, sigma_source, sigma_target, out);
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
  // The pairs run in groups that share every launch.  A group is filled in the call's order from the pairs
  // still waiting, within its bounds (GroupBound), and holds a handle once -- its correspondence buffers are its own -- and
  // no pair that has to recompute the features of a cloud another pair of the group reads; a pair that does not fit waits
  // for a later group.  Every row has the bits of its lone call whatever group it lands in.
  constexpr int kUnset = 1;
  std::vector<int> st((size_t)n, kUnset);
  std::vector<int> waiting((size_t)n), later, pairs;
  for (int i = 0; i < n; ++i) waiting[(size_t)i] = i;
  PoseCovScratch X;
  while (!waiting.empty()) {
    GroupBound gb;
    std::unordered_set<const sicp_context*> handles;
    std::unordered_set<const Cloud*> clouds;
    pairs.clear(); later.clear();
    for (int i : waiting) {
      sicp_context* h = hs[i];
      if (handles.count(h)) { later.push_back(i); continue; }
      const int rc = covariance_ready(h);
      if (rc != SICP_OK) { st[(size_t)i] = rc; continue; }
      const bool em = h->params.mode == SICP_MODE_EM;
      const Cloud *S = &h->cloud(0), *T = &h->cloud(1);
      const long long total = (long long)S->n * h->params.knn;
      const bool rewrites = (!features_current(h, *S, em) && clouds.count(S)) || (!features_current(h, *T, em) && clouds.count(T));
      if (rewrites || !gb.admits(total, T->n)) { later.push_back(i); continue; }
      gb.add(total, T->n);
      handles.insert(h); clouds.insert(S); clouds.insert(T);
      pairs.push_back(i);
    }
    waiting.swap(later);
    if (pairs.empty()) continue;
    int rc;
    try {
      rc = covariance_group(hs, qt, pairs, X, sigma_source, sigma_target, out, st);
    } catch (const std::bad_alloc&) {
      rc = SICP_ERR_OUT_OF_MEMORY;
    }
    for (int i : pairs) {
      if (st[(size_t)i] != kUnset) continue;  // (failed on its own, on the way)
      st[(size_t)i] = rc;
      if (rc != SICP_OK && hs[i] != hs[pairs[0]]) hs[i]->last_error = hs[pairs[0]]->last_error;  // (the group's leader holds the text)
    }
  }
  int first = SICP_OK;
  for (int i = 0; i < n; ++i) {
    const int s = st[(size_t)i];
    if (s != SICP_OK) {
      hs[i]->last_error = "sicp_pose_covariance_batch: pair " + std::to_string(i) + ": " + hs[i]->last_error;
      if (first == SICP_OK) {
        first = s;
        if (h0 != hs[i]) h0->last_error = hs[i]->last_error;
      }
    }
    if (status) status[i] = s;
  }
  return first;
}

// ---- a stream's covariance pass (streams.cpp) -----------------------------------------------------------------------------
// The scratch belongs to the stream: reserved with the first flagged registration, kept across turns, released with the
// stream.  A pass's arguments and results travel through a pinned stage of its own; a stage is used again only when every
// slot of its pass has taken its sums (so the copy engine has long left it).
struct PoseCovStage {
  HostBuf<unsigned char> pin;
  SweepOut o;
  OwnedEvent ev;
  int waiting = 0;  // slots that have not taken their sums yet
};
struct PoseCovStream {
  PoseCovScratch X;
  std::vector<std::unique_ptr<PoseCovStage>> stages;
};

int stream_cov_pass(sicp_stream_ctx* S, const std::vector<int>& slots, const std::vector<const double*>& qts, hipStream_t side) {
  sicp_context* h = S->slots[0];
  if (!S->cov) S->cov = new PoseCovStream();
  PoseCovStream& C = *S->cov;
  for (size_t b = 0; b < slots.size();) {  // (a pass beyond a group's bounds runs as several sweeps, one behind the other)
    GroupBound gb;
    size_t e = b;
    for (; e < slots.size(); ++e) {
      sicp_context* g = S->slots[(size_t)slots[e]];
      const long long total = (long long)g->corr_n * g->corr_K;
      if (!gb.admits(total, g->cloud(1).n)) break;
      gb.add(total, g->cloud(1).n);
    }
    int si = -1;
    for (size_t k = 0; k < C.stages.size() && si < 0; ++k)
      if (C.stages[k]->waiting == 0) si = (int)k;
    if (si < 0) { C.stages.emplace_back(new PoseCovStage()); si = (int)C.stages.size() - 1; }
    PoseCovStage& G = *C.stages[(size_t)si];
    HIPCHECK(G.ev.create());
    std::vector<sicp_context*> gh;
    for (size_t k = b; k < e; ++k) gh.push_back(S->slots[(size_t)slots[k]]);
    SICPCHECK(pose_cov_sweep(h, C.X, G.pin, gh.data(), qts.data() + b, (int)(e - b), side, &G.o));
    HIPCHECK(hipEventRecord(G.ev, side));
    G.waiting = (int)(e - b);
    for (size_t k = b; k < e; ++k) { S->slot_cov_stage[(size_t)slots[k]] = si; S->slot_cov_row[(size_t)slots[k]] = (int)(k - b); }
    b = e;
  }
  return SICP_OK;
}

hipEvent_t stream_cov_event(sicp_stream_ctx* S, int slot) { return S->cov->stages[(size_t)S->slot_cov_stage[(size_t)slot]]->ev; }

void stream_cov_take(sicp_stream_ctx* S, int slot, PoseCovSums* out) {
  PoseCovStage& G = *S->cov->stages[(size_t)S->slot_cov_stage[(size_t)slot]];
  G.o.get(S->slot_cov_row[(size_t)slot], out);
  --G.waiting;
}

void stream_cov_destroy(sicp_stream_ctx* S, bool idle) {
  if (!S->cov) return;
  S->cov->X.idle = idle;
  delete S->cov;
  S->cov = nullptr;
}

int pose_covariance_from_sums(const PoseCovSums& u, double sigma_source, double sigma_target, sicp_pose_covariance_result* out) {
  if (!out || !sigma_ok(sigma_source) || !sigma_ok(sigma_target)) return SICP_ERR_INVALID_ARGUMENT;
  fill_result(u, sigma_source, sigma_target, out);
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
