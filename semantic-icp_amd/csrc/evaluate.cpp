// evaluate.cpp -- sicp_evaluate / sicp_evaluate_batch (include/sicp.h): per pair one K = 1 search of all source points per
// target segment into the handle's evaluate scratch, then ONE sweep for a whole group of pairs -- the job-table kernels of
// evaluate_kernels.hip, one read-back -- and the three ratios on the host.  A lone call is a group of one pair.  Nothing a
// handle holds for align() is touched: not its correspondences, not its statistics.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

bool gate_ok(double g) { return g > 0.0; }  // (NaN fails; +inf passes: every query is an inlier)
bool classes_ok(int32_t C) { return C >= 1 && C <= 255; }

// What bounds a group: the pairs one job table holds, its workgroups, and the result block it reads back (the tables: 8 C^2 bytes
// per pair).  The searches' scratch is the handles' own.
constexpr int kGroupPairs = 256;
constexpr long long kGroupBlocks = 1ll << 30;
constexpr size_t kGroupResultBytes = (size_t)64 << 20;

// A sweep's device scratch: it lives for the call, shared by its groups, and goes back to the arena at the end
// (DevArena::release_scratch: `idle` once the stream has been synchronised behind the sweep).
struct EvalScratch {
  DevBuf<unsigned char> args, res;
  DevBuf<double> part_sum;
  DevBuf<int> part_cnt, nn_idx;
  DevBuf<float> nn_d2;
  int device = -1;
  bool idle = true;
  ~EvalScratch() { DevArena::release_scratch(device, idle, args, res, part_sum, part_cnt, nn_idx, nn_d2); }
};

// what a pair must pass before anything is queued for it
int evaluate_ready(sicp_context* h, bool table) {
  const Cloud &S = h->cloud(0), &T = h->cloud(1);
  if (!S.is_set || !T.is_set) return SICP_ERR_NOT_READY;
  if (table && (!S.has_label || !T.has_label)) {
    h->last_error = "sicp_evaluate: a confusion table was asked for and a cloud was set without labels";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  if (h->params.mode == SICP_MODE_SEMANTIC && (!S.has_label || !T.has_label)) return SICP_ERR_NOT_READY;
  if (T.n < 1) return SICP_ERR_TOO_FEW_POINTS;
  return SICP_OK;
}

// the pair's searches at qt: all source points against every target segment, K = 1, into ev_idx / ev_d2 [n_seg][n_s]; launched
// on the handle's stream, or collected when the handle has a job list
int evaluate_search(sicp_context* h, const double* qt, float gate) {
  Cloud &S = h->cloud(0), &T = h->cloud(1);
  SICPCHECK(prepare_cloud(h, S));
  SICPCHECK(prepare_cloud(h, T));
  const size_t slots = (size_t)(S.n > 0 ? S.n : 1) * (size_t)T.n_seg();
  if ((long long)S.n * T.n_seg() > 0x7fffffffll) return SICP_ERR_INVALID_ARGUMENT;
  HIPCHECK(h->ev_idx.reserve(slots));
  HIPCHECK(h->ev_d2.reserve(slots));
  double M[12];
  matrix34(qt, M);
  for (int ts = 0; ts < T.n_seg(); ++ts)
    SICPCHECK(run_nn(h, 1, S, 0, S.n, M, T, ts, false, gate, h->ev_idx.p + (size_t)ts * S.n, h->ev_d2.p + (size_t)ts * S.n,
                     SICP_PROFILE_NN, h->stream));
  return SICP_OK;
}

// where a sweep's results arrive (pinned, valid once the stream has passed the read-back): pair i is row i
struct SweepOut {
  const sicp::EvalOut* out = nullptr;
  const long long* conf = nullptr;  // [n][C][C] when tables were asked for
};

// The sweep of a group: n pairs (distinct handles, one device) whose searches are complete or queued on `st`.  Everything is
// queued on `st`, nothing is waited for: the job table's upload, the tables' zeros, the two kernels, one read-back into `pin`.
// per_point (n = 1 only): the caller-order winners go to X.nn_idx / X.nn_d2.  `h` leads: it takes the error text.
int evaluate_sweep(sicp_context* h, EvalScratch& X, HostBuf<unsigned char>& pin, sicp_context* const* hs, int n, float gate, int C,
                   bool table, bool per_point, hipStream_t st, SweepOut* o) {
  if (n < 1 || n > kGroupPairs || (per_point && n != 1)) return SICP_ERR_INTERNAL;
  size_t chunks_all = 0;
  long long blocks_all = 0;
  for (int k = 0; k < n; ++k) {
    chunks_all += (size_t)sicp::eval_chunks(hs[k]->cloud(0).n);
    blocks_all += sicp::eval_blocks(hs[k]->cloud(0).n);
  }
  if (blocks_all > kGroupBlocks) return SICP_ERR_INTERNAL;
  const size_t cc = table ? (size_t)C * C : 0;
  // the results: a row per pair | the tables; in `pin` they lie behind the job table
  sicp::ArgBlock res_block;
  const sicp::ArgBlock::Section s_out = res_block.add<sicp::EvalOut>((size_t)n), s_conf = res_block.add<unsigned long long>(cc * (size_t)n);
  const size_t res_bytes = res_block.bytes();
  HIPCHECK(X.res.reserve(res_bytes));
  HIPCHECK(X.part_sum.reserve(std::max<size_t>(chunks_all, 1)));
  HIPCHECK(X.part_cnt.reserve(std::max<size_t>(chunks_all, 1) * 4));
  if (per_point) {
    HIPCHECK(X.nn_idx.reserve((size_t)std::max(hs[0]->cloud(0).n, 1)));
    HIPCHECK(X.nn_d2.reserve((size_t)std::max(hs[0]->cloud(0).n, 1)));
  }
  sicp::EvalOut* d_out = sicp::ArgBlock::dev<sicp::EvalOut>(s_out, X.res.p);
  unsigned long long* d_conf = sicp::ArgBlock::dev<unsigned long long>(s_conf, X.res.p);
  X.device = h->device;
  X.idle = false;
  sicp::JobTable<sicp::EvalJob> tab;  // (a pair without source points keeps its row: the finalize goes by position)
  size_t chunk_off = 0;
  for (int k = 0; k < n; ++k) {
    sicp_context* g = hs[k];
    const Cloud &S = g->cloud(0), &T = g->cloud(1);
    const bool labels = S.has_label && T.has_label;
    sicp::EvalJob J;
    std::memset(&J, 0, sizeof J);
    J.n_s = S.n; J.n_seg = T.n_seg();
    J.idx = g->ev_idx.p; J.d2 = g->ev_d2.p;
    J.slabel = labels ? S.label.p : nullptr; J.tlabel = labels ? T.label.p : nullptr;
    J.sperm = S.d_perm.p; J.tperm = T.d_perm.p;
    J.gate_sq = gate;
    J.C = table ? C : 0;
    J.conf = table ? d_conf + cc * (size_t)k : nullptr;
    J.nn_idx = per_point ? X.nn_idx.p : nullptr;
    J.nn_d2 = per_point ? X.nn_d2.p : nullptr;
    J.part_sum = X.part_sum.p + chunk_off;
    J.part_cnt = X.part_cnt.p + chunk_off * 4;
    J.out = d_out + k;
    chunk_off += (size_t)sicp::eval_chunks(S.n);
    tab.add(J, sicp::eval_blocks(S.n));
  }
  const size_t arg_bytes = tab.bytes();
  HIPCHECK(X.args.reserve(arg_bytes));
  HIPCHECK(pin.resize(arg_bytes + res_bytes));
  tab.pack(pin.data(), X.args.p);
  HIPCHECK(hipMemcpyAsync(X.args.p, pin.data(), arg_bytes, hipMemcpyHostToDevice, st));
  if (cc) HIPCHECK(hipMemsetAsync(d_conf, 0, sizeof(long long) * cc * (size_t)n, st));
  HIPCHECK(sicp::launch_evaluate_jobs(tab.d_jobs(), tab.d_end(), n, tab.blocks, st));
  HIPCHECK(sicp::launch_evaluate_finalize_jobs(tab.d_jobs(), n, st));
  unsigned char* res = pin.data() + arg_bytes;
  HIPCHECK(hipMemcpyAsync(res, X.res.p, res_bytes, hipMemcpyDeviceToHost, st));
  o->out = sicp::ArgBlock::host<const sicp::EvalOut>(s_out, res);
  o->conf = sicp::ArgBlock::host<const long long>(s_conf, res);
  return SICP_OK;
}

// the caller's result from a pair's sums
void fill_result(const sicp::EvalOut& u, int n_source, sicp_evaluate_result* out) {
  sicp_evaluate_result r;
  std::memset(&r, 0, sizeof r);
  r.n_source = n_source;
  r.inliers = u.inliers;
  r.label_agree = u.label_agree;
  r.label_outside = u.label_outside;
  r.sum_d2 = u.sum_d2;
  r.fitness = n_source > 0 ? (double)u.inliers / (double)n_source : 0.0;
  r.inlier_rmse = u.inliers > 0 ? std::sqrt(u.sum_d2 / (double)u.inliers) : std::numeric_limits<double>::quiet_NaN();
  *out = r;
}

// one pair, a group of its own; arguments already checked
int evaluate_one(sicp_context* h, const double* qt, float gate, int C, int64_t* confusion, int32_t* nn_idx, float* nn_d2,
                 sicp_evaluate_result* out) {
  const bool table = confusion != nullptr, per_point = nn_idx != nullptr || nn_d2 != nullptr;
  SICPCHECK(evaluate_ready(h, table));
  SICPCHECK(set_device(h));
  StatsKeeper keep(h);
  SICPCHECK(evaluate_search(h, qt, gate));
  Cloud &S = h->cloud(0), &T = h->cloud(1);
  EvalScratch X;
  SweepOut o;
  SICPCHECK(evaluate_sweep(h, X, h->ev_stage, &h, 1, gate, C, table, per_point, h->stream, &o));
  const int n = S.n;
  const bool direct = S.drop_i.empty() && T.keep.empty();  // no point of either cloud was dropped: the kernel's indices are the caller's
  std::vector<int> ti;
  std::vector<float> td;
  if (per_point && n > 0) {
    if (!direct) { ti.resize((size_t)n); td.resize((size_t)n); }
    if (nn_idx) HIPCHECK(hipMemcpyAsync(direct ? nn_idx : ti.data(), X.nn_idx.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (nn_d2) HIPCHECK(hipMemcpyAsync(direct ? nn_d2 : td.data(), X.nn_d2.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHECK(hipStreamSynchronize(h->stream));
  X.idle = true;
  if (per_point && !direct) {
    for (int i : S.drop_i) {  // a non-finite source point has no neighbour (sicp_cloud_size)
      if (nn_idx) nn_idx[i] = -1;
      if (nn_d2) nn_d2[i] = std::numeric_limits<float>::quiet_NaN();
    }
    for (int i = 0; i < n; ++i) {
      const int c = S.keep.empty() ? i : S.keep[(size_t)i];
      if (nn_idx) nn_idx[c] = ti[(size_t)i] < 0 ? -1 : (T.keep.empty() ? ti[(size_t)i] : T.keep[(size_t)ti[(size_t)i]]);
      if (nn_d2) nn_d2[c] = td[(size_t)i];
    }
  }
  if (table) std::memcpy(confusion, o.conf, sizeof(int64_t) * (size_t)C * C);
  fill_result(o.out[0], n, out);
  return SICP_OK;
}

// One group of a batch call: pairs[0 .. m) index the call's arrays, distinct handles, all past evaluate_ready.  The searches of
// all pairs through ONE job flush on the first handle's stream; the sweep; one read-back, one wait.  status[i] of a pair that
// fails on the way is set; the others go on.  Returns the status of the shared part.
int evaluate_group(sicp_handle* hs, const double* qt, const std::vector<int>& pairs, EvalScratch& X, float gate, int C, int64_t* confusion,
                   sicp_evaluate_result* out, std::vector<int>& status) {
  sicp_context* L = hs[pairs[0]];
  sicp_context* h = L;  // (HIPCHECK reports into the leader)
  std::vector<sicp_context*> gh;
  for (int i : pairs) gh.push_back(hs[i]);
  std::vector<StatsKeeper> keep;
  keep.reserve(gh.size());
  for (sicp_context* g : gh) keep.emplace_back(g);
  std::vector<int> live;  // positions in `pairs` whose searches are queued
  {
    JobCollector jc;
    BatchGuard guard(gh.data(), (int)gh.size(), &jc, L->stream);
    jc.slice = 0;
    for (int k = 0; k < (int)pairs.size(); ++k) {
      const int rc = evaluate_search(gh[(size_t)k], qt + 7 * (size_t)pairs[(size_t)k], gate);
      if (rc != SICP_OK) status[(size_t)pairs[(size_t)k]] = rc; else live.push_back(k);
    }
    SICPCHECK(flush_jobs(L, jc, L->stream));
  }
  if (live.empty()) return SICP_OK;
  std::vector<sicp_context*> sh;
  for (int k : live) sh.push_back(gh[(size_t)k]);
  SweepOut o;
  SICPCHECK(evaluate_sweep(L, X, L->ev_stage, sh.data(), (int)sh.size(), gate, C, confusion != nullptr, false, L->stream, &o));
  HIPCHECK(hipStreamSynchronize(L->stream));
  X.idle = true;
  const size_t cc = (size_t)C * C;
  for (size_t k = 0; k < live.size(); ++k) {
    const int i = pairs[(size_t)live[k]];
    if (confusion) std::memcpy(confusion + cc * (size_t)i, o.conf + cc * k, sizeof(int64_t) * cc);
    fill_result(o.out[k], sh[k]->cloud(0).n, &out[i]);
  }
  return SICP_OK;
}

}  // namespace

int evaluate(sicp_context* h, const double* qt, double max_dist_sq, int32_t num_classes, int64_t* confusion, int32_t* nn_idx,
             float* nn_d2, sicp_evaluate_result* out) {
  if (!h || !qt || !out) return SICP_ERR_INVALID_ARGUMENT;
  if (!gate_ok(max_dist_sq)) {
    h->last_error = "sicp_evaluate: max_dist_sq must be > 0 (+inf is allowed)";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  if (confusion && !classes_ok(num_classes)) {
    h->last_error = "sicp_evaluate: a confusion table needs num_classes in 1..255";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  return evaluate_one(h, qt, (float)max_dist_sq, confusion ? num_classes : 0, confusion, nn_idx, nn_d2, out);
}

int evaluate_batch(sicp_handle* hs, int32_t n, const double* qt, double max_dist_sq, int32_t num_classes, int64_t* confusion,
                   sicp_evaluate_result* out, int32_t* status) {
  if (!hs || n < 1) return SICP_ERR_INVALID_ARGUMENT;
  sicp_context* h0 = hs[0];
  auto refuse = [&](const std::string& why) {
    if (h0) h0->last_error = "sicp_evaluate_batch: " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  for (int i = 0; i < n; ++i)
    if (!hs[i]) return refuse("handle " + std::to_string(i) + " is NULL");
  if (!qt) return refuse("qt is NULL");
  if (!out) return refuse("out is NULL");
  if (!gate_ok(max_dist_sq)) return refuse("max_dist_sq must be > 0 (+inf is allowed)");
  if (confusion && !classes_ok(num_classes)) return refuse("a confusion table needs num_classes in 1..255");
  for (int i = 1; i < n; ++i)
    if (hs[i]->device != h0->device)
      return refuse("handle " + std::to_string(i) + " is on device " + std::to_string(hs[i]->device) + ", handle 0 on " + std::to_string(h0->device));
  const float gate = (float)max_dist_sq;
  const int C = confusion ? num_classes : 0;
  const size_t pair_res = sizeof(sicp::EvalOut) + sizeof(long long) * (size_t)C * C;
  // The pairs run in groups that share every launch.  A group is filled in the call's order from the pairs still waiting,
  // within its bounds, and holds a handle once -- its search scratch is its own -- and no pair that would lay a cloud out
  // anew (a handle of another mode shares it) while another pair of the group searches it; a pair that does not fit waits
  // for a later group.  Every row has the bits of its lone call whatever group it lands in.
  constexpr int kUnset = 1;
  std::vector<int> st((size_t)n, kUnset);
  std::vector<int> waiting((size_t)n), later, pairs;
  for (int i = 0; i < n; ++i) waiting[(size_t)i] = i;
  if (hipSetDevice(h0->device) != hipSuccess) return refuse("its device cannot be selected");
  EvalScratch X;
  while (!waiting.empty()) {
    std::unordered_set<const sicp_context*> handles;
    std::unordered_map<const Cloud*, int> layouts;
    long long blocks = 0;
    pairs.clear(); later.clear();
    for (int i : waiting) {
      sicp_context* h = hs[i];
      if (handles.count(h)) { later.push_back(i); continue; }
      const int rc = evaluate_ready(h, confusion != nullptr);
      if (rc != SICP_OK) { st[(size_t)i] = rc; continue; }
      const int want = h->params.mode == SICP_MODE_SEMANTIC ? 1 : 0;
      const Cloud *S = &h->cloud(0), *T = &h->cloud(1);
      auto clash = [&](const Cloud* c) {
        auto it = layouts.find(c);
        return it != layouts.end() && it->second != want;
      };
      const long long b = sicp::eval_blocks(S->n);
      const bool full = !pairs.empty() && ((int)pairs.size() + 1 > kGroupPairs || blocks + b > kGroupBlocks ||
                                           (pairs.size() + 1) * pair_res > kGroupResultBytes);
      if (clash(S) || clash(T) || full) { later.push_back(i); continue; }
      blocks += b;
      handles.insert(h); layouts[S] = want; layouts[T] = want;
      pairs.push_back(i);
    }
    waiting.swap(later);
    if (pairs.empty()) continue;
    int rc;
    try {
      rc = evaluate_group(hs, qt, pairs, X, gate, C, confusion, out, st);
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
      hs[i]->last_error = "sicp_evaluate_batch: pair " + std::to_string(i) + ": " + hs[i]->last_error;
      if (first == SICP_OK) {
        first = s;
        if (h0 != hs[i]) h0->last_error = hs[i]->last_error;
      }
    }
    if (status) status[i] = s;
  }
  return first;
}

}  // namespace host
}  // namespace sicp
