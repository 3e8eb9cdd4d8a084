// bootstrap.cpp -- the stage driver of the initial alignment without a pose prior (exec/bootstrap.h, class Bootstrap):
// box filter + VoxelGrid keypoints, radius neighbourhoods, normals and FPFH features of both clouds on the device, then
// SampleConsensusInitialAlignment: the hypotheses are drawn on the host from a documented PRNG (splitmix64), their rigid
// transforms solved on the host in f64, and all of them are scored on the device at once -- one K = 1 box-tree search per
// hypothesis over a tree of the target keypoints, collected into the packet kernel's job launches, then one
// truncated-error reduction.  Orders and precisions: INTEGRATION.md ("Bootstrap").
//
// Every call is a batch of pairs (sicp_bootstrap = a batch of one): each stage runs over all clouds / pairs of a group at
// once -- the hot kernels as one job launch (kernels.h: BootCloudJob / BootPairJob), the rocPRIM sorts and scans queued
// cloud after cloud -- with one host synchronisation per stage for the whole group.  A cloud shared by several pairs
// (sicp_share_cloud) gets its keypoints and features once per call.
//
// The label forms (sicp_bootstrap_semantic*) run the same stages with a sicp_bootstrap_label_params (`lp`, NULL in the
// label-blind calls): the ignore list joins the box filter, every keypoint gets its voxel's label vote, and the two flags
// choose the label forms of the feature k-NN and of the error kernel.
#include <map>
#include <set>
#include <thread>

#include "bootstrap.hpp"

namespace sicp {
namespace host {

namespace {

typedef unsigned long long u64;

// pairs and new cloud points per group: what bounds the scratch of a call whatever its number of pairs
constexpr int kGroupPairs = 64;
constexpr long long kGroupPoints = 16ll << 20;
// search outputs (one per source keypoint and hypothesis) in flight per scoring chunk
constexpr long long kScoreOutputs = 32ll << 20;
// host threads drawing the hypotheses of a group's pairs (a GPU host command gets 16 CPUs: never sized by the machine)
constexpr int kGenThreads = 8;

// the keypoints of one cloud and their features, device-resident (keypoint order)
struct BootCloud {
  int n = 0;
  std::vector<float> hx, hy, hz;  // host copy of the keypoints (sampling distances, the search tree's staging)
  DevBuf<float> kx, ky, kz;
  // the keypoints' labels (the label forms only)
  std::vector<uint32_t> hl;
  DevBuf<uint32_t> kl;
  // neighbourhoods of the feature radius (CSR); those of the normal radius when the two radii differ live in nrm_*
  long long n_nbrs = 0;
  int max_nbrs = 0;
  DevBuf<long long> off;
  DevBuf<int> idx;
  DevBuf<float> d2;
  DevBuf<double> n3;
  DevBuf<float> fpfh;
};

// every scratch buffer of one cloud (arena blocks: recycled between calls)
struct BootScratch {
  DevBuf<float> x, y, z, blk;
  DevBuf<uint32_t> lab;  // the points' labels (the label forms only)
  DevBuf<u64> key, key2;
  DevBuf<int> flag, pos, heads, nout, val, val2;
  DevBuf<long long> cnt;
  DevBuf<unsigned char> temp;
  DevBuf<double> spfh;
  DevBuf<u64> list, list2;
  // the normal radius' own lists (normal_radius != feature_radius)
  DevBuf<long long> noff;
  DevBuf<int> nidx;
  DevBuf<float> nd2;
};

// one distinct cloud of a call: its keypoints, features and what the stages hand each other
struct CloudWork {
  const Cloud* c = nullptr;
  int status = SICP_OK;
  std::string msg;  // why status != SICP_OK (without the entry point's name)
  BootCloud k;
  BootScratch s;
  std::vector<char> valid;      // keypoints with a feature
  std::shared_ptr<Cloud> tree;  // the keypoints as an engine cloud: query set and search tree of the scoring
  // stage hand-over
  std::vector<float> blk;
  long long n_kept = 0;
  int n_kp = 0;
  size_t scan_bytes = 0;
  std::vector<long long> cnt;
  long long total = 0;
  std::vector<double> n3;
  bool live() const { return status == SICP_OK; }
  void fail(int st, std::string why) { status = st; msg = std::move(why); }
};

// one pair of a call
struct PairWork {
  int index = 0;
  CloudWork *S = nullptr, *T = nullptr;
  int status = SICP_OK;
  bool done = false;  // its pose and info are written
  std::string msg;
  std::vector<int> knn;  // [n_source][k]
  int k_eff = 0;         // k clamped to the target keypoints with a feature
  std::vector<int> row_k;  // match_same_label: the entries >= 0 of every row of knn (empty otherwise: k_eff for every row)
  std::vector<int> src_valid;  // the source keypoints that can be sampled
  int tgt_valid = 0;
  int n_hyp = 0;
  std::vector<double> M, Q, err;  // [n_hyp][12], [n_hyp][4], [n_hyp]
  size_t knn_at = 0, err_at = 0;  // places in the stage buffers
};

// one launch's job table with its two copies: the device block, and the host bytes (pageable) that stay alive with the
// table -- a table lives until its stage synchronises.  (Callers skip empty clouds and pairs themselves: a job added with
// zero blocks would be kept in the table.)
template <class J>
struct BootTable : sicp::JobTable<J> {
  std::vector<unsigned char> host;
  DevBuf<unsigned char> dev;
  hipError_t upload(hipStream_t st) {
    if (this->nj() == 0) return hipSuccess;
    host.resize(this->bytes());
    hipError_t e = dev.reserve(host.size());
    if (e != hipSuccess) return e;
    this->pack(host.data(), dev.p);
    return hipMemcpyAsync(dev.p, host.data(), host.size(), hipMemcpyHostToDevice, st);
  }
};

int temp_reserve(sicp_context* h, BootScratch& s, size_t bytes) {
  HIPCHECK(s.temp.reserve(bytes + 256));
  return SICP_OK;
}

int check_params(sicp_context* h, const sicp_bootstrap_params& p, const char* who) {
  auto bad = [&](const char* what) {
    h->last_error = std::string(who) + ": " + what;
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (std::isnan(p.box_max)) return bad("box_max is NaN");
  if (!(p.leaf_size > 0) || !std::isfinite(p.leaf_size) || !std::isfinite(1.0f / (float)p.leaf_size)) return bad("leaf_size must be positive and finite");
  if (!(p.normal_radius > 0) || !std::isfinite(p.normal_radius)) return bad("normal_radius must be positive and finite");
  if (!(p.feature_radius > 0) || !std::isfinite(p.feature_radius)) return bad("feature_radius must be positive and finite");
  if (!(p.min_sample_distance >= 0) || !std::isfinite(p.min_sample_distance)) return bad("min_sample_distance must be >= 0 and finite");
  if (!(p.max_corr_distance > 0) || !std::isfinite(p.max_corr_distance)) return bad("max_corr_distance must be positive and finite");
  if (p.max_iterations < 1) return bad("max_iterations must be >= 1");
  if (p.nr_samples < 3 || p.nr_samples > kBootMaxSamples) return bad("nr_samples must be in 3..8");
  if (p.k_correspondences < 1 || p.k_correspondences > kBootMaxK) return bad("k_correspondences must be in 1..16");
  return SICP_OK;
}

int check_label_params(sicp_context* h, const sicp_bootstrap_label_params& lp, const char* who) {
  auto bad = [&](const char* what) {
    h->last_error = std::string(who) + ": " + what;
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (lp.match_same_label != 0 && lp.match_same_label != 1) return bad("match_same_label must be 0 or 1");
  if (lp.score_same_label != 0 && lp.score_same_label != 1) return bad("score_same_label must be 0 or 1");
  if (lp.n_ignore < 0 || lp.n_ignore > SICP_BOOTSTRAP_MAX_IGNORE) return bad("n_ignore must be in 0..64");
  return SICP_OK;
}

sicp::BootIgnore ignore_of(const sicp_bootstrap_label_params& lp) {
  static_assert(sicp::kBootMaxIgnore == SICP_BOOTSTRAP_MAX_IGNORE, "the kernel argument holds the whole ignore list");
  sicp::BootIgnore ig;
  std::memset(&ig, 0, sizeof ig);
  ig.n = lp.n_ignore;
  for (int k = 0; k < lp.n_ignore; ++k) ig.v[k] = lp.ignore[k];
  return ig;
}

// the engine's searches run on flat clouds with the box tree whatever the handle's mode / engine knobs: they are restored after
struct BootParamsScope {
  sicp_context* h;
  sicp_params saved;
  explicit BootParamsScope(sicp_context* ctx) : h(ctx), saved(ctx->params) {
    h->params.mode = SICP_MODE_GICP;
    h->params.nn_method = 1;
    h->params.profile = 0;
  }
  ~BootParamsScope() { h->params = saved; }
};
struct CollectScope {
  sicp_context* h;
  CollectScope(sicp_context* ctx, JobCollector* jc) : h(ctx) { h->collect = jc; }
  ~CollectScope() { h->collect = nullptr; }
};

// Horn's closed form (the rotation of the largest eigenvector of the 4x4 matrix of the cross-covariance): the rigid
// transform without scale that Umeyama's SVD gives with its reflection fix.  f64; q = (w, x, y, z), w >= 0.
void rigid_from_pairs(int n, const double* s, const double* t, double q[4], double M[12]) {
  double cs[3] = {0, 0, 0}, ct[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int d = 0; d < 3; ++d) { cs[d] += s[3 * i + d]; ct[d] += t[3 * i + d]; }
  for (int d = 0; d < 3; ++d) { cs[d] /= n; ct[d] /= n; }
  double S[3][3] = {};
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) S[a][b] += (s[3 * i + a] - cs[a]) * (t[3 * i + b] - ct[b]);
  double N[4][4] = {
      {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
      {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
      {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
      {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 50; ++sweep) {  // cyclic Jacobi
    double off = 0, dia = 0;
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) (a == b ? dia : off) += N[a][b] * N[a][b];
    if (off <= 1e-300 || off <= 1e-34 * dia) break;
    for (int pp = 0; pp < 3; ++pp)
      for (int qq = pp + 1; qq < 4; ++qq) {
        const double apq = N[pp][qq];
        if (apq == 0.0) continue;
        const double tau = (N[qq][qq] - N[pp][pp]) / (2.0 * apq);
        const double tt = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double c = 1.0 / std::sqrt(1.0 + tt * tt), sn = tt * c;
        for (int k = 0; k < 4; ++k) {
          const double akp = N[k][pp], akq = N[k][qq];
          N[k][pp] = c * akp - sn * akq; N[k][qq] = sn * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = N[pp][k], aqk = N[qq][k];
          N[pp][k] = c * apk - sn * aqk; N[qq][k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][pp], vkq = V[k][qq];
          V[k][pp] = c * vkp - sn * vkq; V[k][qq] = sn * vkp + c * vkq;
        }
      }
  }
  int col = 0;
  for (int a = 1; a < 4; ++a)
    if (N[a][a] > N[col][col]) col = a;
  double w = V[0][col], x = V[1][col], y = V[2][col], z = V[3][col];
  const double nrm = std::sqrt(w * w + x * x + y * y + z * z);
  const double sg = w < 0 ? -1.0 : 1.0;
  w *= sg / nrm; x *= sg / nrm; y *= sg / nrm; z *= sg / nrm;
  q[0] = w; q[1] = x; q[2] = y; q[3] = z;
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                       2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  for (int r = 0; r < 3; ++r) {
    M[4 * r + 0] = R[3 * r + 0]; M[4 * r + 1] = R[3 * r + 1]; M[4 * r + 2] = R[3 * r + 2];
    M[4 * r + 3] = ct[r] - (R[3 * r + 0] * cs[0] + R[3 * r + 1] * cs[1] + R[3 * r + 2] * cs[2]);
  }
}

// box filter + voxel grid of every cloud: keypoints = centroids of the occupied voxels in ascending voxel index.  Three
// synchronisations for all clouds: the bounds, the keypoint counts, the keypoints' host copies.
int voxel_stage(sicp_context* h, const sicp_bootstrap_params& p, const sicp_bootstrap_label_params* lp,
                const std::vector<CloudWork*>& W) {
  const hipStream_t st = h->stream;
  const bool ignoring = lp && lp->n_ignore > 0;
  const sicp::BootIgnore ig_list = lp ? ignore_of(*lp) : sicp::BootIgnore();
  const sicp::BootIgnore* ig = ignoring ? &ig_list : nullptr;  // (without a list: the label-blind kernels)
  for (CloudWork* w : W) {
    const Cloud& c = *w->c;
    const int n = c.n;
    w->k.n = 0;
    w->n_kept = 0;
    if (n <= 0) continue;
    if (c.hx.size() < (size_t)n) { w->fail(SICP_ERR_NOT_READY, "a cloud has no host copy"); continue; }
    if (lp && (!c.has_label || c.hl.size() < (size_t)n)) { w->fail(SICP_ERR_INVALID_ARGUMENT, "a cloud has no labels"); continue; }
    BootScratch& s = w->s;
    if (lp) {
      HIPCHECK(s.lab.reserve(n));
      HIPCHECK(hipMemcpyAsync(s.lab.p, c.hl.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
    }
    HIPCHECK(s.x.reserve(n)); HIPCHECK(s.y.reserve(n)); HIPCHECK(s.z.reserve(n));
    HIPCHECK(hipMemcpyAsync(s.x.p, c.hx.data(), sizeof(float) * n, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(s.y.p, c.hy.data(), sizeof(float) * n, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(s.z.p, c.hz.data(), sizeof(float) * n, hipMemcpyHostToDevice, st));
    const int nb = boot_bounds_blocks(n);
    HIPCHECK(s.blk.reserve((size_t)nb * 8));
    HIPCHECK(launch_boot_bounds(n, s.x.p, s.y.p, s.z.p, s.lab.p, ig, p.box_max, s.blk.p, st));
    w->blk.assign((size_t)nb * 8, 0.f);
    HIPCHECK(hipMemcpyAsync(w->blk.data(), s.blk.p, sizeof(float) * w->blk.size(), hipMemcpyDeviceToHost, st));
  }
  HIPCHECK(hipStreamSynchronize(st));
  const float inv_leaf = 1.0f / (float)p.leaf_size;
  for (CloudWork* w : W) {
    if (!w->live() || w->c->n <= 0) continue;
    const int n = w->c->n;
    const int nb = boot_bounds_blocks(n);
    const float inf = std::numeric_limits<float>::infinity();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    long long n_kept = 0;
    for (int b = 0; b < nb; ++b) {
      for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], w->blk[b * 8 + d]); hi[d] = std::max(hi[d], w->blk[b * 8 + 3 + d]); }
      n_kept += (long long)w->blk[b * 8 + 6];
    }
    if (n_kept == 0) continue;
    // PCL VoxelGrid::applyFilter: min_b / max_b = floor(min_p / max_p * (1 / leaf)) in f32
    int min_b[3];
    long long div[3];
    bool beyond = false;
    for (int d = 0; d < 3; ++d) {
      const float a = std::floor(lo[d] * inv_leaf), b = std::floor(hi[d] * inv_leaf);
      if (!(std::fabs(a) < 1073741824.f) || !(std::fabs(b) < 1073741824.f)) { beyond = true; break; }
      min_b[d] = (int)a;
      div[d] = (long long)b - (long long)a + 1;
    }
    if (beyond) {
      w->fail(SICP_ERR_INVALID_ARGUMENT, "the voxel grid of leaf size " + std::to_string(p.leaf_size) + " has coordinates beyond int32");
      continue;
    }
    if (div[0] * div[1] > (long long)INT32_MAX || div[0] * div[1] * div[2] > (long long)INT32_MAX) {
      w->fail(SICP_ERR_INVALID_ARGUMENT, "leaf size " + std::to_string(p.leaf_size) + " is too small for the cloud: the voxel grid (" +
                                             std::to_string(div[0]) + " x " + std::to_string(div[1]) + " x " + std::to_string(div[2]) +
                                             ") overflows int32");
      continue;
    }
    w->n_kept = n_kept;
    BootScratch& s = w->s;
    HIPCHECK(s.key.reserve(n)); HIPCHECK(s.key2.reserve(n));
    HIPCHECK(launch_boot_voxel_keys(n, s.x.p, s.y.p, s.z.p, s.lab.p, ig, p.box_max, inv_leaf, min_b, (int)div[0], (int)(div[0] * div[1]),
                                    s.key.p, st));
    size_t sort_bytes = 0, scan_bytes = 0;
    HIPCHECK(prim_sort_keys(nullptr, sort_bytes, s.key.p, s.key2.p, n, 0, 64, st));
    HIPCHECK(prim_scan_int(nullptr, scan_bytes, s.flag.p, s.pos.p, n_kept, st));
    SICPCHECK(temp_reserve(h, s, std::max(sort_bytes, scan_bytes)));
    HIPCHECK(prim_sort_keys(s.temp.p, sort_bytes, s.key.p, s.key2.p, n, 0, 64, st));
    HIPCHECK(s.flag.reserve(n_kept)); HIPCHECK(s.pos.reserve(n_kept)); HIPCHECK(s.heads.reserve(n_kept)); HIPCHECK(s.nout.reserve(1));
    HIPCHECK(launch_boot_voxel_compact((int)n_kept, s.key2.p, s.flag.p, s.pos.p, s.heads.p, s.nout.p, s.temp.p, scan_bytes, st));
    w->n_kp = 0;
    HIPCHECK(hipMemcpyAsync(&w->n_kp, s.nout.p, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIPCHECK(hipStreamSynchronize(st));
  for (CloudWork* w : W) {
    if (!w->live() || w->n_kept == 0) continue;
    BootScratch& s = w->s;
    BootCloud& out = w->k;
    const int n_kp = w->n_kp;
    out.n = n_kp;
    const size_t m = (size_t)std::max(n_kp, 1);
    HIPCHECK(out.kx.reserve(m)); HIPCHECK(out.ky.reserve(m)); HIPCHECK(out.kz.reserve(m));
    HIPCHECK(launch_boot_centroids(n_kp, (int)w->n_kept, s.heads.p, s.key2.p, s.x.p, s.y.p, s.z.p, out.kx.p, out.ky.p, out.kz.p, st));
    out.hx.resize(n_kp); out.hy.resize(n_kp); out.hz.resize(n_kp);
    HIPCHECK(hipMemcpyAsync(out.hx.data(), out.kx.p, sizeof(float) * n_kp, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.hy.data(), out.ky.p, sizeof(float) * n_kp, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.hz.data(), out.kz.p, sizeof(float) * n_kp, hipMemcpyDeviceToHost, st));
    if (lp) {
      HIPCHECK(out.kl.reserve(m));
      HIPCHECK(launch_boot_label_vote(n_kp, (int)w->n_kept, s.heads.p, s.key2.p, s.lab.p, out.kl.p, st));
      out.hl.resize(n_kp);
      HIPCHECK(hipMemcpyAsync(out.hl.data(), out.kl.p, sizeof(uint32_t) * n_kp, hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHECK(hipStreamSynchronize(st));
  return SICP_OK;
}

// radius-r neighbourhoods of every cloud's keypoints among themselves, CSR sorted by (d^2, index): count (one job launch),
// scan, fill (one job launch), segmented sort.  One synchronisation (the list totals) for all clouds.  normal = 0: the
// feature radius' lists (k.off / idx / d2), 1: the normal radius' own (s.noff / nidx / nd2)
int radius_stage(sicp_context* h, double r, int normal, const std::vector<CloudWork*>& W) {
  const hipStream_t st = h->stream;
  const float r2 = (float)(r * r);
  const float inv_cell = 1.0f / ((float)r * 1.001f);  // cells a little larger than r: every neighbour is in an adjacent cell
  std::vector<CloudWork*> L;
  for (CloudWork* w : W)
    if (w->live() && w->k.n > 0) L.push_back(w);
  auto lists = [&](CloudWork* w, DevBuf<long long>*& off, DevBuf<int>*& idx, DevBuf<float>*& d2) {
    if (normal) { off = &w->s.noff; idx = &w->s.nidx; d2 = &w->s.nd2; }
    else { off = &w->k.off; idx = &w->k.idx; d2 = &w->k.d2; }
  };
  auto job_of = [&](CloudWork* w) {
    BootCloudJob j;
    std::memset(&j, 0, sizeof j);
    j.m = w->k.n;
    j.x = w->k.kx.p; j.y = w->k.ky.p; j.z = w->k.kz.p;
    j.inv_cell = inv_cell; j.r2 = r2;
    j.skey = w->s.key2.p; j.sval = w->s.val2.p;
    return j;
  };
  BootTable<BootCloudJob> count;
  for (CloudWork* w : L) {
    const int m = w->k.n;
    BootScratch& s = w->s;
    DevBuf<long long>* off; DevBuf<int>* idx; DevBuf<float>* d2;
    lists(w, off, idx, d2);
    HIPCHECK(s.key.reserve(m)); HIPCHECK(s.key2.reserve(m)); HIPCHECK(s.val.reserve(m)); HIPCHECK(s.val2.reserve(m));
    HIPCHECK(s.cnt.reserve((size_t)m + 1)); HIPCHECK(off->reserve((size_t)m + 1));
    HIPCHECK(launch_boot_cell_keys(m, w->k.kx.p, w->k.ky.p, w->k.kz.p, inv_cell, s.key.p, s.val.p, st));
    size_t bytes = 0;
    w->scan_bytes = 0;
    HIPCHECK(prim_sort_pairs(nullptr, bytes, s.key.p, s.key2.p, s.val.p, s.val2.p, m, 0, 63, st));
    HIPCHECK(prim_scan_ll(nullptr, w->scan_bytes, s.cnt.p, off->p, m + 1, st));
    SICPCHECK(temp_reserve(h, s, std::max(bytes, w->scan_bytes)));
    HIPCHECK(prim_sort_pairs(s.temp.p, bytes, s.key.p, s.key2.p, s.val.p, s.val2.p, m, 0, 63, st));
    HIPCHECK(hipMemsetAsync(s.cnt.p + m, 0, sizeof(long long), st));
    BootCloudJob j = job_of(w);
    j.count = s.cnt.p;
    count.add(j, (m + 255) / 256);
  }
  HIPCHECK(count.upload(st));
  HIPCHECK(launch_boot_radius_jobs(0, count.d_jobs(), count.d_end(), count.nj(), count.blocks, st));
  for (CloudWork* w : L) {
    const int m = w->k.n;
    BootScratch& s = w->s;
    DevBuf<long long>* off; DevBuf<int>* idx; DevBuf<float>* d2;
    lists(w, off, idx, d2);
    HIPCHECK(prim_scan_ll(s.temp.p, w->scan_bytes, s.cnt.p, off->p, m + 1, st));
    w->cnt.assign(m, 0);
    w->total = 0;
    HIPCHECK(hipMemcpyAsync(w->cnt.data(), s.cnt.p, sizeof(long long) * m, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(&w->total, off->p + m, sizeof(long long), hipMemcpyDeviceToHost, st));
  }
  HIPCHECK(hipStreamSynchronize(st));
  BootTable<BootCloudJob> fill;
  std::vector<CloudWork*> F;
  for (CloudWork* w : L) {
    if (w->total > (long long)INT32_MAX) { w->fail(SICP_ERR_INVALID_ARGUMENT, "the radius neighbourhoods hold more than 2^31 entries"); continue; }
    long long mx = 0;
    for (long long v : w->cnt) mx = std::max(mx, v);
    if (normal) w->k.max_nbrs = std::max(w->k.max_nbrs, (int)mx);
    else { w->k.n_nbrs = w->total; w->k.max_nbrs = (int)mx; }
    BootScratch& s = w->s;
    DevBuf<long long>* off; DevBuf<int>* idx; DevBuf<float>* d2;
    lists(w, off, idx, d2);
    HIPCHECK(s.list.reserve((size_t)w->total + 1)); HIPCHECK(s.list2.reserve((size_t)w->total + 1));
    HIPCHECK(idx->reserve((size_t)w->total + 1)); HIPCHECK(d2->reserve((size_t)w->total + 1));
    BootCloudJob j = job_of(w);
    j.loff = off->p; j.list = s.list.p;
    fill.add(j, (w->k.n + 255) / 256);
    F.push_back(w);
  }
  HIPCHECK(fill.upload(st));
  HIPCHECK(launch_boot_radius_jobs(1, fill.d_jobs(), fill.d_end(), fill.nj(), fill.blocks, st));
  for (CloudWork* w : F) {
    BootScratch& s = w->s;
    DevBuf<long long>* off; DevBuf<int>* idx; DevBuf<float>* d2;
    lists(w, off, idx, d2);
    size_t bytes = 0;
    HIPCHECK(prim_segmented_sort_keys(nullptr, bytes, s.list.p, s.list2.p, w->total, w->k.n, off->p, st));
    SICPCHECK(temp_reserve(h, s, bytes));
    HIPCHECK(prim_segmented_sort_keys(s.temp.p, bytes, s.list.p, s.list2.p, w->total, w->k.n, off->p, st));
    HIPCHECK(launch_boot_split(w->total, s.list2.p, idx->p, d2->p, st));
  }
  // (the tables' host copies live until here: the stream is synchronised by the caller's next stage before they go)
  HIPCHECK(hipStreamSynchronize(st));
  return SICP_OK;
}

// normals (normal radius) and FPFH (feature radius) of every cloud's keypoints: one job launch each; then which
// keypoints have a feature (one synchronisation)
int feature_stage(sicp_context* h, const sicp_bootstrap_params& p, const std::vector<CloudWork*>& W) {
  const hipStream_t st = h->stream;
  SICPCHECK(radius_stage(h, p.feature_radius, 0, W));
  const bool own_normal_lists = p.normal_radius != p.feature_radius;
  if (own_normal_lists) SICPCHECK(radius_stage(h, p.normal_radius, 1, W));
  BootTable<BootCloudJob> nrm, pts;
  for (CloudWork* w : W) {
    if (!w->live() || w->k.n <= 0) continue;
    BootCloud& k = w->k;
    const int m = k.n;
    HIPCHECK(k.n3.reserve((size_t)m * 3)); HIPCHECK(k.fpfh.reserve((size_t)m * 33)); HIPCHECK(w->s.spfh.reserve((size_t)m * 33));
    BootCloudJob j;
    std::memset(&j, 0, sizeof j);
    j.m = m;
    j.x = k.kx.p; j.y = k.ky.p; j.z = k.kz.p;
    j.noff = own_normal_lists ? w->s.noff.p : k.off.p;
    j.nidx = own_normal_lists ? w->s.nidx.p : k.idx.p;
    j.off = k.off.p; j.idx = k.idx.p; j.d2 = k.d2.p;
    j.n3 = k.n3.p; j.spfh = w->s.spfh.p; j.fpfh = k.fpfh.p;
    nrm.add(j, (m + 255) / 256);
    pts.add(j, m);
  }
  HIPCHECK(nrm.upload(st));
  HIPCHECK(pts.upload(st));
  HIPCHECK(launch_boot_normal_jobs(nrm.d_jobs(), nrm.d_end(), nrm.nj(), nrm.blocks, st));
  HIPCHECK(launch_boot_fpfh_jobs(pts.d_jobs(), pts.d_end(), pts.nj(), pts.blocks, st));
  for (CloudWork* w : W) {
    if (!w->live()) continue;
    w->n3.assign((size_t)w->k.n * 3, 0.0);
    if (w->k.n > 0) HIPCHECK(hipMemcpyAsync(w->n3.data(), w->k.n3.p, sizeof(double) * w->n3.size(), hipMemcpyDeviceToHost, st));
  }
  HIPCHECK(hipStreamSynchronize(st));
  for (CloudWork* w : W) {
    if (!w->live()) continue;
    w->valid.resize(w->k.n);
    for (int i = 0; i < w->k.n; ++i) w->valid[i] = !std::isnan(w->n3[3 * (size_t)i]);
  }
  return SICP_OK;
}

// the feature k-NN of every source keypoint of every pair: one job launch, one read-back
int knn_stage(sicp_context* h, const sicp_bootstrap_params& p, const sicp_bootstrap_label_params* lp,
              const std::vector<PairWork*>& P) {
  const hipStream_t st = h->stream;
  const int k = p.k_correspondences;
  const bool same_label = lp && lp->match_same_label;
  BootTable<BootPairJob> tab;
  size_t total = 0;
  std::vector<PairWork*> L;
  for (PairWork* q : P) {
    const int ns = q->S->k.n, nt = q->T->k.n;
    q->knn.assign((size_t)ns * k, -1);
    if (ns > 0 && nt > 0) {
      q->knn_at = total;
      total += (size_t)ns * k;
      L.push_back(q);
    }
  }
  DevBuf<int> dk;
  HIPCHECK(dk.reserve(std::max<size_t>(total, 1)));
  for (PairWork* q : L) {
    BootPairJob j;
    std::memset(&j, 0, sizeof j);
    j.n = q->S->k.n; j.nt = q->T->k.n;
    j.sf = q->S->k.fpfh.p; j.tf = q->T->k.fpfh.p;
    j.out = dk.p + q->knn_at;
    if (same_label) { j.sl = q->S->k.kl.p; j.tl = q->T->k.kl.p; }
    tab.add(j, (j.n + 255) / 256);
  }
  HIPCHECK(tab.upload(st));
  HIPCHECK(launch_boot_feature_knn_jobs(tab.d_jobs(), tab.d_end(), tab.nj(), tab.blocks, k, same_label, st));
  for (PairWork* q : L) HIPCHECK(hipMemcpyAsync(q->knn.data(), dk.p + q->knn_at, sizeof(int) * q->knn.size(), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  for (PairWork* q : P) {
    q->src_valid.clear();
    q->row_k.clear();
    if (same_label) {
      // a row holds its label's neighbours first and -1 behind them; a keypoint without any cannot be sampled
      q->row_k.assign(q->S->k.n, 0);
      for (int i = 0; i < q->S->k.n; ++i) {
        int c = 0;
        while (c < k && q->knn[(size_t)i * k + c] >= 0) ++c;
        q->row_k[i] = c;
        if (q->S->valid[i] && c >= 1) q->src_valid.push_back(i);
      }
    } else {
      for (int i = 0; i < q->S->k.n; ++i)
        if (q->S->valid[i]) q->src_valid.push_back(i);
    }
    q->tgt_valid = 0;
    for (char v : q->T->valid) q->tgt_valid += v;
    q->k_eff = std::min(k, q->tgt_valid);
  }
  return SICP_OK;
}

// SampleConsensusInitialAlignment::computeTransformation of one pair on the host: per iteration selectSamples, then one
// random feature neighbour per sample (findSimilarFeatures), then the rigid transform of the pairs.  Depends on the
// pair and the seed only.
void draw_hypotheses(const sicp_bootstrap_params& p, PairWork& q) {
  const int iters = p.max_iterations, k = p.k_correspondences, nr = p.nr_samples;
  q.n_hyp = iters;
  q.M.assign((size_t)iters * 12, 0.0);
  q.Q.assign((size_t)iters * 4, 0.0);
  BootRng rng{p.seed};
  const int nv = (int)q.src_valid.size();
  const BootCloud &S = q.S->k, &T = q.T->k;
  std::vector<int> smp(nr);
  double sp[3 * kBootMaxSamples], tp[3 * kBootMaxSamples];
  for (int it = 0; it < iters; ++it) {
    int got = 0, fails = 0;
    float min_d = (float)p.min_sample_distance;
    const int max_fails = 3 * nv;
    while (got < nr) {
      const int si = q.src_valid[rng.index(nv)];
      bool ok = true;
      for (int j = 0; j < got; ++j) {
        const int sj = smp[j];
        const float dx = S.hx[si] - S.hx[sj], dy = S.hy[si] - S.hy[sj], dz = S.hz[si] - S.hz[sj];
        const float d = std::sqrt((dx * dx + dy * dy) + dz * dz);
        if (si == sj || d < min_d) { ok = false; break; }
      }
      if (ok) { smp[got++] = si; fails = 0; } else ++fails;
      if (fails >= max_fails) { min_d *= 0.5f; fails = 0; }
    }
    for (int j = 0; j < nr; ++j) {
      const int tj = q.knn[(size_t)smp[j] * k + rng.index(q.row_k.empty() ? q.k_eff : q.row_k[smp[j]])];
      sp[3 * j] = S.hx[smp[j]]; sp[3 * j + 1] = S.hy[smp[j]]; sp[3 * j + 2] = S.hz[smp[j]];
      tp[3 * j] = T.hx[tj]; tp[3 * j + 1] = T.hy[tj]; tp[3 * j + 2] = T.hz[tj];
    }
    rigid_from_pairs(nr, sp, tp, &q.Q[(size_t)it * 4], &q.M[(size_t)it * 12]);
  }
}

// the pairs' hypotheses on up to kGenThreads host threads (each pair is drawn by one thread: the result does not depend on
// how many there are)
void draw_all(const sicp_bootstrap_params& p, const std::vector<PairWork*>& P) {
  const int nt = std::min<int>(kGenThreads, (int)P.size());
  if (nt <= 1) {
    for (PairWork* q : P) draw_hypotheses(p, *q);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (size_t i = t; i < P.size(); i += nt) draw_hypotheses(p, *P[i]);
    });
  for (std::thread& x : th) x.join();
}

// the keypoints of a cloud as an engine cloud (flat layout, box tree): the scoring's query set and search tree
// (labels: with the keypoints' labels, which the tree build carries into its device order beside the coordinates)
int keypoint_tree(sicp_context* h, CloudWork& w, bool labels) {
  if (w.tree) return SICP_OK;
  w.tree = acquire_cloud(h->device);
  const BootCloud& k = w.k;
  const StridedCloud ks = {(const char*)k.hx.data(), (const char*)k.hy.data(), (const char*)k.hz.data(),
                           labels ? (const char*)k.hl.data() : nullptr, 4, 4};
  SICPCHECK(stage_cloud(h, *w.tree, k.n, ks));
  w.tree->is_set = true; w.tree->layout = -1;
  return prepare_cloud(h, *w.tree);
}

// the truncated error of every pair's hypotheses (rows 0..2 of their 4x4 matrices): one K = 1 search of every source
// keypoint per hypothesis on a box tree of the target keypoints.  The hypotheses of all pairs are cut into chunks of at most
// kScoreOutputs search outputs; a chunk's searches are collected into the packet kernel's job launches, then one
// error launch reduces the whole chunk.  One read-back at the end.
int score_stage(sicp_context* h, const sicp_bootstrap_params& p, const sicp_bootstrap_label_params* lp,
                const std::vector<PairWork*>& P) {
  const hipStream_t st = h->stream;
  const bool same_label = lp && lp->score_same_label;
  BootParamsScope scope(h);
  for (PairWork* q : P) { SICPCHECK(keypoint_tree(h, *q->S, same_label)); SICPCHECK(keypoint_tree(h, *q->T, same_label)); }
  for (PairWork* q : P) { SICPCHECK(cloud_wait(h, *q->S->tree)); SICPCHECK(cloud_wait(h, *q->T->tree)); }
  size_t n_err = 0;
  long long outputs = 0, max_nq = 1;
  for (PairWork* q : P) {
    q->err_at = n_err;
    n_err += (size_t)q->n_hyp;
    const long long nq = q->S->tree->n;
    outputs += nq * q->n_hyp;
    max_nq = std::max(max_nq, nq);
  }
  if (n_err == 0) return SICP_OK;
  const long long cap = std::max(max_nq, std::min(outputs, kScoreOutputs));
  DevBuf<int> oi;
  DevBuf<float> od;
  DevBuf<double> derr;
  HIPCHECK(oi.reserve((size_t)cap)); HIPCHECK(od.reserve((size_t)cap)); HIPCHECK(derr.reserve(n_err));
  const float inf = std::numeric_limits<float>::infinity();
  const double t = (double)(float)p.max_corr_distance;
  std::vector<std::unique_ptr<BootTable<BootPairJob>>> tables;  // (alive until the read-back's synchronisation)
  JobCollector jc;
  std::unique_ptr<BootTable<BootPairJob>> tab(new BootTable<BootPairJob>);
  long long used = 0;
  auto flush = [&]() -> int {
    if (jc.part[0].knn.empty()) return SICP_OK;
    HIPCHECK(sicp::launch_bvh_knn_packet_jobs(jc.part[0].knn_K, jc.part[0].knn.data(), (int)jc.part[0].knn.size(), st));
    HIPCHECK(tab->upload(st));
    HIPCHECK(launch_boot_error_jobs(tab->d_jobs(), tab->d_end(), tab->nj(), tab->blocks, t, same_label, st));
    tables.push_back(std::move(tab));
    tab.reset(new BootTable<BootPairJob>);
    jc.part[0].knn.clear();
    used = 0;
    return SICP_OK;
  };
  for (PairWork* q : P) {
    const Cloud &qc = *q->S->tree, &tc = *q->T->tree;
    const int nq = qc.n;
    for (int i0 = 0; i0 < q->n_hyp;) {
      if (used > 0 && used + nq > cap) SICPCHECK(flush());
      // this pair's hypotheses that fit into the chunk: one error job
      const int cnt = (int)std::min<long long>(q->n_hyp - i0, std::max<long long>(1, (cap - used) / std::max(nq, 1)));
      BootPairJob j;
      std::memset(&j, 0, sizeof j);
      j.n = cnt; j.nt = nq;
      j.d2 = od.p + used;
      j.err = derr.p + q->err_at + i0;
      // (the search writes row r for the source tree's device point r, and the target tree's device index of its neighbour)
      if (same_label) { j.nbr = oi.p + used; j.sl = qc.label.p; j.tl = tc.label.p; }
      {
        CollectScope cs(h, &jc);
        for (int i = 0; i < cnt; ++i)
          SICPCHECK(run_nn(h, 1, qc, 0, nq, q->M.data() + 12 * (size_t)(i0 + i), tc, 0, false, inf, oi.p + used + (size_t)i * nq,
                           od.p + used + (size_t)i * nq, 0, st));
      }
      tab->add(j, cnt);
      used += (long long)cnt * nq;
      i0 += cnt;
    }
  }
  SICPCHECK(flush());
  std::vector<double> err(n_err);
  HIPCHECK(hipMemcpyAsync(err.data(), derr.p, sizeof(double) * n_err, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  for (PairWork* q : P) q->err.assign(err.begin() + q->err_at, err.begin() + q->err_at + q->n_hyp);
  return SICP_OK;
}

int check_clouds(sicp_context* h) {
  if (!h->cl[0] || !h->cl[1] || !h->cloud(SICP_SOURCE).is_set || !h->cloud(SICP_TARGET).is_set) return SICP_ERR_NOT_READY;
  return SICP_OK;
}

// keypoints + features of every cloud, then the feature k-NN of every pair whose clouds have them
int prepare(sicp_context* h, const sicp_bootstrap_params& p, const sicp_bootstrap_label_params* lp,
            const std::vector<CloudWork*>& W, const std::vector<PairWork*>& P, double* t_kp, double* t_feat, double* t_knn) {
  const double t0 = now_ms();
  SICPCHECK(voxel_stage(h, p, lp, W));
  const double t1 = now_ms();
  SICPCHECK(feature_stage(h, p, W));
  const double t2 = now_ms();
  std::vector<PairWork*> L;
  for (PairWork* q : P) {
    if (q->status != SICP_OK) continue;
    for (CloudWork* w : {q->S, q->T})
      if (!w->live() && q->status == SICP_OK) { q->status = w->status; q->msg = w->msg; }
    if (q->status == SICP_OK) L.push_back(q);
  }
  SICPCHECK(knn_stage(h, p, lp, L));
  const double t3 = now_ms();
  if (t_kp) *t_kp += t1 - t0;
  if (t_feat) *t_feat += t2 - t1;
  if (t_knn) *t_knn += t3 - t2;
  return SICP_OK;
}

// the whole bootstrap of n pairs (hs[i]'s source onto its target) on h's stream; status[i] per pair, messages prefixed
// with `who` (and the pair's index when `indexed`).  Returns SICP_OK or the code of a failure of the call itself (HIP,
// memory), which is then every unfinished pair's status too.
int run_batch(sicp_context* h, sicp_handle* hs, int n, const sicp_bootstrap_params& p, const sicp_bootstrap_label_params* lp,
              double* out_qt, int32_t* status, sicp_bootstrap_info* infos, const char* who, bool indexed) {
  const double t_begin = now_ms();
  std::vector<PairWork> pairs(n);
  for (int i = 0; i < n; ++i) {
    pairs[i].index = i;
    if (check_clouds(hs[i]) != SICP_OK) { pairs[i].status = SICP_ERR_NOT_READY; pairs[i].msg = "the handle has no source or no target cloud"; }
    else if (lp && (!hs[i]->cloud(SICP_SOURCE).has_label || !hs[i]->cloud(SICP_TARGET).has_label)) {
      pairs[i].status = SICP_ERR_INVALID_ARGUMENT;
      pairs[i].msg = std::string(hs[i]->cloud(SICP_SOURCE).has_label ? "the target" : "the source") + " cloud has no labels";
    }
  }
  double t_kp = 0, t_feat = 0, t_match = 0, t_score = 0;
  std::map<const Cloud*, std::unique_ptr<CloudWork>> cache;  // this group's clouds (and the previous group's it shares)
  int rc = SICP_OK;
  int i0 = 0;
  while (i0 < n && rc == SICP_OK) {
    // the next group: up to kGroupPairs pairs whose clouds not yet prepared hold up to kGroupPoints points (at least one pair)
    std::vector<PairWork*> G;
    std::set<const Cloud*> need;
    long long pts = 0;
    int i1 = i0;
    for (; i1 < n && (int)G.size() < kGroupPairs; ++i1) {
      PairWork& q = pairs[i1];
      if (q.status != SICP_OK) continue;
      const Cloud *a = hs[i1]->cl[0].get(), *b = hs[i1]->cl[1].get();
      long long add = 0;
      for (const Cloud* c : {a, b})
        if (!need.count(c) && !cache.count(c) && !(c == b && a == b)) add += c->n;  // (a == b: counted once)
      if (!G.empty() && pts + add > kGroupPoints) break;
      pts += add;
      need.insert(a); need.insert(b);
      G.push_back(&q);
    }
    i0 = i1;
    for (auto it = cache.begin(); it != cache.end();) it = need.count(it->first) ? std::next(it) : cache.erase(it);
    std::vector<CloudWork*> W;
    for (PairWork* q : G) {
      const Cloud* cs[2] = {hs[q->index]->cl[0].get(), hs[q->index]->cl[1].get()};
      for (int w = 0; w < 2; ++w) {
        std::unique_ptr<CloudWork>& slot = cache[cs[w]];
        if (!slot) { slot.reset(new CloudWork); slot->c = cs[w]; W.push_back(slot.get()); }
        (w == 0 ? q->S : q->T) = slot.get();
      }
    }
    rc = prepare(h, p, lp, W, G, &t_kp, &t_feat, &t_match);
    if (rc != SICP_OK) break;
    const double tm0 = now_ms();
    std::vector<PairWork*> L;
    for (PairWork* q : G) {
      if (q->status != SICP_OK) continue;
      if ((int)q->src_valid.size() < p.nr_samples || q->tgt_valid < 1) {
        q->status = SICP_ERR_TOO_FEW_POINTS;
        q->msg = std::to_string(q->src_valid.size()) + " source / " + std::to_string(q->tgt_valid) + " target keypoints with features";
        continue;
      }
      L.push_back(q);
    }
    draw_all(p, L);
    const double tm1 = now_ms();
    t_match += tm1 - tm0;
    rc = score_stage(h, p, lp, L);
    t_score += now_ms() - tm1;
    if (rc != SICP_OK) break;
    for (PairWork* q : L) {
      int best = 0;
      for (int it = 1; it < q->n_hyp; ++it)
        if (q->err[it] < q->err[best]) best = it;
      const double* Q = &q->Q[(size_t)best * 4];
      double* o = out_qt + 7 * (size_t)q->index;
      o[0] = Q[1]; o[1] = Q[2]; o[2] = Q[3]; o[3] = Q[0];
      o[4] = q->M[(size_t)best * 12 + 3]; o[5] = q->M[(size_t)best * 12 + 7]; o[6] = q->M[(size_t)best * 12 + 11];
      if (infos) {
        sicp_bootstrap_info& info = infos[q->index];
        info.n_source_keypoints = q->S->k.n;
        info.n_target_keypoints = q->T->k.n;
        info.max_neighbours = std::max(q->S->k.max_nbrs, q->T->k.max_nbrs);
        info.best_iteration = best;
        info.best_error = q->err[best];
      }
      q->err.clear(); q->M.clear(); q->Q.clear(); q->knn.clear(); q->row_k.clear();
      q->done = true;
    }
  }
  const std::string why = rc != SICP_OK ? h->last_error : std::string();
  int first = -1;
  for (int i = 0; i < n; ++i) {
    PairWork& q = pairs[i];
    if (q.status == SICP_OK && !q.done) { q.status = rc != SICP_OK ? rc : SICP_ERR_INTERNAL; q.msg = rc != SICP_OK ? why : "not run"; }
    if (status) status[i] = q.status;
    if (q.status != SICP_OK) {
      const std::string m = std::string(who) + ": " + (indexed ? "pair " + std::to_string(i) + ": " : std::string()) + q.msg;
      hs[i]->last_error = m;
      if (first < 0) { first = i; h->last_error = m; }
    }
  }
  if (infos) {
    const double t_total = now_ms() - t_begin;
    for (int i = 0; i < n; ++i) {
      if (pairs[i].status != SICP_OK) continue;
      sicp_bootstrap_info& info = infos[i];
      info.t_keypoints_ms = t_kp;
      info.t_features_ms = t_feat;
      info.t_match_ms = t_match;
      info.t_score_ms = t_score;
      info.t_total_ms = t_total;
    }
  }
  if (rc != SICP_OK) return rc;
  return first < 0 ? SICP_OK : pairs[first].status;
}

}  // namespace

// splitmix64 (Steele, Lea, Flood 2014): the sampling's documented PRNG
uint64_t BootRng::next() {
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
int BootRng::index(int n) {
  const double u = (double)(next() >> 11) * 0x1.0p-53;
  return (int)std::floor((double)n * u);
}

void bootstrap_default_params(sicp_bootstrap_params* p) {
  std::memset(p, 0, sizeof *p);
  p->box_max = 35.0;
  p->leaf_size = 0.4;
  p->normal_radius = 3.0;
  p->feature_radius = 3.0;
  p->min_sample_distance = 0.4;
  p->max_corr_distance = 0.8;
  p->max_iterations = 500;
  p->nr_samples = 3;
  p->k_correspondences = 10;
  p->seed = 1;
}

namespace {

// sicp_bootstrap / sicp_bootstrap_semantic (lp: NULL in the former, checked by the caller in the latter)
int run_one(sicp_context* h, const sicp_bootstrap_params* pp, const sicp_bootstrap_label_params* lp, double* out_qt,
            sicp_bootstrap_info* info, const char* who) {
  if (!pp || !out_qt) return SICP_ERR_INVALID_ARGUMENT;
  const sicp_bootstrap_params p = *pp;
  SICPCHECK(check_params(h, p, who));
  if (lp) SICPCHECK(check_label_params(h, *lp, who));
  SICPCHECK(set_device(h));
  SICPCHECK(check_clouds(h));
  // a batch of one: the same stages and kernels as any batch
  int32_t st = SICP_OK;
  sicp_handle hs[1] = {h};
  const int rc = run_batch(h, hs, 1, p, lp, out_qt, &st, info, who, false);
  return rc != SICP_OK ? rc : st;
}

int run_many(sicp_handle* hs, int32_t n, const sicp_bootstrap_params* pp, const sicp_bootstrap_label_params* lp, bool semantic,
             double* out_qt, int32_t* status, sicp_bootstrap_info* infos, const char* who) {
  if (!hs || n < 1) return SICP_ERR_INVALID_ARGUMENT;
  sicp_context* h = hs[0];
  auto refuse = [&](const std::string& why) {
    if (h) h->last_error = std::string(who) + ": " + why;
    return SICP_ERR_INVALID_ARGUMENT;
  };
  for (int i = 0; i < n; ++i)
    if (!hs[i]) return refuse("handle " + std::to_string(i) + " is NULL");
  if (!pp) return refuse("params is NULL");
  if (semantic && !lp) return refuse("label params is NULL");
  if (!out_qt) return refuse("out_qt is NULL");
  for (int i = 1; i < n; ++i)
    if (hs[i]->device != h->device)
      return refuse("handle " + std::to_string(i) + " is on device " + std::to_string(hs[i]->device) + ", handle 0 on " + std::to_string(h->device));
  const sicp_bootstrap_params p = *pp;
  SICPCHECK(check_params(h, p, who));
  sicp_bootstrap_label_params l;
  if (lp) { l = *lp; SICPCHECK(check_label_params(h, l, who)); }
  SICPCHECK(set_device(h));
  return run_batch(h, hs, n, p, lp ? &l : nullptr, out_qt, status, infos, who, true);
}

// a semantic entry point's label params: NULL is refused with its message
int need_label_params(sicp_context* h, const sicp_bootstrap_label_params* lp, const char* who) {
  if (lp) return SICP_OK;
  h->last_error = std::string(who) + ": label params is NULL";
  return SICP_ERR_INVALID_ARGUMENT;
}

// a hook's clouds carry labels when it runs a label form
int need_labels(sicp_context* h, const sicp_bootstrap_label_params* lp, int first, int last, const char* who) {
  if (!lp) return SICP_OK;
  for (int w = first; w <= last; ++w)
    if (!h->cloud(w).has_label) {
      h->last_error = std::string(who) + ": the " + (w == SICP_SOURCE ? "source" : "target") + " cloud has no labels";
      return SICP_ERR_INVALID_ARGUMENT;
    }
  return SICP_OK;
}

// sicp_bootstrap_score / sicp_bootstrap_semantic_score
int score_hook(sicp_context* h, const sicp_bootstrap_params* pp, const sicp_bootstrap_label_params* lpp, int32_t n,
               const int32_t* src_idx, const int32_t* tgt_idx, double* M12, double* err, int32_t knn_capacity, int32_t* feat_knn,
               const char* who) {
  if (!pp || n < 0 || (n > 0 && (!src_idx || !tgt_idx || !err))) return SICP_ERR_INVALID_ARGUMENT;
  const sicp_bootstrap_params p = *pp;
  SICPCHECK(check_params(h, p, who));
  sicp_bootstrap_label_params l;
  if (lpp) { l = *lpp; SICPCHECK(check_label_params(h, l, who)); }
  const sicp_bootstrap_label_params* lp = lpp ? &l : nullptr;
  SICPCHECK(set_device(h));
  SICPCHECK(check_clouds(h));
  SICPCHECK(need_labels(h, lp, SICP_SOURCE, SICP_TARGET, who));
  CloudWork cw[2];
  cw[0].c = &h->cloud(SICP_SOURCE);
  cw[1].c = &h->cloud(SICP_TARGET);
  PairWork q;
  q.S = &cw[0]; q.T = &cw[1];
  SICPCHECK(prepare(h, p, lp, {&cw[0], &cw[1]}, {&q}, nullptr, nullptr, nullptr));
  if (q.status != SICP_OK) {
    h->last_error = std::string(who) + ": " + q.msg;
    return q.status;
  }
  const BootCloud &S = cw[0].k, &T = cw[1].k;
  if (feat_knn) {
    if ((long long)knn_capacity < (long long)S.n * p.k_correspondences) return SICP_ERR_INVALID_ARGUMENT;
    std::memcpy(feat_knn, q.knn.data(), sizeof(int) * q.knn.size());
  }
  if (n == 0) return SICP_OK;
  if (S.n < 1 || T.n < 1) return SICP_ERR_TOO_FEW_POINTS;
  const int nr = p.nr_samples;
  q.n_hyp = n;
  q.M.assign((size_t)n * 12, 0.0);
  double sp[3 * kBootMaxSamples], tp[3 * kBootMaxSamples], qq[4];
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < nr; ++j) {
      const int a = src_idx[(size_t)i * nr + j], b = tgt_idx[(size_t)i * nr + j];
      if (a < 0 || a >= S.n || b < 0 || b >= T.n) {
        h->last_error = std::string(who) + "_score: sample " + std::to_string(i) + " names a keypoint that does not exist";
        return SICP_ERR_INVALID_ARGUMENT;
      }
      sp[3 * j] = S.hx[a]; sp[3 * j + 1] = S.hy[a]; sp[3 * j + 2] = S.hz[a];
      tp[3 * j] = T.hx[b]; tp[3 * j + 1] = T.hy[b]; tp[3 * j + 2] = T.hz[b];
    }
    rigid_from_pairs(nr, sp, tp, qq, &q.M[(size_t)i * 12]);
  }
  SICPCHECK(score_stage(h, p, lp, {&q}));
  std::memcpy(err, q.err.data(), sizeof(double) * n);
  if (M12) std::memcpy(M12, q.M.data(), sizeof(double) * q.M.size());
  return SICP_OK;
}

}  // namespace

void bootstrap_default_label_params(sicp_bootstrap_label_params* lp) {
  std::memset(lp, 0, sizeof *lp);
  lp->match_same_label = 1;
  lp->score_same_label = 1;
}

int bootstrap_run(sicp_context* h, const sicp_bootstrap_params* pp, double* out_qt, sicp_bootstrap_info* info) {
  return run_one(h, pp, nullptr, out_qt, info, "sicp_bootstrap");
}

int bootstrap_semantic_run(sicp_context* h, const sicp_bootstrap_params* pp, const sicp_bootstrap_label_params* lpp, double* out_qt,
                           sicp_bootstrap_info* info) {
  SICPCHECK(need_label_params(h, lpp, "sicp_bootstrap_semantic"));
  const sicp_bootstrap_label_params lp = *lpp;
  return run_one(h, pp, &lp, out_qt, info, "sicp_bootstrap_semantic");
}

int bootstrap_batch(sicp_handle* hs, int32_t n, const sicp_bootstrap_params* pp, double* out_qt, int32_t* status,
                    sicp_bootstrap_info* infos) {
  return run_many(hs, n, pp, nullptr, false, out_qt, status, infos, "sicp_bootstrap_batch");
}

int bootstrap_semantic_batch(sicp_handle* hs, int32_t n, const sicp_bootstrap_params* pp, const sicp_bootstrap_label_params* lp,
                             double* out_qt, int32_t* status, sicp_bootstrap_info* infos) {
  return run_many(hs, n, pp, lp, true, out_qt, status, infos, "sicp_bootstrap_semantic_batch");
}

int bootstrap_keypoints(sicp_context* h, int which, const sicp_bootstrap_params* pp, int32_t capacity, int64_t nbr_capacity,
                        int32_t* n_keypoints, int64_t* n_nbrs, float* xyz3, double* normal3, float* fpfh33,
                        int64_t* nbr_offsets, int32_t* nbr_idx) {
  if (!pp || (which != SICP_SOURCE && which != SICP_TARGET)) return SICP_ERR_INVALID_ARGUMENT;
  const sicp_bootstrap_params p = *pp;
  SICPCHECK(check_params(h, p, "sicp_bootstrap"));
  SICPCHECK(set_device(h));
  SICPCHECK(check_clouds(h));
  CloudWork w;
  w.c = &h->cloud(which);
  const std::vector<CloudWork*> W = {&w};
  SICPCHECK(voxel_stage(h, p, nullptr, W));
  SICPCHECK(feature_stage(h, p, W));
  if (!w.live()) {
    h->last_error = "sicp_bootstrap: " + w.msg;
    return w.status;
  }
  const BootCloud& k = w.k;
  if (n_keypoints) *n_keypoints = k.n;
  if (n_nbrs) *n_nbrs = k.n_nbrs;
  const int m = k.n;
  if ((xyz3 || normal3 || fpfh33 || nbr_offsets) && capacity < m) return SICP_ERR_INVALID_ARGUMENT;
  if (nbr_idx && nbr_capacity < k.n_nbrs) return SICP_ERR_INVALID_ARGUMENT;
  if (m == 0) {
    if (nbr_offsets) nbr_offsets[0] = 0;
    return SICP_OK;
  }
  const hipStream_t st = h->stream;
  if (xyz3)
    for (int i = 0; i < m; ++i) { xyz3[3 * i] = k.hx[i]; xyz3[3 * i + 1] = k.hy[i]; xyz3[3 * i + 2] = k.hz[i]; }
  if (normal3) std::memcpy(normal3, w.n3.data(), sizeof(double) * 3 * m);
  if (fpfh33) HIPCHECK(hipMemcpyAsync(fpfh33, k.fpfh.p, sizeof(float) * 33 * m, hipMemcpyDeviceToHost, st));
  if (nbr_offsets) HIPCHECK(hipMemcpyAsync(nbr_offsets, k.off.p, sizeof(long long) * (m + 1), hipMemcpyDeviceToHost, st));
  if (nbr_idx && k.n_nbrs > 0) HIPCHECK(hipMemcpyAsync(nbr_idx, k.idx.p, sizeof(int) * k.n_nbrs, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return SICP_OK;
}

// the keypoints of the label forms and their labels: the voxel stage alone
int bootstrap_semantic_keypoints(sicp_context* h, int which, const sicp_bootstrap_params* pp, const sicp_bootstrap_label_params* lpp,
                                 int32_t capacity, int32_t* n_keypoints, float* xyz3, uint32_t* label) {
  const char* who = "sicp_bootstrap_semantic_keypoints";
  if (!pp || (which != SICP_SOURCE && which != SICP_TARGET)) return SICP_ERR_INVALID_ARGUMENT;
  SICPCHECK(need_label_params(h, lpp, who));
  const sicp_bootstrap_params p = *pp;
  const sicp_bootstrap_label_params lp = *lpp;
  SICPCHECK(check_params(h, p, who));
  SICPCHECK(check_label_params(h, lp, who));
  SICPCHECK(set_device(h));
  SICPCHECK(check_clouds(h));
  SICPCHECK(need_labels(h, &lp, which, which, who));
  CloudWork w;
  w.c = &h->cloud(which);
  SICPCHECK(voxel_stage(h, p, &lp, {&w}));
  if (!w.live()) {
    h->last_error = std::string(who) + ": " + w.msg;
    return w.status;
  }
  const BootCloud& k = w.k;
  if (n_keypoints) *n_keypoints = k.n;
  if ((xyz3 || label) && capacity < k.n) return SICP_ERR_INVALID_ARGUMENT;
  if (xyz3)
    for (int i = 0; i < k.n; ++i) { xyz3[3 * i] = k.hx[i]; xyz3[3 * i + 1] = k.hy[i]; xyz3[3 * i + 2] = k.hz[i]; }
  if (label && k.n > 0) std::memcpy(label, k.hl.data(), sizeof(uint32_t) * k.n);
  return SICP_OK;
}

int bootstrap_score(sicp_context* h, const sicp_bootstrap_params* pp, int32_t n, const int32_t* src_idx, const int32_t* tgt_idx,
                    double* M12, double* err, int32_t knn_capacity, int32_t* feat_knn) {
  return score_hook(h, pp, nullptr, n, src_idx, tgt_idx, M12, err, knn_capacity, feat_knn, "sicp_bootstrap");
}

int bootstrap_semantic_score(sicp_context* h, const sicp_bootstrap_params* pp, const sicp_bootstrap_label_params* lp, int32_t n,
                             const int32_t* src_idx, const int32_t* tgt_idx, double* M12, double* err, int32_t knn_capacity,
                             int32_t* feat_knn) {
  SICPCHECK(need_label_params(h, lp, "sicp_bootstrap_semantic_score"));
  return score_hook(h, pp, lp, n, src_idx, tgt_idx, M12, err, knn_capacity, feat_knn, "sicp_bootstrap_semantic");
}

}  // namespace host
}  // namespace sicp
