// bootstrap.cpp -- the stage driver of the initial alignment without a pose prior (exec/bootstrap.h, class Bootstrap):
// box filter + VoxelGrid keypoints, radius neighbourhoods, normals and FPFH features of both clouds on the device, then
// SampleConsensusInitialAlignment: the hypotheses are drawn on the host from a documented PRNG (splitmix64), their rigid
// transforms solved on the host in f64, and all of them are scored on the device at once -- one K = 1 box-tree search per
// hypothesis over a tree of the target keypoints, collected into the packet kernel's job launches, then one
// truncated-error reduction.  Orders and precisions: INTEGRATION.md ("Bootstrap").
#include "bootstrap.hpp"

namespace sicp {
namespace host {

namespace {

typedef unsigned long long u64;

// the keypoints of one cloud and their features, device-resident (keypoint order)
struct BootCloud {
  int n = 0;
  std::vector<float> hx, hy, hz;  // host copy of the keypoints (sampling distances, the search tree's staging)
  DevBuf<float> kx, ky, kz;
  // neighbourhoods of the feature radius (CSR); those of the normal radius when the two radii differ live in nrm_*
  long long n_nbrs = 0;
  int max_nbrs = 0;
  DevBuf<long long> off;
  DevBuf<int> idx;
  DevBuf<float> d2;
  DevBuf<double> n3;
  DevBuf<float> fpfh;
};

// every scratch buffer of one call (arena blocks: recycled between calls)
struct BootScratch {
  DevBuf<float> x, y, z, blk;
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

int temp_reserve(sicp_context* h, BootScratch& s, size_t bytes) {
  HIPCHECK(s.temp.reserve(bytes + 256));
  return SICP_OK;
}

int check_params(sicp_context* h, const sicp_bootstrap_params& p) {
  auto bad = [&](const char* what) {
    h->last_error = std::string("sicp_bootstrap: ") + what;
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

// box filter + voxel grid: keypoints = centroids of the occupied voxels in ascending voxel index
int voxel_keypoints(sicp_context* h, const Cloud& c, const sicp_bootstrap_params& p, BootScratch& s, BootCloud& out) {
  const int n = c.n;
  const hipStream_t st = h->stream;
  out.n = 0;
  if (n <= 0) return SICP_OK;
  if (c.hx.size() < (size_t)n) return SICP_ERR_NOT_READY;
  HIPCHECK(s.x.reserve(n)); HIPCHECK(s.y.reserve(n)); HIPCHECK(s.z.reserve(n));
  HIPCHECK(hipMemcpyAsync(s.x.p, c.hx.data(), sizeof(float) * n, hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemcpyAsync(s.y.p, c.hy.data(), sizeof(float) * n, hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemcpyAsync(s.z.p, c.hz.data(), sizeof(float) * n, hipMemcpyHostToDevice, st));
  const int nb = boot_bounds_blocks(n);
  HIPCHECK(s.blk.reserve((size_t)nb * 8));
  HIPCHECK(launch_boot_bounds(n, s.x.p, s.y.p, s.z.p, p.box_max, s.blk.p, st));
  std::vector<float> blk((size_t)nb * 8);
  HIPCHECK(hipMemcpyAsync(blk.data(), s.blk.p, sizeof(float) * blk.size(), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  const float inf = std::numeric_limits<float>::infinity();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  long long n_kept = 0;
  for (int b = 0; b < nb; ++b) {
    for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], blk[b * 8 + d]); hi[d] = std::max(hi[d], blk[b * 8 + 3 + d]); }
    n_kept += (long long)blk[b * 8 + 6];
  }
  if (n_kept == 0) return SICP_OK;
  // PCL VoxelGrid::applyFilter: min_b / max_b = floor(min_p / max_p * (1 / leaf)) in f32
  const float inv_leaf = 1.0f / (float)p.leaf_size;
  int min_b[3];
  long long div[3];
  for (int d = 0; d < 3; ++d) {
    const float a = std::floor(lo[d] * inv_leaf), b = std::floor(hi[d] * inv_leaf);
    if (!(std::fabs(a) < 1073741824.f) || !(std::fabs(b) < 1073741824.f)) {
      h->last_error = "sicp_bootstrap: the voxel grid of leaf size " + std::to_string(p.leaf_size) + " has coordinates beyond int32";
      return SICP_ERR_INVALID_ARGUMENT;
    }
    min_b[d] = (int)a;
    div[d] = (long long)b - (long long)a + 1;
  }
  if (div[0] * div[1] > (long long)INT32_MAX || div[0] * div[1] * div[2] > (long long)INT32_MAX) {
    h->last_error = "sicp_bootstrap: leaf size " + std::to_string(p.leaf_size) + " is too small for the cloud: the voxel grid (" +
                    std::to_string(div[0]) + " x " + std::to_string(div[1]) + " x " + std::to_string(div[2]) + ") overflows int32";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  HIPCHECK(s.key.reserve(n)); HIPCHECK(s.key2.reserve(n));
  HIPCHECK(launch_boot_voxel_keys(n, s.x.p, s.y.p, s.z.p, p.box_max, inv_leaf, min_b, (int)div[0], (int)(div[0] * div[1]), s.key.p, st));
  size_t sort_bytes = 0, scan_bytes = 0;
  HIPCHECK(boot_sort_keys(nullptr, sort_bytes, s.key.p, s.key2.p, n, st));
  HIPCHECK(boot_scan_int(nullptr, scan_bytes, s.flag.p, s.pos.p, (int)n_kept, st));
  SICPCHECK(temp_reserve(h, s, std::max(sort_bytes, scan_bytes)));
  HIPCHECK(boot_sort_keys(s.temp.p, sort_bytes, s.key.p, s.key2.p, n, st));
  HIPCHECK(s.flag.reserve(n_kept)); HIPCHECK(s.pos.reserve(n_kept)); HIPCHECK(s.heads.reserve(n_kept)); HIPCHECK(s.nout.reserve(1));
  HIPCHECK(launch_boot_voxel_compact((int)n_kept, s.key2.p, s.flag.p, s.pos.p, s.heads.p, s.nout.p, s.temp.p, scan_bytes, st));
  int n_kp = 0;
  HIPCHECK(hipMemcpyAsync(&n_kp, s.nout.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  out.n = n_kp;
  const size_t m = (size_t)std::max(n_kp, 1);
  HIPCHECK(out.kx.reserve(m)); HIPCHECK(out.ky.reserve(m)); HIPCHECK(out.kz.reserve(m));
  HIPCHECK(launch_boot_centroids(n_kp, (int)n_kept, s.heads.p, s.key2.p, s.x.p, s.y.p, s.z.p, out.kx.p, out.ky.p, out.kz.p, st));
  out.hx.resize(n_kp); out.hy.resize(n_kp); out.hz.resize(n_kp);
  HIPCHECK(hipMemcpyAsync(out.hx.data(), out.kx.p, sizeof(float) * n_kp, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(out.hy.data(), out.ky.p, sizeof(float) * n_kp, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(out.hz.data(), out.kz.p, sizeof(float) * n_kp, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return SICP_OK;
}

// radius-r neighbourhoods of the keypoints among themselves, CSR sorted by (d^2, index): count, scan, fill, segmented sort
int radius_lists(sicp_context* h, const BootCloud& k, double r, BootScratch& s, DevBuf<long long>& off, DevBuf<int>& idx,
                 DevBuf<float>& d2, long long* total_out, int* max_out) {
  const int m = k.n;
  const hipStream_t st = h->stream;
  const float r2 = (float)(r * r);
  const float inv_cell = 1.0f / ((float)r * 1.001f);  // cells a little larger than r: every neighbour is in an adjacent cell
  HIPCHECK(s.key.reserve(m)); HIPCHECK(s.key2.reserve(m)); HIPCHECK(s.val.reserve(m)); HIPCHECK(s.val2.reserve(m));
  HIPCHECK(s.cnt.reserve((size_t)m + 1)); HIPCHECK(off.reserve((size_t)m + 1));
  HIPCHECK(launch_boot_cell_keys(m, k.kx.p, k.ky.p, k.kz.p, inv_cell, s.key.p, s.val.p, st));
  size_t bytes = 0, scan_bytes = 0;
  HIPCHECK(boot_sort_pairs(nullptr, bytes, s.key.p, s.key2.p, s.val.p, s.val2.p, m, st));
  HIPCHECK(boot_scan_ll(nullptr, scan_bytes, s.cnt.p, off.p, m + 1, st));
  SICPCHECK(temp_reserve(h, s, std::max(bytes, scan_bytes)));
  HIPCHECK(boot_sort_pairs(s.temp.p, bytes, s.key.p, s.key2.p, s.val.p, s.val2.p, m, st));
  HIPCHECK(hipMemsetAsync(s.cnt.p + m, 0, sizeof(long long), st));
  HIPCHECK(launch_boot_radius(0, m, k.kx.p, k.ky.p, k.kz.p, inv_cell, s.key2.p, s.val2.p, r2, s.cnt.p, nullptr, nullptr, st));
  HIPCHECK(boot_scan_ll(s.temp.p, scan_bytes, s.cnt.p, off.p, m + 1, st));
  std::vector<long long> cnt(m);
  long long total = 0;
  HIPCHECK(hipMemcpyAsync(cnt.data(), s.cnt.p, sizeof(long long) * m, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(&total, off.p + m, sizeof(long long), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  if (total > (long long)INT32_MAX) {
    h->last_error = "sicp_bootstrap: the radius neighbourhoods hold more than 2^31 entries";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  long long mx = 0;
  for (long long v : cnt) mx = std::max(mx, v);
  HIPCHECK(s.list.reserve((size_t)total + 1)); HIPCHECK(s.list2.reserve((size_t)total + 1));
  HIPCHECK(idx.reserve((size_t)total + 1)); HIPCHECK(d2.reserve((size_t)total + 1));
  HIPCHECK(launch_boot_radius(1, m, k.kx.p, k.ky.p, k.kz.p, inv_cell, s.key2.p, s.val2.p, r2, nullptr, off.p, s.list.p, st));
  bytes = 0;
  HIPCHECK(boot_segmented_sort(nullptr, bytes, s.list.p, s.list2.p, total, m, off.p, st));
  SICPCHECK(temp_reserve(h, s, bytes));
  HIPCHECK(boot_segmented_sort(s.temp.p, bytes, s.list.p, s.list2.p, total, m, off.p, st));
  HIPCHECK(launch_boot_split(total, s.list2.p, idx.p, d2.p, st));
  *total_out = total;
  *max_out = (int)mx;
  return SICP_OK;
}

// normals (normal radius) and FPFH (feature radius) of a keypoint cloud
int keypoint_features(sicp_context* h, const sicp_bootstrap_params& p, BootScratch& s, BootCloud& k) {
  const int m = k.n;
  if (m <= 0) return SICP_OK;
  const hipStream_t st = h->stream;
  HIPCHECK(k.n3.reserve((size_t)m * 3)); HIPCHECK(k.fpfh.reserve((size_t)m * 33)); HIPCHECK(s.spfh.reserve((size_t)m * 33));
  SICPCHECK(radius_lists(h, k, p.feature_radius, s, k.off, k.idx, k.d2, &k.n_nbrs, &k.max_nbrs));
  if (p.normal_radius == p.feature_radius) {
    HIPCHECK(launch_boot_normals(m, k.kx.p, k.ky.p, k.kz.p, k.off.p, k.idx.p, k.n3.p, st));
  } else {
    long long nt = 0;
    int nm = 0;
    SICPCHECK(radius_lists(h, k, p.normal_radius, s, s.noff, s.nidx, s.nd2, &nt, &nm));
    k.max_nbrs = std::max(k.max_nbrs, nm);
    HIPCHECK(launch_boot_normals(m, k.kx.p, k.ky.p, k.kz.p, s.noff.p, s.nidx.p, k.n3.p, st));
  }
  HIPCHECK(launch_boot_fpfh(m, k.kx.p, k.ky.p, k.kz.p, k.n3.p, k.off.p, k.idx.p, k.d2.p, s.spfh.p, k.fpfh.p, st));
  return SICP_OK;
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

// the truncated error of n hypotheses (rows 0..2 of their 4x4 matrices): one K = 1 search of every source keypoint per
// hypothesis on a box tree of the target keypoints, collected into job launches, then one reduction per batch
int score_hypotheses(sicp_context* h, const sicp_bootstrap_params& p, const BootCloud& S, const BootCloud& T, int n,
                     const double* M12, double* err) {
  const hipStream_t st = h->stream;
  BootParamsScope scope(h);
  std::shared_ptr<Cloud> qc = acquire_cloud(h->device), tc = acquire_cloud(h->device);
  const StridedCloud qs = {(const char*)S.hx.data(), (const char*)S.hy.data(), (const char*)S.hz.data(), nullptr, 4, 4};
  const StridedCloud ts = {(const char*)T.hx.data(), (const char*)T.hy.data(), (const char*)T.hz.data(), nullptr, 4, 4};
  SICPCHECK(stage_cloud(h, *qc, S.n, qs));
  qc->is_set = true; qc->layout = -1;
  SICPCHECK(prepare_cloud(h, *qc));
  SICPCHECK(stage_cloud(h, *tc, T.n, ts));
  tc->is_set = true; tc->layout = -1;
  SICPCHECK(prepare_cloud(h, *tc));
  SICPCHECK(cloud_wait(h, *qc));
  SICPCHECK(cloud_wait(h, *tc));
  const int nq = qc->n;
  const int batch = (int)std::max<long long>(1, std::min<long long>(n, (32ll << 20) / std::max(nq, 1)));
  DevBuf<int> oi;
  DevBuf<float> od;
  DevBuf<double> derr;
  HIPCHECK(oi.reserve((size_t)batch * nq)); HIPCHECK(od.reserve((size_t)batch * nq)); HIPCHECK(derr.reserve((size_t)n));
  const float inf = std::numeric_limits<float>::infinity();
  const double t = (double)(float)p.max_corr_distance;
  for (int b0 = 0; b0 < n; b0 += batch) {
    const int cnt = std::min(batch, n - b0);
    JobCollector jc;
    {
      CollectScope cs(h, &jc);
      for (int i = 0; i < cnt; ++i)
        SICPCHECK(run_nn(h, 1, *qc, 0, nq, M12 + 12 * (size_t)(b0 + i), *tc, 0, false, inf, oi.p + (size_t)i * nq,
                         od.p + (size_t)i * nq, 0, st));
    }
    HIPCHECK(sicp::launch_bvh_knn_packet_jobs(jc.knn_K[0], jc.knn[0].data(), (int)jc.knn[0].size(), st));
    HIPCHECK(launch_boot_error(cnt, nq, od.p, t, derr.p + b0, st));
  }
  HIPCHECK(hipMemcpyAsync(err, derr.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return SICP_OK;
}

// keypoints + features of both clouds and the feature k-NN of every source keypoint
struct BootState {
  BootCloud k[2];
  std::vector<int> knn;  // [n_source][k]
  int k_eff = 0;         // k clamped to the target keypoints with a feature
  std::vector<int> src_valid;
  int tgt_valid = 0;
};

int check_clouds(sicp_context* h) {
  if (!h->cl[0] || !h->cl[1] || !h->cloud(SICP_SOURCE).is_set || !h->cloud(SICP_TARGET).is_set) return SICP_ERR_NOT_READY;
  return SICP_OK;
}

int valid_flags(sicp_context* h, const BootCloud& k, std::vector<char>& ok) {
  std::vector<double> n3((size_t)k.n * 3);
  if (k.n > 0) HIPCHECK(hipMemcpyAsync(n3.data(), k.n3.p, sizeof(double) * n3.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  ok.resize(k.n);
  for (int i = 0; i < k.n; ++i) ok[i] = !std::isnan(n3[3 * (size_t)i]);
  return SICP_OK;
}

int prepare(sicp_context* h, const sicp_bootstrap_params& p, BootState& B, double* t_kp, double* t_feat, double* t_knn) {
  BootScratch s;
  double t0 = now_ms();
  for (int w = 0; w < 2; ++w) SICPCHECK(voxel_keypoints(h, h->cloud(w), p, s, B.k[w]));
  double t1 = now_ms();
  for (int w = 0; w < 2; ++w) SICPCHECK(keypoint_features(h, p, s, B.k[w]));
  HIPCHECK(hipStreamSynchronize(h->stream));
  double t2 = now_ms();
  std::vector<char> sv, tv;
  SICPCHECK(valid_flags(h, B.k[0], sv));
  SICPCHECK(valid_flags(h, B.k[1], tv));
  B.src_valid.clear();
  for (int i = 0; i < B.k[0].n; ++i)
    if (sv[i]) B.src_valid.push_back(i);
  B.tgt_valid = 0;
  for (char v : tv) B.tgt_valid += v;
  const int k = p.k_correspondences;
  B.k_eff = std::min(k, B.tgt_valid);
  const int ns = B.k[0].n;
  B.knn.assign((size_t)ns * k, -1);
  if (ns > 0 && B.k[1].n > 0) {
    DevBuf<int> dk;
    HIPCHECK(dk.reserve((size_t)ns * k));
    HIPCHECK(launch_boot_feature_knn(ns, B.k[0].fpfh.p, B.k[1].n, B.k[1].fpfh.p, k, dk.p, h->stream));
    HIPCHECK(hipMemcpyAsync(B.knn.data(), dk.p, sizeof(int) * B.knn.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  double t3 = now_ms();
  if (t_kp) *t_kp = t1 - t0;
  if (t_feat) *t_feat = t2 - t1;
  if (t_knn) *t_knn = t3 - t2;
  return SICP_OK;
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

int bootstrap_run(sicp_context* h, const sicp_bootstrap_params* pp, double* out_qt, sicp_bootstrap_info* info) {
  if (!pp || !out_qt) return SICP_ERR_INVALID_ARGUMENT;
  const sicp_bootstrap_params p = *pp;
  SICPCHECK(check_params(h, p));
  SICPCHECK(set_device(h));
  SICPCHECK(check_clouds(h));
  const double t_begin = now_ms();
  BootState B;
  double t_kp = 0, t_feat = 0, t_knn = 0;
  SICPCHECK(prepare(h, p, B, &t_kp, &t_feat, &t_knn));
  const int ns = B.k[0].n, nr = p.nr_samples;
  if ((int)B.src_valid.size() < nr || B.tgt_valid < 1) {
    h->last_error = "sicp_bootstrap: " + std::to_string(B.src_valid.size()) + " source / " + std::to_string(B.tgt_valid) +
                    " target keypoints with features";
    return SICP_ERR_TOO_FEW_POINTS;
  }
  // SampleConsensusInitialAlignment::computeTransformation: per iteration selectSamples, then one random feature
  // neighbour per sample (findSimilarFeatures), then the rigid transform of the pairs
  const double tm0 = now_ms();
  const int iters = p.max_iterations, k = p.k_correspondences;
  std::vector<double> M((size_t)iters * 12), Q((size_t)iters * 4);
  BootRng rng{p.seed};
  const int nv = (int)B.src_valid.size();
  const BootCloud &S = B.k[0], &T = B.k[1];
  std::vector<int> smp(nr);
  double sp[3 * kBootMaxSamples], tp[3 * kBootMaxSamples];
  for (int it = 0; it < iters; ++it) {
    int got = 0, fails = 0;
    float min_d = (float)p.min_sample_distance;
    const int max_fails = 3 * nv;
    while (got < nr) {
      const int si = B.src_valid[rng.index(nv)];
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
      const int tj = B.knn[(size_t)smp[j] * k + rng.index(B.k_eff)];
      sp[3 * j] = S.hx[smp[j]]; sp[3 * j + 1] = S.hy[smp[j]]; sp[3 * j + 2] = S.hz[smp[j]];
      tp[3 * j] = T.hx[tj]; tp[3 * j + 1] = T.hy[tj]; tp[3 * j + 2] = T.hz[tj];
    }
    rigid_from_pairs(nr, sp, tp, &Q[(size_t)it * 4], &M[(size_t)it * 12]);
  }
  const double tm1 = now_ms();
  std::vector<double> err(iters);
  SICPCHECK(score_hypotheses(h, p, S, T, iters, M.data(), err.data()));
  int best = 0;
  for (int it = 1; it < iters; ++it)
    if (err[it] < err[best]) best = it;
  const double* q = &Q[(size_t)best * 4];
  out_qt[0] = q[1]; out_qt[1] = q[2]; out_qt[2] = q[3]; out_qt[3] = q[0];
  out_qt[4] = M[(size_t)best * 12 + 3]; out_qt[5] = M[(size_t)best * 12 + 7]; out_qt[6] = M[(size_t)best * 12 + 11];
  if (info) {
    info->n_source_keypoints = ns;
    info->n_target_keypoints = T.n;
    info->max_neighbours = std::max(S.max_nbrs, T.max_nbrs);
    info->best_iteration = best;
    info->best_error = err[best];
    info->t_keypoints_ms = t_kp;
    info->t_features_ms = t_feat;
    info->t_match_ms = t_knn + (tm1 - tm0);
    info->t_score_ms = now_ms() - tm1;
    info->t_total_ms = now_ms() - t_begin;
  }
  return SICP_OK;
}

int bootstrap_keypoints(sicp_context* h, int which, const sicp_bootstrap_params* pp, int32_t capacity, int64_t nbr_capacity,
                        int32_t* n_keypoints, int64_t* n_nbrs, float* xyz3, double* normal3, float* fpfh33,
                        int64_t* nbr_offsets, int32_t* nbr_idx) {
  if (!pp || (which != SICP_SOURCE && which != SICP_TARGET)) return SICP_ERR_INVALID_ARGUMENT;
  const sicp_bootstrap_params p = *pp;
  SICPCHECK(check_params(h, p));
  SICPCHECK(set_device(h));
  SICPCHECK(check_clouds(h));
  BootScratch s;
  BootCloud k;
  SICPCHECK(voxel_keypoints(h, h->cloud(which), p, s, k));
  SICPCHECK(keypoint_features(h, p, s, k));
  HIPCHECK(hipStreamSynchronize(h->stream));
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
  if (normal3) HIPCHECK(hipMemcpyAsync(normal3, k.n3.p, sizeof(double) * 3 * m, hipMemcpyDeviceToHost, st));
  if (fpfh33) HIPCHECK(hipMemcpyAsync(fpfh33, k.fpfh.p, sizeof(float) * 33 * m, hipMemcpyDeviceToHost, st));
  if (nbr_offsets) HIPCHECK(hipMemcpyAsync(nbr_offsets, k.off.p, sizeof(long long) * (m + 1), hipMemcpyDeviceToHost, st));
  if (nbr_idx && k.n_nbrs > 0) HIPCHECK(hipMemcpyAsync(nbr_idx, k.idx.p, sizeof(int) * k.n_nbrs, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return SICP_OK;
}

int bootstrap_score(sicp_context* h, const sicp_bootstrap_params* pp, int32_t n, const int32_t* src_idx, const int32_t* tgt_idx,
                    double* M12, double* err, int32_t knn_capacity, int32_t* feat_knn) {
  if (!pp || n < 0 || (n > 0 && (!src_idx || !tgt_idx || !err))) return SICP_ERR_INVALID_ARGUMENT;
  const sicp_bootstrap_params p = *pp;
  SICPCHECK(check_params(h, p));
  SICPCHECK(set_device(h));
  SICPCHECK(check_clouds(h));
  BootState B;
  SICPCHECK(prepare(h, p, B, nullptr, nullptr, nullptr));
  const BootCloud &S = B.k[0], &T = B.k[1];
  if (feat_knn) {
    if ((long long)knn_capacity < (long long)S.n * p.k_correspondences) return SICP_ERR_INVALID_ARGUMENT;
    std::memcpy(feat_knn, B.knn.data(), sizeof(int) * B.knn.size());
  }
  if (n == 0) return SICP_OK;
  if (S.n < 1 || T.n < 1) return SICP_ERR_TOO_FEW_POINTS;
  const int nr = p.nr_samples;
  std::vector<double> M((size_t)n * 12);
  double sp[3 * kBootMaxSamples], tp[3 * kBootMaxSamples], q[4];
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < nr; ++j) {
      const int a = src_idx[(size_t)i * nr + j], b = tgt_idx[(size_t)i * nr + j];
      if (a < 0 || a >= S.n || b < 0 || b >= T.n) {
        h->last_error = "sicp_bootstrap_score: sample " + std::to_string(i) + " names a keypoint that does not exist";
        return SICP_ERR_INVALID_ARGUMENT;
      }
      sp[3 * j] = S.hx[a]; sp[3 * j + 1] = S.hy[a]; sp[3 * j + 2] = S.hz[a];
      tp[3 * j] = T.hx[b]; tp[3 * j + 1] = T.hy[b]; tp[3 * j + 2] = T.hz[b];
    }
    rigid_from_pairs(nr, sp, tp, q, &M[(size_t)i * 12]);
  }
  SICPCHECK(score_hypotheses(h, p, S, T, n, M.data(), err));
  if (M12) std::memcpy(M12, M.data(), sizeof(double) * M.size());
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
