// cluster.cpp -- sicp_cluster (include/sicp.h, "objects of a labelled cloud"): the kernels of cluster_kernels.hip on the cloud's
// device copy -- cell keys, a stable sort, the pair pass into a union-find, component sizes, cluster numbers -- one read-back of
// the counts, then the per-cluster table and one read-back of the results.  Nothing the handle holds for align() is touched: the
// call reads the cloud's caller-order arrays (valid in every layout) and writes scratch of its own.
#include <cfloat>
#include <climits>

#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

// A call's device scratch: taken from the arena, given back at the end (DevArena::release_scratch: `idle` once the stream
// has been synchronised behind the call's launches).
struct ClusterScratch {
  DevBuf<unsigned char> temp;
  DevBuf<unsigned long long> k0, k1, k2, k3;
  DevBuf<int> val, sval, flag, pos, heads, parent, size, cid, res, ocount, ofirst;
  DevBuf<float4> spt;
  DevBuf<uint32_t> olabel;
  DevBuf<double> ocentroid;
  DevBuf<float> obmin, obmax;
  int device = -1;
  bool idle = true;
  ~ClusterScratch() {
    DevArena::release_scratch(device, idle, temp, k0, k1, k2, k3, val, sval, flag, pos, heads, parent, size, cid, res, ocount, ofirst, spt,
                              olabel, ocentroid, obmin, obmax);
  }
};

}  // namespace

// the largest float inv with inv * t <= 1, decided on the exact double product (cell_grid.hpp: the proof, step 2); 0 -- one
// cell for everything -- when no finite positive inverse exists
float cells_per_metre(float t) {
  if (!(t > 0.f) || !std::isfinite(t)) return 0.f;
  float inv = (float)(1.0 / (double)t);
  if (!std::isfinite(inv)) return 0.f;
  while ((double)inv * (double)t > 1.0) inv = std::nextafterf(inv, 0.f);
  return inv;
}

void cluster_default_params(sicp_cluster_params* p) {
  std::memset(p, 0, sizeof *p);
  p->tolerance = 0.5;
  p->min_points = 10;
  p->max_points = 0;
  p->same_label = 1;
  p->n_ignore = 0;
}

int cluster(sicp_context* h, int which, const sicp_cluster_params* p, int32_t* cluster_id, int32_t capacity, uint32_t* label,
            int32_t* count, int32_t* first_index, double* centroid, float* bbox_min, float* bbox_max, sicp_cluster_info* info) {
  if (!h) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    h->last_error = "sicp_cluster: " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!p) return refuse("the params are NULL");
  if (which != SICP_SOURCE && which != SICP_TARGET) return refuse("which is neither SICP_SOURCE nor SICP_TARGET");
  if (!std::isfinite(p->tolerance) || !(p->tolerance > 0.0)) return refuse("tolerance must be finite and > 0");
  if (p->min_points < 1) return refuse("min_points must be >= 1");
  if (p->max_points < 0) return refuse("max_points must be >= 0 (0: no limit)");
  if (p->max_points > 0 && p->max_points < p->min_points) return refuse("max_points is below min_points");
  if (p->same_label != 0 && p->same_label != 1) return refuse("same_label must be 0 or 1");
  if (p->n_ignore < 0 || p->n_ignore > SICP_CLUSTER_MAX_IGNORE) return refuse("n_ignore must be in 0 .. " + std::to_string(SICP_CLUSTER_MAX_IGNORE));
  if (capacity < 0) return refuse("capacity must be >= 0");
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    h->last_error = "sicp_cluster: the slot holds no cloud";
    return SICP_ERR_NOT_READY;
  }
  if (!c.has_label && (p->same_label != 0 || p->n_ignore != 0))
    return refuse("the cloud was set without labels: only same_label = 0 with n_ignore = 0 can cluster it");
  const double t_begin = now_ms();
  SICPCHECK(set_device(h));
  // the cloud's device copy: the finite points in caller order (Cloud::rx ..., valid in every layout), prepared as a merge part is
  if (c.layout < 0) SICPCHECK(prepare_cloud(h, c));
  SICPCHECK(cloud_wait(h, c));
  const int n = c.n;
  const bool labels = c.has_label, vote = labels && p->same_label == 0;
  const bool want_table = label || count || first_index || centroid || bbox_min || bbox_max;
  const float t = (float)p->tolerance;
  int res[kClRes] = {0, 0, 0, 0, 0, 0, 0, 0};
  ClusterScratch X;
  hipStream_t st = h->stream;
  sicp::ClusterArgs A;
  std::memset(&A, 0, sizeof A);
  size_t sort_bytes = 0;
  if (n > 0) {
    const size_t m = (size_t)n;
    X.device = h->device;
    X.idle = false;
    HIPCHECK(X.k0.reserve(m)); HIPCHECK(X.k1.reserve(m));
    if (vote) { HIPCHECK(X.k2.reserve(m)); HIPCHECK(X.k3.reserve(m)); }
    HIPCHECK(X.val.reserve(m)); HIPCHECK(X.sval.reserve(m)); HIPCHECK(X.flag.reserve(m)); HIPCHECK(X.pos.reserve(m));
    HIPCHECK(X.heads.reserve(m + 1)); HIPCHECK(X.parent.reserve(m)); HIPCHECK(X.size.reserve(m)); HIPCHECK(X.cid.reserve(m));
    HIPCHECK(X.spt.reserve(m));
    HIPCHECK(X.res.reserve(kClRes));
    size_t pair_bytes = 0, scan_bytes = 0;
    HIPCHECK(sicp::prim_sort_pairs(nullptr, pair_bytes, X.k0.p, X.k1.p, X.val.p, X.sval.p, n, 0, 64, st));
    HIPCHECK(sicp::prim_sort_keys(nullptr, sort_bytes, X.k1.p, X.k0.p, n, 0, 64, st));
    HIPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, n, st));
    HIPCHECK(X.temp.reserve(std::max(std::max(pair_bytes, sort_bytes), scan_bytes) + 256));

    A.n = n;
    A.same_label = p->same_label; A.labels = labels ? 1 : 0;
    A.n_ignore = p->n_ignore;
    A.min_points = p->min_points; A.max_points = p->max_points > 0 ? p->max_points : INT_MAX;
    A.inv = cells_per_metre(t);
    A.t2 = t * t;
    for (int k = 0; k < p->n_ignore; ++k) A.ignore[k] = p->ignore[k];
    A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
    A.label = labels ? c.rl.p : nullptr;
    // the unsorted cell keys are dead once sorted and the sorted ones once the cells are formed: the cells' keys, then the
    // sorted member keys, take the first buffer, the member keys the second
    A.key = X.k0.p; A.skey = X.k1.p; A.ckey = X.k0.p;
    A.mkey = X.k1.p; A.msorted = X.k0.p;
    A.lkey = vote ? X.k2.p : nullptr; A.lsorted = vote ? X.k3.p : nullptr;
    A.val = X.val.p; A.sval = X.sval.p;
    A.flag = X.flag.p; A.pos = X.pos.p;
    A.heads = X.heads.p; A.mheads = X.heads.p;  // (the cells' heads are dead behind the pair pass)
    A.spt = X.spt.p;
    A.parent = X.parent.p; A.size = X.size.p; A.cid = X.cid.p;
    A.res = X.res.p;

    HIPCHECK(hipMemsetAsync(X.res.p, 0, sizeof res, st));
    HIPCHECK(sicp::launch_cluster_keys(A, st));
    // (all 64 bits: the non-vertices' key ~0 sorts them behind every cell; stable, so the indices ascend inside a cell)
    HIPCHECK(sicp::prim_sort_pairs(X.temp.p, pair_bytes, X.k0.p, X.k1.p, X.val.p, X.sval.p, n, 0, 64, st));
    HIPCHECK(sicp::launch_cluster_cell_flags(A, st));
    HIPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, n, st));
    HIPCHECK(sicp::launch_cluster_cells(A, st));
    if (A.t2 > 0.f) HIPCHECK(sicp::launch_cluster_pairs(A, st));  // (t2 = 0: d2 < t2 never holds)
    HIPCHECK(sicp::launch_cluster_sizes(A, st));
    HIPCHECK(sicp::launch_cluster_root_flags(A, st));
    HIPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, n, st));
    HIPCHECK(sicp::launch_cluster_ids(A, st));
    HIPCHECK(h->cl_stage.resize(sizeof res));
    HIPCHECK(hipMemcpyAsync(h->cl_stage.data(), X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    std::memcpy(res, h->cl_stage.data(), sizeof res);
  }
  if (res[kClRange]) {
    X.idle = true;
    return refuse("tolerance " + std::to_string(p->tolerance) + " is too small for the points: a cell coordinate of the search grid reaches 2^20 - 1");
  }
  const int nc = res[kClClusters];
  sicp_cluster_info I;
  std::memset(&I, 0, sizeof I);
  I.n_points = c.n_caller;
  I.n_kept = res[kClKept];
  I.n_components = res[kClComponents];
  I.n_clustered = res[kClClustered];
  I.n_clusters = nc;
  I.max_cluster_points = res[kClMaxCount];
  if (want_table && capacity < nc) {
    X.idle = true;
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    h->last_error = "sicp_cluster: there are " + std::to_string(nc) + " clusters, the table arrays hold " + std::to_string(capacity);
    return SICP_ERR_INVALID_ARGUMENT;
  }
  // pinned: centroid | cluster_id by finite index | label | count | first | bbox_min | bbox_max
  const size_t m = (size_t)n, k = (size_t)nc;
  const bool table = want_table && nc > 0, ids = cluster_id != nullptr && n > 0;
  const size_t o_cen = 0, o_cid = o_cen + 24 * k, o_lab = o_cid + 4 * m, o_cnt = o_lab + 4 * k, o_first = o_cnt + 4 * k,
               o_min = o_first + 4 * k, o_max = o_min + 12 * k, o_end = o_max + 12 * k;
  if (table || ids) {
    HIPCHECK(h->cl_stage.resize(o_end));
    unsigned char* o = h->cl_stage.data();
    if (table) {
      HIPCHECK(X.olabel.reserve(k)); HIPCHECK(X.ocount.reserve(k)); HIPCHECK(X.ofirst.reserve(k));
      HIPCHECK(X.ocentroid.reserve(3 * k)); HIPCHECK(X.obmin.reserve(3 * k)); HIPCHECK(X.obmax.reserve(3 * k));
      A.olabel = X.olabel.p; A.ocount = X.ocount.p; A.ofirst = X.ofirst.p;
      A.ocentroid = X.ocentroid.p; A.obmin = X.obmin.p; A.obmax = X.obmax.p;
      HIPCHECK(sicp::prim_sort_keys(X.temp.p, sort_bytes, A.mkey, A.msorted, n, 0, 64, st));
      if (vote) HIPCHECK(sicp::prim_sort_keys(X.temp.p, sort_bytes, A.lkey, A.lsorted, n, 0, 64, st));
      HIPCHECK(sicp::launch_cluster_member_heads(A, st));
      HIPCHECK(sicp::launch_cluster_table(A, nc, st));
      HIPCHECK(hipMemcpyAsync(o + o_cen, X.ocentroid.p, 24 * k, hipMemcpyDeviceToHost, st));
      HIPCHECK(hipMemcpyAsync(o + o_lab, X.olabel.p, 4 * k, hipMemcpyDeviceToHost, st));
      HIPCHECK(hipMemcpyAsync(o + o_cnt, X.ocount.p, 4 * k, hipMemcpyDeviceToHost, st));
      HIPCHECK(hipMemcpyAsync(o + o_first, X.ofirst.p, 4 * k, hipMemcpyDeviceToHost, st));
      HIPCHECK(hipMemcpyAsync(o + o_min, X.obmin.p, 12 * k, hipMemcpyDeviceToHost, st));
      HIPCHECK(hipMemcpyAsync(o + o_max, X.obmax.p, 12 * k, hipMemcpyDeviceToHost, st));
    }
    if (ids) HIPCHECK(hipMemcpyAsync(o + o_cid, X.cid.p, 4 * m, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
  }
  X.idle = true;
  const unsigned char* o = h->cl_stage.data();
  if (cluster_id) {
    // device index i is the i-th finite point; keep[i] is its caller index (empty: nothing was dropped)
    if (c.keep.empty() && n == c.n_caller) {
      if (n > 0) std::memcpy(cluster_id, o + o_cid, 4 * m);
    } else {
      const int32_t* d = reinterpret_cast<const int32_t*>(o + o_cid);
      for (int i = 0; i < c.n_caller; ++i) cluster_id[i] = -1;
      for (int i = 0; i < n; ++i) cluster_id[c.keep[(size_t)i]] = d[i];
    }
  }
  if (table) {
    if (centroid) std::memcpy(centroid, o + o_cen, 24 * k);
    if (label) std::memcpy(label, o + o_lab, 4 * k);
    if (count) std::memcpy(count, o + o_cnt, 4 * k);
    if (first_index) {
      const int32_t* d = reinterpret_cast<const int32_t*>(o + o_first);
      for (size_t j = 0; j < k; ++j) first_index[j] = c.keep.empty() ? d[j] : c.keep[(size_t)d[j]];
    }
    if (bbox_min) std::memcpy(bbox_min, o + o_min, 12 * k);
    if (bbox_max) std::memcpy(bbox_max, o + o_max, 12 * k);
  }
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
