// filter.cpp -- sicp_filter (include/sicp.h, "filtering a cloud"): the cloud's own search trees give every point its distance
// list (run_nn, per label segment on a grouped cloud, merged by value), then the kernels of filter_kernels.hip -- classes, mean
// distances, the tree sums and the threshold, the radius count on the cluster's cell grid, flags, a scan, a gather -- one
// read-back of counts and per-point outputs and, with dst, one of the kept points, staged into dst's slot through the path of
// sicp_set_cloud.  Without dst nothing the handle holds for align() is touched: the call reads the cloud and its trees and
// writes scratch of its own; the searches' counters are given back.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

// A call's device scratch: taken from the arena, given back at the end (DevArena::release_scratch: `idle` once the stream
// has been synchronised behind the call's launches).
struct FilterScratch {
  DevBuf<unsigned char> temp, cls, mask, okeep;
  DevBuf<unsigned long long> k0, k1;
  DevBuf<int> caller, idx, val, sval, flag, pos, heads, parent, size, nb, onb, gres, res;
  DevBuf<float> list, list2, ox, oy, oz;
  DevBuf<float4> spt;
  DevBuf<uint32_t> ol;
  DevBuf<double> omd, part1, part2;
  DevBuf<sicp::FilterStats> stats;
  int device = -1;
  bool idle = true;
  ~FilterScratch() {
    DevArena::release_scratch(device, idle, temp, cls, mask, okeep, k0, k1, caller, idx, val, sval, flag, pos, heads, parent, size, nb, onb,
                              gres, res, list, list2, ox, oy, oz, spt, ol, omd, part1, part2, stats);
  }
};

bool slot_ok(int which) { return which == SICP_SOURCE || which == SICP_TARGET; }
size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

void filter_default_params(sicp_filter_params* p) {
  std::memset(p, 0, sizeof *p);
  p->mean_k = 20;
  p->std_mul = 2.0;
  p->radius = 0.0;
  p->min_neighbors = 2;
}

int filter(sicp_context* h, int which, const sicp_filter_params* p, const uint8_t* mask, sicp_context* dst, int dst_which, uint8_t* keep,
           double* mean_dist, int32_t* neighbors, sicp_filter_info* info) {
  if (!h) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    h->last_error = "sicp_filter: " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  auto too_few = [&](const std::string& why) {
    h->last_error = "sicp_filter: " + why;
    return SICP_ERR_TOO_FEW_POINTS;
  };
  if (!p) return refuse("the params are NULL");
  if (!slot_ok(which)) return refuse("which is neither SICP_SOURCE nor SICP_TARGET");
  if (dst && !slot_ok(dst_which)) return refuse("dst_which is neither SICP_SOURCE nor SICP_TARGET");
  if (dst && dst->device != h->device) return refuse("dst is on device " + std::to_string(dst->device) + ", the handle on " + std::to_string(h->device));
  if (p->mean_k < 0 || p->mean_k > 31) return refuse("mean_k must be in 0 .. 31 (0: the statistical test is off)");
  if (!std::isfinite(p->std_mul) || !(p->std_mul >= 0.0)) return refuse("std_mul must be finite and >= 0");
  if (!std::isfinite(p->radius) || !(p->radius >= 0.0)) return refuse("radius must be finite and >= 0 (0: the radius test is off)");
  const bool stat = p->mean_k > 0, rad = p->radius > 0.0;
  if (rad && p->min_neighbors < 1) return refuse("min_neighbors must be >= 1 when the radius test is on");
  if (p->n_drop < 0 || p->n_drop > SICP_FILTER_MAX_LABELS) return refuse("n_drop must be in 0 .. " + std::to_string(SICP_FILTER_MAX_LABELS));
  if (p->n_protect < 0 || p->n_protect > SICP_FILTER_MAX_LABELS) return refuse("n_protect must be in 0 .. " + std::to_string(SICP_FILTER_MAX_LABELS));
  for (int i = 0; i < p->n_drop; ++i)
    for (int k = 0; k < p->n_protect; ++k)
      if (p->drop[i] == p->protect[k]) return refuse("label " + std::to_string(p->drop[i]) + " is in both drop and protect");
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    h->last_error = "sicp_filter: the slot holds no cloud";
    return SICP_ERR_NOT_READY;
  }
  if (!c.has_label && (p->n_drop != 0 || p->n_protect != 0))
    return refuse("the cloud was set without labels: only empty drop and protect lists can filter it");
  const int n = c.n, nc = c.n_caller;
  const int K = p->mean_k + 1;
  if (stat && n < K)
    return too_few("the statistical test with mean_k = " + std::to_string(p->mean_k) + " needs " + std::to_string(K) + " finite points, the cloud has " + std::to_string(n));
  const double t_begin = now_ms();
  SICPCHECK(set_device(h));
  // the cloud's device copy and trees, in the layout they have (a cloud not yet indexed is prepared as the handle's next call would)
  if (c.layout < 0) SICPCHECK(prepare_cloud(h, c));
  SICPCHECK(cloud_wait(h, c));
  const bool labels = c.has_label, mapped = !c.keep.empty();
  hipStream_t st = h->stream;
  FilterScratch X;
  sicp::FilterArgs A;
  std::memset(&A, 0, sizeof A);
  int res[kFlRes] = {0, 0, 0, 0, 0, 0, 0, 0}, gres[kClRes] = {0, 0, 0, 0, 0, 0, 0, 0};
  sicp::FilterStats S;
  std::memset(&S, 0, sizeof S);
  // pinned: caller indices | mask on their way up; counts | grid counts | statistics | mean_dist | neighbors | keep on their way back
  const size_t m = (size_t)std::max(n, 1), mc = (size_t)std::max(nc, 1);
  const size_t o_caller = 0, o_mask = o_caller + up8(mapped ? 4 * m : 0), o_res = o_mask + up8(mask ? mc : 0), o_gres = o_res + sizeof res,
               o_stats = o_gres + sizeof gres, o_md = o_stats + up8(sizeof S), o_nb = o_md + 8 * mc, o_keep = o_nb + up8(4 * mc),
               o_end = o_keep + up8(mc);
  HIPCHECK(h->fl_stage.resize(o_end));
  unsigned char* o = h->fl_stage.data();
  if (nc > 0) {
    X.device = h->device;
    X.idle = false;
    HIPCHECK(X.cls.reserve(m)); HIPCHECK(X.okeep.reserve(mc)); HIPCHECK(X.omd.reserve(mc)); HIPCHECK(X.onb.reserve(mc));
    HIPCHECK(X.nb.reserve(m)); HIPCHECK(X.flag.reserve(m)); HIPCHECK(X.pos.reserve(m));
    HIPCHECK(X.ox.reserve(m)); HIPCHECK(X.oy.reserve(m)); HIPCHECK(X.oz.reserve(m));
    if (labels) HIPCHECK(X.ol.reserve(m));
    HIPCHECK(X.res.reserve(kFlRes)); HIPCHECK(X.gres.reserve(kClRes)); HIPCHECK(X.stats.reserve(1));
    size_t pair_bytes = 0, scan_bytes = 0;
    HIPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, std::max(n, 1), st));
    if (rad) {
      HIPCHECK(X.k0.reserve(m)); HIPCHECK(X.k1.reserve(m)); HIPCHECK(X.val.reserve(m)); HIPCHECK(X.sval.reserve(m));
      HIPCHECK(X.heads.reserve(m + 1)); HIPCHECK(X.parent.reserve(m)); HIPCHECK(X.size.reserve(m)); HIPCHECK(X.spt.reserve(m));
      HIPCHECK(sicp::prim_sort_pairs(nullptr, pair_bytes, X.k0.p, X.k1.p, X.val.p, X.sval.p, std::max(n, 1), 0, 64, st));
    }
    HIPCHECK(X.temp.reserve(std::max(pair_bytes, scan_bytes) + 256));

    A.n = n; A.n_caller = nc;
    A.labels = labels ? 1 : 0;
    A.mean_k = p->mean_k; A.min_neighbors = rad ? p->min_neighbors : 0;
    A.n_drop = p->n_drop; A.n_protect = p->n_protect;
    for (int k = 0; k < p->n_drop; ++k) A.drop[k] = p->drop[k];
    for (int k = 0; k < p->n_protect; ++k) A.protect[k] = p->protect[k];
    A.std_mul = p->std_mul;
    const float r = (float)p->radius;
    A.r2 = r * r;
    A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
    A.label = labels ? c.rl.p : nullptr;
    A.perm = c.d_perm.p;
    A.cls = X.cls.p;
    A.nb = X.nb.p; A.flag = X.flag.p; A.pos = X.pos.p;
    A.okeep = X.okeep.p; A.omd = X.omd.p; A.onb = X.onb.p;
    A.ox = X.ox.p; A.oy = X.oy.p; A.oz = X.oz.p; A.ol = labels ? X.ol.p : nullptr;
    A.stats = X.stats.p; A.res = X.res.p;
    if (mapped) {  // points were dropped: finite index -> caller index
      HIPCHECK(X.caller.reserve(m));
      std::memcpy(o + o_caller, c.keep.data(), 4 * (size_t)n);
      HIPCHECK(hipMemcpyAsync(X.caller.p, o + o_caller, 4 * (size_t)n, hipMemcpyHostToDevice, st));
      A.caller = X.caller.p;
    }
    if (mask) {
      HIPCHECK(X.mask.reserve(mc));
      std::memcpy(o + o_mask, mask, (size_t)nc);
      HIPCHECK(hipMemcpyAsync(X.mask.p, o + o_mask, (size_t)nc, hipMemcpyHostToDevice, st));
      A.mask = X.mask.p;
    }
    HIPCHECK(hipMemsetAsync(X.res.p, 0, sizeof res, st));
    HIPCHECK(hipMemsetAsync(X.gres.p, 0, sizeof gres, st));
    HIPCHECK(hipMemsetAsync(X.stats.p, 0, sizeof S, st));
    HIPCHECK(sicp::launch_filter_classes(A, st));

    if (stat) {
      // every point of the cloud, in device order, against every segment of its own trees -- the point itself is found, at
      // d2 = 0; a second segment's lists are merged into the first's, segment by segment: two lists per point
      if ((long long)n * K > 0x7fffffffll) return refuse("the cloud is too large for lists of mean_k + 1 entries per point");
      HIPCHECK(X.list.reserve(m * (size_t)K)); HIPCHECK(X.idx.reserve(m * (size_t)K));
      if (c.n_seg() > 1) HIPCHECK(X.list2.reserve(m * (size_t)K));
      A.list = X.list.p; A.list2 = X.list2.p; A.list_k = K;
      {
        StatsKeeper keep_stats(h);  // (the searches' counters and timers go back as they were)
        for (int ts = 0; ts < c.n_seg(); ++ts) {
          SICPCHECK(run_nn(h, K, c, 0, n, nullptr, c, ts, false, std::numeric_limits<float>::infinity(), X.idx.p,
                           ts == 0 ? X.list.p : X.list2.p, SICP_PROFILE_NN, st));
          if (ts > 0) HIPCHECK(sicp::launch_filter_merge_lists(A, st));
        }
      }
      HIPCHECK(sicp::launch_filter_mean_dist(A, st));
      // the tree sums: level by level until one workgroup holds what is left
      size_t part_n = 0;
      for (long long cnt = nc;;) {
        cnt = (cnt + sicp::kFilterTreeRun - 1) / sicp::kFilterTreeRun;
        part_n += (size_t)cnt;
        if (cnt == 1) break;
      }
      HIPCHECK(X.part1.reserve(part_n)); HIPCHECK(X.part2.reserve(part_n));
      const double *in1 = X.omd.p, *in2 = nullptr;
      size_t off = 0;
      for (int cnt = nc, first = 1;; first = 0) {
        const int blocks = (cnt + sicp::kFilterTreeRun - 1) / sicp::kFilterTreeRun;
        HIPCHECK(sicp::launch_filter_tree_sum(in1, in2, cnt, first, X.part1.p + off, X.part2.p + off, st));
        in1 = X.part1.p + off; in2 = X.part2.p + off;
        off += (size_t)blocks;
        cnt = blocks;
        if (blocks == 1) break;
      }
      HIPCHECK(sicp::launch_filter_threshold(A, in1, in2, st));
    }

    if (rad && n > 0) {
      // the cluster's grid with the radius as the tolerance and every finite point a vertex
      sicp::ClusterArgs G;
      std::memset(&G, 0, sizeof G);
      G.n = n;
      G.inv = cells_per_metre(r);
      G.t2 = A.r2;
      G.x = c.rx.p; G.y = c.ry.p; G.z = c.rz.p;
      G.key = X.k0.p; G.skey = X.k1.p; G.ckey = X.k0.p;  // (the unsorted keys are dead once sorted: cluster.cpp)
      G.val = X.val.p; G.sval = X.sval.p;
      G.flag = X.flag.p; G.pos = X.pos.p;
      G.heads = X.heads.p; G.spt = X.spt.p;
      G.parent = X.parent.p; G.size = X.size.p;
      G.res = X.gres.p;
      A.heads = X.heads.p; A.ckey = X.k0.p; A.spt = X.spt.p; A.sval = X.sval.p; A.grid_res = X.gres.p;
      HIPCHECK(hipMemsetAsync(X.nb.p, 0, 4 * (size_t)n, st));
      HIPCHECK(sicp::launch_cluster_keys(G, st));
      HIPCHECK(sicp::prim_sort_pairs(X.temp.p, pair_bytes, X.k0.p, X.k1.p, X.val.p, X.sval.p, n, 0, 64, st));
      HIPCHECK(sicp::launch_cluster_cell_flags(G, st));
      HIPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, n, st));
      HIPCHECK(sicp::launch_cluster_cells(G, st));
      if (A.r2 > 0.f) HIPCHECK(sicp::launch_filter_radius_count(A, st));  // (r2 = 0: d2 < r2 never holds)
    }

    if (n > 0) {
      HIPCHECK(sicp::launch_filter_flags(A, st));
      HIPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, n, st));
      HIPCHECK(sicp::launch_filter_gather(A, st));
    }
    HIPCHECK(hipMemcpyAsync(o + o_res, X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(o + o_gres, X.gres.p, sizeof gres, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(o + o_stats, X.stats.p, sizeof S, hipMemcpyDeviceToHost, st));
    if (mean_dist) HIPCHECK(hipMemcpyAsync(o + o_md, X.omd.p, 8 * (size_t)nc, hipMemcpyDeviceToHost, st));
    if (neighbors) HIPCHECK(hipMemcpyAsync(o + o_nb, X.onb.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, st));
    if (keep) HIPCHECK(hipMemcpyAsync(o + o_keep, X.okeep.p, (size_t)nc, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    std::memcpy(res, o + o_res, sizeof res);
    std::memcpy(gres, o + o_gres, sizeof gres);
    std::memcpy(&S, o + o_stats, sizeof S);
  }
  if (gres[kClRange]) {
    X.idle = true;
    return refuse("radius " + std::to_string(p->radius) + " is too small for the points: a cell coordinate of the search grid reaches 2^20 - 1");
  }
  if (stat && res[kFlTested] < 2) {
    X.idle = true;
    return too_few("the statistical test needs 2 tested points, the cloud has " + std::to_string(res[kFlTested]));
  }
  const int n_kept = res[kFlKept];
  if (dst && n_kept == 0) {
    X.idle = true;
    return too_few("the result is empty; dst keeps its cloud");
  }
  if (dst) {
    // the kept points -> pinned memory: all of them are on the host before dst's slot lets go of its old cloud (merge.cpp)
    const size_t mo = (size_t)n_kept;
    HIPCHECK(h->fl_out.resize(mo * 4));
    uint32_t* q = h->fl_out.data();
    HIPCHECK(hipMemcpyAsync(q, X.ox.p, 4 * mo, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(q + mo, X.oy.p, 4 * mo, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(q + 2 * mo, X.oz.p, 4 * mo, hipMemcpyDeviceToHost, st));
    if (labels) HIPCHECK(hipMemcpyAsync(q + 3 * mo, X.ol.p, 4 * mo, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    X.idle = true;
    const StridedCloud in = {(const char*)q, (const char*)(q + mo), (const char*)(q + 2 * mo), labels ? (const char*)(q + 3 * mo) : nullptr, 4, 4};
    const int rc = set_cloud_common(dst, dst_which, n_kept, in);  // (in place: `c` is the new cloud from here on)
    if (rc != SICP_OK) {
      if (dst != h) h->last_error = "sicp_filter: dst: " + dst->last_error;
      return rc;
    }
  }
  X.idle = true;
  if (nc > 0) {
    if (mean_dist) std::memcpy(mean_dist, o + o_md, 8 * (size_t)nc);
    if (neighbors) std::memcpy(neighbors, o + o_nb, 4 * (size_t)nc);
    if (keep) std::memcpy(keep, o + o_keep, (size_t)nc);
  }
  if (info) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    sicp_filter_info I;
    std::memset(&I, 0, sizeof I);
    I.n_points = nc;
    I.n_finite = n;
    I.n_tested = res[kFlTested];
    I.n_protected = res[kFlProtected];
    I.n_kept = n_kept;
    I.n_fail_stat = res[kFlFailStat];
    I.n_fail_radius = res[kFlFailRadius];
    I.mean = stat ? S.mean : nan;
    I.stddev = stat ? S.stddev : nan;
    I.threshold = stat ? S.threshold : nan;
    I.t_total_ms = now_ms() - t_begin;
    *info = I;
  }
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
