// merge.cpp -- sicp_merge_clouds (include/sicp.h): the finite points of several handles' clouds, each at its pose, cropped
// about a centre and reduced on an absolute voxel grid to one cloud -- the kernels of merge_kernels.hip on the parts' device
// copies, one read-back of the counts, one of the result -- and, when asked, staged into a handle's slot through the path of
// sicp_set_cloud.  Nothing a part holds for align() is touched: its layout, features, correspondences and statistics stay.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

// A call's device scratch: taken from the arena, given back at the end (DevArena::release_scratch: `idle` once the stream
// has been synchronised behind the call's launches).
struct MergeScratch {
  DevBuf<unsigned char> args, temp;
  DevBuf<float> tx, ty, tz, gx, gy, gz, ox, oy, oz;
  DevBuf<uint32_t> tl, ol, oc;
  DevBuf<unsigned long long> key, key2;
  DevBuf<int> val, val2, flag, pos, heads, res;
  int device = -1;
  bool idle = true;
  ~MergeScratch() {
    DevArena::release_scratch(device, idle, args, temp, tx, ty, tz, gx, gy, gz, ox, oy, oz, tl, ol, oc, key, key2, val, val2, flag, pos, heads, res);
  }
};

bool slot_ok(int which) { return which == SICP_SOURCE || which == SICP_TARGET; }

}  // namespace

void merge_default_params(sicp_merge_params* p) {
  std::memset(p, 0, sizeof *p);
  p->leaf_size = 0.2;
  p->crop_range = 0.0;
}

int merge_clouds(sicp_handle* parts, const int32_t* part_which, int32_t n_parts, const double* qt, const sicp_merge_params* p,
                 sicp_context* dst, int dst_which, int32_t capacity, float* x, float* y, float* z, uint32_t* label, uint32_t* count,
                 sicp_merge_info* info) {
  if (!parts || n_parts < 1 || !parts[0]) return SICP_ERR_INVALID_ARGUMENT;
  sicp_context* h = parts[0];  // leads: its stream runs the kernels, it takes the error text
  auto refuse = [&](const std::string& why) {
    h->last_error = "sicp_merge_clouds: " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!part_which) return refuse("part_which is NULL");
  if (!p) return refuse("the params are NULL");
  for (int i = 0; i < n_parts; ++i) {
    if (!parts[i]) return refuse("handle " + std::to_string(i) + " is NULL");
    if (!slot_ok(part_which[i])) return refuse("part_which[" + std::to_string(i) + "] is neither SICP_SOURCE nor SICP_TARGET");
    if (parts[i]->device != h->device)
      return refuse("handle " + std::to_string(i) + " is on device " + std::to_string(parts[i]->device) + ", handle 0 on " + std::to_string(h->device));
  }
  if (dst && !slot_ok(dst_which)) return refuse("dst_which is neither SICP_SOURCE nor SICP_TARGET");
  if (dst && dst->device != h->device) return refuse("dst is on device " + std::to_string(dst->device) + ", handle 0 on " + std::to_string(h->device));
  if (!(p->leaf_size >= 0.0) || !std::isfinite(p->leaf_size)) return refuse("leaf_size must be finite and >= 0");
  if (!(p->crop_range >= 0.0)) return refuse("crop_range must be >= 0 (+inf is allowed)");
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(p->crop_center[d])) return refuse("crop_center must be finite");
  if (qt)
    for (size_t k = 0; k < 7 * (size_t)n_parts; ++k)
      if (!std::isfinite(qt[k])) return refuse("pose " + std::to_string(k / 7) + " is not finite");
  long long n_in = 0;
  int labelled = 0;
  for (int i = 0; i < n_parts; ++i) {
    const Cloud& c = parts[i]->cloud(part_which[i]);
    if (!c.is_set) {
      h->last_error = "sicp_merge_clouds: part " + std::to_string(i) + " has no cloud";
      return SICP_ERR_NOT_READY;
    }
    n_in += c.n;
    labelled += c.has_label ? 1 : 0;
  }
  if (labelled != 0 && labelled != n_parts) return refuse("some parts have labels and some have none");
  if (n_in > 0x7fffffffll) return refuse("the parts hold more than 2^31 - 1 points");
  const bool has_label = labelled != 0, voxel = p->leaf_size > 0.0, crop = p->crop_range > 0.0;
  const double t_begin = now_ms();
  SICPCHECK(set_device(h));
  // the parts' device copies: the finite points in caller order (Cloud::rx ..., valid in every layout).  A part that is
  // already on the device is neither uploaded nor laid out again, whatever its handle's mode; one that is not yet indexed is
  // prepared as its handle's next call would prepare it.
  for (int i = 0; i < n_parts; ++i) {
    Cloud& c = parts[i]->cloud(part_which[i]);
    if (c.layout < 0) {
      const int rc = prepare_cloud(parts[i], c);
      if (rc != SICP_OK) {
        if (parts[i] != h) h->last_error = "sicp_merge_clouds: part " + std::to_string(i) + ": " + parts[i]->last_error;
        return rc;
      }
    }
    SICPCHECK(cloud_wait(h, c));
  }
  const int n = (int)n_in;
  int res[kMergeRes] = {0, 0, 0, 0};
  MergeScratch X;
  hipStream_t st = h->stream;
  static const bool log_env = debug_enabled() && std::getenv("SICP_MERGE_LOG") != nullptr;
  StageLog log(log_env, st);
  if (n > 0) {
    const size_t m = (size_t)n;
    sicp::JobTable<sicp::MergePart> tab;  // (a part without points stays in it: it owns no workgroup)
    const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
    int off = 0;
    for (int i = 0; i < n_parts; ++i) {
      const Cloud& c = parts[i]->cloud(part_which[i]);
      sicp::MergePart P;
      std::memset(&P, 0, sizeof P);
      P.x = c.rx.p; P.y = c.ry.p; P.z = c.rz.p;
      P.label = has_label ? c.rl.p : nullptr;
      matrix34(qt ? qt + 7 * (size_t)i : ident, P.M);
      P.n = c.n; P.off = off;
      off += c.n;
      tab.add(P, (c.n + 255) / 256);
    }
    const size_t arg_bytes = tab.bytes();
    HIPCHECK(h->mg_stage.resize(arg_bytes + sizeof res));  // behind the table: the counts' read-back
    X.device = h->device;
    X.idle = false;
    HIPCHECK(X.args.reserve(arg_bytes));
    tab.pack(h->mg_stage.data(), X.args.p);
    HIPCHECK(X.tx.reserve(m)); HIPCHECK(X.ty.reserve(m)); HIPCHECK(X.tz.reserve(m));
    HIPCHECK(X.gx.reserve(m)); HIPCHECK(X.gy.reserve(m)); HIPCHECK(X.gz.reserve(m));
    HIPCHECK(X.ox.reserve(m)); HIPCHECK(X.oy.reserve(m)); HIPCHECK(X.oz.reserve(m));
    HIPCHECK(X.oc.reserve(m));
    if (has_label) { HIPCHECK(X.tl.reserve(m)); HIPCHECK(X.ol.reserve(m)); }
    HIPCHECK(X.key.reserve(m)); HIPCHECK(X.key2.reserve(m));
    HIPCHECK(X.val.reserve(m)); HIPCHECK(X.val2.reserve(m));
    HIPCHECK(X.flag.reserve(m)); HIPCHECK(X.pos.reserve(m)); HIPCHECK(X.heads.reserve(m));
    HIPCHECK(X.res.reserve(kMergeRes));
    const int begin_bit = voxel ? 0 : 63;  // without a grid the keys are 0 and ~0: one bit decides
    size_t pair_bytes = 0, key_bytes = 0, scan_bytes = 0;
    HIPCHECK(sicp::prim_sort_pairs(nullptr, pair_bytes, X.key.p, X.key2.p, X.val.p, X.val2.p, n, begin_bit, 64, st));
    HIPCHECK(sicp::prim_sort_keys(nullptr, key_bytes, X.key.p, X.key2.p, n, 0, 64, st));
    HIPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, n, st));
    HIPCHECK(X.temp.reserve(std::max(std::max(pair_bytes, key_bytes), scan_bytes) + 256));

    sicp::MergeKeyArgs K;
    K.parts = tab.d_jobs();
    K.blk_end = tab.d_end();
    K.n_parts = n_parts;
    K.voxel = voxel ? 1 : 0; K.crop = crop ? 1 : 0;
    K.inv_leaf = voxel ? 1.0f / (float)p->leaf_size : 0.f;
    K.cx = (float)p->crop_center[0]; K.cy = (float)p->crop_center[1]; K.cz = (float)p->crop_center[2];
    K.range_sq = p->crop_range * p->crop_range;
    K.tx = X.tx.p; K.ty = X.ty.p; K.tz = X.tz.p;
    K.tlabel = has_label ? X.tl.p : nullptr;
    K.key = X.key.p; K.val = X.val.p; K.res = X.res.p;
    sicp::MergeReduceArgs R;
    R.n = n; R.voxel = K.voxel; R.labels = has_label ? 1 : 0;
    R.skey = X.key2.p; R.sval = X.val2.p;
    R.flag = X.flag.p; R.pos = X.pos.p; R.heads = X.heads.p;
    R.tx = X.tx.p; R.ty = X.ty.p; R.tz = X.tz.p; R.tlabel = K.tlabel;
    R.gx = X.gx.p; R.gy = X.gy.p; R.gz = X.gz.p;
    // the unsorted keys are dead once sorted, the sorted ones once gathered: the (rank, label) keys take their places
    R.lkey = X.key.p;
    R.lsorted = voxel ? X.key2.p : X.key.p;
    R.ox = X.ox.p; R.oy = X.oy.p; R.oz = X.oz.p;
    R.olabel = has_label ? X.ol.p : nullptr; R.ocount = X.oc.p;
    R.res = X.res.p;

    log.mark("begin");
    HIPCHECK(hipMemcpyAsync(X.args.p, h->mg_stage.data(), arg_bytes, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(X.res.p, 0, sizeof res, st));
    HIPCHECK(sicp::launch_merge_keys(K, tab.blocks, st));
    log.mark("key");
    HIPCHECK(sicp::prim_sort_pairs(X.temp.p, pair_bytes, X.key.p, X.key2.p, X.val.p, X.val2.p, n, begin_bit, 64, st));
    log.mark("sort");
    HIPCHECK(sicp::launch_merge_heads(R, st));
    HIPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, n, st));
    HIPCHECK(sicp::launch_merge_gather(R, st));
    log.mark("compact_gather");
    HIPCHECK(sicp::launch_merge_centroids(R, st));
    log.mark("centroid");
    if (has_label) {
      if (voxel) HIPCHECK(sicp::prim_sort_keys(X.temp.p, key_bytes, X.key.p, X.key2.p, n, 0, 64, st));
      HIPCHECK(sicp::launch_merge_labels(R, st));
      log.mark("label");
    }
    int* h_res = reinterpret_cast<int*>(h->mg_stage.data() + arg_bytes);
    HIPCHECK(hipMemcpyAsync(h_res, X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    std::memcpy(res, h_res, sizeof res);
  }
  if (res[kMergeRange]) {
    X.idle = true;
    return refuse("leaf size " + std::to_string(p->leaf_size) + " is too small for the points: a voxel coordinate reaches 2^20");
  }
  const int n_out = res[kMergeOut];
  sicp_merge_info I;
  std::memset(&I, 0, sizeof I);
  I.n_in = n_in;
  I.n_kept = res[kMergeKept];
  I.n_out = n_out;
  I.max_voxel_points = res[kMergeMaxCount];
  I.has_label = has_label ? 1 : 0;
  const bool want_arrays = x || y || z || label || count;
  if (want_arrays && capacity < n_out) {
    X.idle = true;
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    h->last_error = "sicp_merge_clouds: the result has " + std::to_string(n_out) + " points, the output arrays hold " + std::to_string(capacity);
    return SICP_ERR_INVALID_ARGUMENT;
  }
  if (dst && n_out == 0) {
    X.idle = true;
    h->last_error = "sicp_merge_clouds: the result is empty; dst keeps its cloud";
    return SICP_ERR_TOO_FEW_POINTS;
  }
  // the result -> pinned memory: the whole of it is on the host before dst's slot lets go of its old cloud
  const size_t mo = (size_t)n_out;
  if (n_out > 0 && (want_arrays || dst)) {
    HIPCHECK(h->mg_out.resize(mo * 5));
    uint32_t* o = h->mg_out.data();
    HIPCHECK(hipMemcpyAsync(o, X.ox.p, 4 * mo, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(o + mo, X.oy.p, 4 * mo, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(o + 2 * mo, X.oz.p, 4 * mo, hipMemcpyDeviceToHost, st));
    if (has_label) HIPCHECK(hipMemcpyAsync(o + 3 * mo, X.ol.p, 4 * mo, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(o + 4 * mo, X.oc.p, 4 * mo, hipMemcpyDeviceToHost, st));
    log.mark("result");
    HIPCHECK(hipStreamSynchronize(st));
  }
  X.idle = true;
  log.print("sicp_merge: n_in=" + std::to_string(n_in) + " n_out=" + std::to_string(n_out));
  const uint32_t* o = h->mg_out.data();
  if (dst) {
    const StridedCloud in = {(const char*)o, (const char*)(o + mo), (const char*)(o + 2 * mo), has_label ? (const char*)(o + 3 * mo) : nullptr, 4, 4};
    const int rc = set_cloud_common(dst, dst_which, n_out, in);
    if (rc != SICP_OK) {
      if (dst != h) h->last_error = "sicp_merge_clouds: dst: " + dst->last_error;
      return rc;
    }
  }
  if (n_out > 0) {
    if (x) std::memcpy(x, o, 4 * mo);
    if (y) std::memcpy(y, o + mo, 4 * mo);
    if (z) std::memcpy(z, o + 2 * mo, 4 * mo);
    if (label && has_label) std::memcpy(label, o + 3 * mo, 4 * mo);
    if (count) std::memcpy(count, o + 4 * mo, 4 * mo);
  }
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
