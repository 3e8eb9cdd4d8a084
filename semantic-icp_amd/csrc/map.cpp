// map.cpp -- sicp_map_* (include/sicp.h): a voxel map that lives on the device between calls.  Its rows (kernels.h: MapRows)
// lie sorted by key in one of two sets of arena buffers.  A call that changes the map -- integrate, prune -- computes into the
// spare set and swaps only once the counts and flags have been read back clean, so a refused call leaves the map as it was by
// construction.  The kernels: map_kernels.hip, map_merge_kernels.hip, merge's heads and gather launches, the rocPRIM wrappers.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

#define MAPCHECK(expr)                                                                         \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      m->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
      return _e == hipErrorOutOfMemory ? SICP_ERR_OUT_OF_MEMORY : SICP_ERR_HIP;                \
    }                                                                                          \
  } while (0)

// A call's device scratch: taken from the arena, given back at the end (`idle`: the stream has been synchronised behind the
// call's launches).
struct MapScratch {
  DevBuf<unsigned char> temp;
  DevBuf<float> tx, ty, tz, gx, gy, gz, ox, oy, oz;
  DevBuf<uint32_t> ol, oc, ohist;
  DevBuf<double> oconf, mx, my, mz;
  DevBuf<unsigned long long> key, key2, miss_key, total, stat;
  DevBuf<int> val, val2, flag, pos, heads, rank, miss, mpos, miss_rank, src_of, res, ray_hit;
  DevBuf<uint32_t> ray_miss;
  int device = -1;
  bool idle = true;
  ~MapScratch() {
    DevArena::release_scratch(device, idle, temp, tx, ty, tz, gx, gy, gz, ox, oy, oz, ol, oc, ohist, oconf, key, key2, miss_key, total, stat,
                              val, val2, flag, pos, heads, rank, miss, mpos, miss_rank, src_of, res, ray_hit, ray_miss, mx, my, mz);
  }
};

bool slot_ok(int which) { return which == SICP_SOURCE || which == SICP_TARGET; }

bool log_enabled() {
  static const bool on = debug_enabled() && std::getenv("SICP_MAP_LOG") != nullptr;
  return on;
}

int stride_of(const sicp_map_ctx* m) { return m->params.num_classes > 0 ? m->params.num_classes + 1 : 0; }

sicp::MapRows rows_of(sicp_map_ctx::Rows& r, bool hist) {
  sicp::MapRows R;
  R.key = r.key.p; R.sx = r.sx.p; R.sy = r.sy.p; R.sz = r.sz.p; R.cnt = r.cnt.p;
  R.hist = hist ? r.hist.p : nullptr;
  return R;
}

// room for `n` rows in a set (its contents are lost when it grows: only ever the spare set)
hipError_t reserve_rows(sicp_map_ctx::Rows& r, size_t n, int stride) {
  hipError_t e = r.key.reserve(n);
  if (e == hipSuccess) e = r.sx.reserve(n);
  if (e == hipSuccess) e = r.sy.reserve(n);
  if (e == hipSuccess) e = r.sz.reserve(n);
  if (e == hipSuccess) e = r.cnt.reserve(n);
  if (e == hipSuccess && stride > 0) e = r.hist.reserve(n * (size_t)stride);
  return e;
}

// crop arguments shared by the three calls: c = (float)centre, range^2 in double
struct Crop {
  int on;
  float c[3];
  double range_sq;
};
Crop make_crop(const double* center, double range) {
  Crop k;
  k.on = range > 0.0 ? 1 : 0;
  for (int d = 0; d < 3; ++d) k.c[d] = center ? (float)center[d] : 0.f;
  k.range_sq = range * range;
  return k;
}

// The rows whose S.flag is 1 become the map (prune and carve): the flags' scan, the survivors bit for bit into the spare set
// (S.to, reserved by the caller for n_map rows, as are X.pos, X.src_of, X.res -- zeroed --, X.total and X.temp for the scan),
// their histograms behind them, and the swap.  Takes the stream as it is, leaves it idle.
int keep_flagged_rows(sicp_map_ctx* m, MapScratch& X, const sicp::MapSelectArgs& S, size_t scan_bytes) {
  hipStream_t st = m->stream;
  X.idle = false;
  MAPCHECK(m->stage.resize(sizeof(int) * sicp::kMapRes + sizeof(unsigned long long)));
  MAPCHECK(hipMemsetAsync(X.total.p, 0, sizeof(unsigned long long), st));
  MAPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, S.flag, S.pos, S.n_map, st));
  MAPCHECK(sicp::launch_map_prune(S, st));
  int res[sicp::kMapRes];
  unsigned long long kept_points = 0;
  MAPCHECK(hipMemcpyAsync(m->stage.data(), X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
  MAPCHECK(hipMemcpyAsync(m->stage.data() + sizeof res, X.total.p, sizeof kept_points, hipMemcpyDeviceToHost, st));
  MAPCHECK(hipStreamSynchronize(st));
  std::memcpy(res, m->stage.data(), sizeof res);
  std::memcpy(&kept_points, m->stage.data() + sizeof res, sizeof kept_points);
  const int n_keep = res[sicp::kMapOut];
  if (S.stride > 0 && n_keep > 0) {  // (the rows' places are known: their histograms follow)
    MAPCHECK(sicp::launch_map_move_hist(S.rows.hist, S.to.hist, S.src_of, n_keep, S.stride, st));
    MAPCHECK(hipStreamSynchronize(st));
  }
  X.idle = true;
  m->cur ^= 1;
  m->n_voxels = n_keep;
  m->n_points = kept_points;
  return SICP_OK;
}

}  // namespace

void map_default_params(sicp_map_params* p) {
  std::memset(p, 0, sizeof *p);
  p->leaf_size = 0.2;
}

void map_default_extract_params(sicp_map_extract_params* p) {
  std::memset(p, 0, sizeof *p);
  p->min_count = 1;
}

void map_default_carve_params(sicp_map_carve_params* p) {
  std::memset(p, 0, sizeof *p);
  p->min_rays = 3;
  p->end_margin = 1;
}

int map_create(int device_id, const sicp_map_params* p, sicp_map_ctx** out) {
  if (!out) return SICP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!p || !(p->leaf_size > 0.0) || !std::isfinite(p->leaf_size) || p->num_classes < 0 || p->num_classes > 255) return SICP_ERR_INVALID_ARGUMENT;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SICP_ERR_NO_DEVICE;
  if (device_id < 0 || device_id >= n) return SICP_ERR_INVALID_ARGUMENT;
  sicp_map_ctx* m = new (std::nothrow) sicp_map_ctx();
  if (!m) return SICP_ERR_OUT_OF_MEMORY;
  m->device = device_id;
  m->params = *p;
  m->params.reserved_ = 0;
  if (hipSetDevice(device_id) != hipSuccess || m->stream.create() != hipSuccess) {
    delete m;
    return SICP_ERR_NO_DEVICE;
  }
  *out = m;
  return SICP_OK;
}

int map_destroy(sicp_map_ctx* m) {
  if (!m) return SICP_OK;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  {
    DevArena::FreeScope once(m->device);  // one wait for the device, not one per buffer
    delete m;
  }
  return SICP_OK;
}

int map_integrate(sicp_map_ctx* m, sicp_context* h, int which, const double* qt, const double* crop_center, double crop_range,
                  sicp_map_integrate_info* info) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_integrate: " + why + "; the map is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!h) return refuse("the handle is NULL");
  if (!slot_ok(which)) return refuse("`which` is neither SICP_SOURCE nor SICP_TARGET");
  if (h->device != m->device) return refuse("the handle is on device " + std::to_string(h->device) + ", the map on " + std::to_string(m->device));
  if (!(crop_range >= 0.0)) return refuse("crop_range must be >= 0 (+inf is allowed)");
  if (crop_center)
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(crop_center[d])) return refuse("crop_center must be finite");
  if (qt)
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(qt[k])) return refuse("the pose is not finite");
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    m->last_error = "sicp_map_integrate: the slot has no cloud";
    return SICP_ERR_NOT_READY;
  }
  const int C = m->params.num_classes, stride = stride_of(m);
  if (C > 0 && !c.has_label) return refuse("the cloud has no labels and the map keeps " + std::to_string(C) + " classes");
  const double t_begin = now_ms();
  MAPCHECK(hipSetDevice(m->device));
  // the scan's device copy: the finite points in caller order (Cloud::rx ..., valid in every layout), prepared as a merge part is
  if (c.layout < 0) {
    const int rc = prepare_cloud(h, c);
    if (rc != SICP_OK) {
      m->last_error = "sicp_map_integrate: the cloud: " + (h->last_error.empty() ? std::string("not ready") : h->last_error);
      return rc;
    }
  }
  if (c.pending && c.ready_ev) {  // (the upload runs on the handle's stream, the kernels below on the map's)
    MAPCHECK(hipEventSynchronize(c.ready_ev));
    c.pending = false;
  }
  const int n = c.n;
  const int n_map = (int)m->n_voxels;
  sicp_map_integrate_info I;
  std::memset(&I, 0, sizeof I);
  I.n_in = n;
  I.n_voxels = m->n_voxels;
  if (n == 0) {
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    return SICP_OK;
  }
  hipStream_t st = m->stream;
  StageLog log(log_enabled(), st);
  MapScratch X;
  X.device = m->device;
  X.idle = false;
  const size_t np = (size_t)n;
  MAPCHECK(m->stage.resize(sizeof(int) * sicp::kMapRes));
  MAPCHECK(X.tx.reserve(np)); MAPCHECK(X.ty.reserve(np)); MAPCHECK(X.tz.reserve(np));
  MAPCHECK(X.gx.reserve(np)); MAPCHECK(X.gy.reserve(np)); MAPCHECK(X.gz.reserve(np));
  MAPCHECK(X.key.reserve(np)); MAPCHECK(X.key2.reserve(np));
  MAPCHECK(X.val.reserve(np)); MAPCHECK(X.val2.reserve(np));
  MAPCHECK(X.flag.reserve(np)); MAPCHECK(X.pos.reserve(np)); MAPCHECK(X.heads.reserve(np));
  MAPCHECK(X.rank.reserve(np)); MAPCHECK(X.miss.reserve(np)); MAPCHECK(X.mpos.reserve(np));
  MAPCHECK(X.miss_key.reserve(np)); MAPCHECK(X.miss_rank.reserve(np));
  MAPCHECK(X.res.reserve(sicp::kMapRes));
  size_t pair_bytes = 0, scan_bytes = 0;
  MAPCHECK(sicp::prim_sort_pairs(nullptr, pair_bytes, X.key.p, X.key2.p, X.val.p, X.val2.p, n, 0, 64, st));
  MAPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, n, st));
  MAPCHECK(X.temp.reserve(std::max(pair_bytes, scan_bytes) + 256));

  const Crop crop = make_crop(crop_center, crop_range);
  const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
  sicp::MapKeyArgs K;
  std::memset(&K, 0, sizeof K);
  K.x = c.rx.p; K.y = c.ry.p; K.z = c.rz.p;
  K.label = C > 0 ? c.rl.p : nullptr;
  matrix34(qt ? qt : ident, K.M);
  K.n = n; K.crop = crop.on; K.num_classes = C;
  K.inv_leaf = 1.0f / (float)m->params.leaf_size;
  K.cx = crop.c[0]; K.cy = crop.c[1]; K.cz = crop.c[2];
  K.range_sq = crop.range_sq;
  K.tx = X.tx.p; K.ty = X.ty.p; K.tz = X.tz.p;
  K.key = X.key.p; K.val = X.val.p; K.res = X.res.p;
  // the scan's runs of equal keys: merge's heads and gather (the labels ride in the low word of its rank | label keys)
  sicp::MergeReduceArgs R;
  std::memset(&R, 0, sizeof R);
  R.n = n; R.voxel = 1; R.labels = C > 0 ? 1 : 0;
  R.skey = X.key2.p; R.sval = X.val2.p;
  R.flag = X.flag.p; R.pos = X.pos.p; R.heads = X.heads.p;
  R.tx = X.tx.p; R.ty = X.ty.p; R.tz = X.tz.p; R.tlabel = K.label;
  R.gx = X.gx.p; R.gy = X.gy.p; R.gz = X.gz.p;
  R.lkey = X.key.p;  // (the unsorted keys are dead once sorted)
  R.res = X.res.p;
  sicp_map_ctx::Rows& cur = m->rows[m->cur];
  sicp_map_ctx::Rows& spare = m->rows[m->cur ^ 1];
  sicp::MapFoldArgs F;
  std::memset(&F, 0, sizeof F);
  F.n = n; F.n_map = n_map; F.n_new = 0; F.stride = stride;
  F.skey = X.key2.p; F.heads = X.heads.p;
  F.gx = X.gx.p; F.gy = X.gy.p; F.gz = X.gz.p; F.lkey = X.key.p;
  F.rank = X.rank.p; F.miss = X.miss.p; F.mpos = X.mpos.p;
  F.miss_key = X.miss_key.p; F.miss_rank = X.miss_rank.p;
  F.res = X.res.p;
  F.from = rows_of(cur, stride > 0);

  log.mark("begin");
  MAPCHECK(hipMemsetAsync(X.res.p, 0, sizeof(int) * sicp::kMapRes, st));
  MAPCHECK(sicp::launch_map_keys(K, st));
  log.mark("key");
  MAPCHECK(sicp::prim_sort_pairs(X.temp.p, pair_bytes, X.key.p, X.key2.p, X.val.p, X.val2.p, n, 0, 64, st));
  log.mark("sort");
  MAPCHECK(sicp::launch_merge_heads(R, st));
  MAPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, n, st));
  MAPCHECK(sicp::launch_merge_gather(R, st));
  log.mark("runs");
  MAPCHECK(sicp::launch_map_lookup(F, st));
  MAPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.miss.p, X.mpos.p, n, st));
  MAPCHECK(sicp::launch_map_misses(F, st));
  log.mark("lookup");
  int res[sicp::kMapRes];
  MAPCHECK(hipMemcpyAsync(m->stage.data(), X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
  MAPCHECK(hipStreamSynchronize(st));
  std::memcpy(res, m->stage.data(), sizeof res);
  X.idle = true;
  // every refusal lies before the first write to a row
  if (res[sicp::kMapRange])
    return refuse("leaf size " + std::to_string(m->params.leaf_size) + " is too small for the points: a voxel coordinate reaches 2^20");
  if (res[sicp::kMapBadLabel]) {
    m->last_error = "sicp_map_integrate: a label above num_classes = " + std::to_string(C) + "; the map is unchanged";
    return SICP_ERR_BAD_LABEL;
  }
  const int n_kept = res[sicp::kMapKept], n_scan_vox = res[sicp::kMapScanVoxels], n_new = res[sicp::kMapNew];
  I.n_kept = n_kept;
  I.n_scan_voxels = n_scan_vox;
  I.n_new_voxels = n_new;
  if (n_kept == 0) {
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    return SICP_OK;
  }
  if (m->n_voxels + (long long)n_new > 0x7fffffffll) return refuse("the map would hold more than 2^31 - 1 voxels");
  if (m->n_points + (unsigned long long)n_kept > 0xffffffffull) return refuse("the map would hold more than 2^32 - 1 points");
  const size_t rows = (size_t)n_map + (size_t)n_new;
  X.idle = false;
  MAPCHECK(reserve_rows(spare, rows, stride));
  MAPCHECK(X.src_of.reserve(rows));
  F.n_new = n_new;
  F.src_of = X.src_of.p;
  F.to = rows_of(spare, stride > 0);
  MAPCHECK(sicp::launch_map_scatter(F, st));
  if (stride > 0) MAPCHECK(sicp::launch_map_move_hist(F.from.hist, F.to.hist, F.src_of, (long long)rows, stride, st));
  log.mark("scatter");
  MAPCHECK(sicp::launch_map_fold(F, st));
  log.mark("fold");
  MAPCHECK(hipStreamSynchronize(st));
  X.idle = true;
  m->cur ^= 1;
  m->n_voxels = (long long)rows;
  m->n_points += (unsigned long long)n_kept;
  I.n_voxels = m->n_voxels;
  log.print("sicp_map_integrate: n_in=" + std::to_string(n) + " n_map=" + std::to_string(n_map) + " n_new=" + std::to_string(n_new));
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

int map_prune(sicp_map_ctx* m, const double* center, double range, int64_t* n_removed) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_prune: " + why + "; the map is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!center) return refuse("the centre is NULL");
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(center[d])) return refuse("the centre must be finite");
  if (!(range > 0.0)) return refuse("the range must be > 0 (+inf keeps everything)");
  if (n_removed) *n_removed = 0;
  const int n_map = (int)m->n_voxels, stride = stride_of(m);
  if (n_map == 0) return SICP_OK;
  MAPCHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  MapScratch X;
  X.device = m->device;
  X.idle = false;
  const size_t nr = (size_t)n_map;
  sicp_map_ctx::Rows& cur = m->rows[m->cur];
  sicp_map_ctx::Rows& spare = m->rows[m->cur ^ 1];
  MAPCHECK(m->stage.resize(sizeof(int) * sicp::kMapRes + sizeof(unsigned long long)));
  MAPCHECK(reserve_rows(spare, nr, stride));
  MAPCHECK(X.flag.reserve(nr)); MAPCHECK(X.pos.reserve(nr)); MAPCHECK(X.src_of.reserve(nr));
  MAPCHECK(X.res.reserve(sicp::kMapRes)); MAPCHECK(X.total.reserve(1));
  size_t scan_bytes = 0;
  MAPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, n_map, st));
  MAPCHECK(X.temp.reserve(scan_bytes + 256));
  const Crop crop = make_crop(center, range);
  sicp::MapSelectArgs S;
  std::memset(&S, 0, sizeof S);
  S.n_map = n_map; S.stride = stride; S.min_count = 0; S.crop = 1;
  S.cx = crop.c[0]; S.cy = crop.c[1]; S.cz = crop.c[2]; S.range_sq = crop.range_sq;
  S.rows = rows_of(cur, stride > 0);
  S.to = rows_of(spare, stride > 0);
  S.flag = X.flag.p; S.pos = X.pos.p; S.src_of = X.src_of.p;
  S.kept_points = X.total.p; S.res = X.res.p;
  MAPCHECK(hipMemsetAsync(X.res.p, 0, sizeof(int) * sicp::kMapRes, st));
  MAPCHECK(sicp::launch_map_select(S, st));
  const int rc = keep_flagged_rows(m, X, S, scan_bytes);
  if (rc == SICP_OK && n_removed) *n_removed = (int64_t)n_map - m->n_voxels;
  return rc;
}

int map_carve(sicp_map_ctx* m, sicp_context* h, int which, const double* qt, const double* sensor_origin, const sicp_map_carve_params* p,
              int32_t capacity, uint32_t* miss, sicp_map_carve_info* info) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_carve: " + why + "; the map is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!h) return refuse("the handle is NULL");
  if (!p) return refuse("the params are NULL");
  if (!slot_ok(which)) return refuse("`which` is neither SICP_SOURCE nor SICP_TARGET");
  if (h->device != m->device) return refuse("the handle is on device " + std::to_string(h->device) + ", the map on " + std::to_string(m->device));
  if (!(p->max_range >= 0.0)) return refuse("max_range must be >= 0 (+inf is allowed)");
  if (p->min_rays < 1) return refuse("min_rays must be >= 1");
  if (p->end_margin < 0) return refuse("end_margin must be >= 0");
  if (p->dry_run != 0 && p->dry_run != 1) return refuse("dry_run is neither 0 nor 1");
  const int C = m->params.num_classes, stride = stride_of(m);
  if (p->n_protect < 0 || p->n_protect > SICP_MAP_MAX_PROTECT) return refuse("n_protect must be 0.." + std::to_string(SICP_MAP_MAX_PROTECT));
  if (p->n_protect > 0 && C == 0) return refuse("the map keeps no labels: there is nothing to protect");
  for (int j = 0; j < p->n_protect; ++j)
    if (p->protect[j] > (uint32_t)C) return refuse("protect[" + std::to_string(j) + "] = " + std::to_string(p->protect[j]) + " is above num_classes = " + std::to_string(C));
  if (sensor_origin)
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(sensor_origin[d])) return refuse("sensor_origin must be finite");
  if (qt)
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(qt[k])) return refuse("the pose is not finite");
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    m->last_error = "sicp_map_carve: the slot has no cloud";
    return SICP_ERR_NOT_READY;
  }
  const double t_begin = now_ms();
  MAPCHECK(hipSetDevice(m->device));
  if (c.layout < 0) {  // (prepared as a merge part is: sicp_map_integrate's rule)
    const int rc = prepare_cloud(h, c);
    if (rc != SICP_OK) {
      m->last_error = "sicp_map_carve: the cloud: " + (h->last_error.empty() ? std::string("not ready") : h->last_error);
      return rc;
    }
  }
  if (c.pending && c.ready_ev) {
    MAPCHECK(hipEventSynchronize(c.ready_ev));
    c.pending = false;
  }
  const int n = c.n;
  const int n_map = (int)m->n_voxels;
  const size_t nr = (size_t)n_map;
  sicp_map_carve_info I;
  std::memset(&I, 0, sizeof I);
  I.n_in = n;
  I.n_voxels = m->n_voxels;
  const bool short_miss = miss && capacity < n_map;
  auto capacity_refusal = [&]() {
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    m->last_error = "sicp_map_carve: the map has " + std::to_string(n_map) + " rows, miss holds " + std::to_string(capacity) + "; the map is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  hipStream_t st = m->stream;
  StageLog log(log_enabled(), st);
  MapScratch X;
  unsigned long long stat[sicp::kCarveStats] = {};
  size_t scan_bytes = 0;
  sicp::MapSelectArgs S;
  std::memset(&S, 0, sizeof S);
  {  // (a slot without a finite point goes the same way: its origin is checked, its counts are zero)
    X.device = m->device;
    X.idle = false;
    const size_t head = sizeof(int) * sicp::kMapRes + sizeof stat;
    MAPCHECK(m->stage.resize(head));
    MAPCHECK(X.res.reserve(sicp::kMapRes)); MAPCHECK(X.stat.reserve(sicp::kCarveStats));
    if (n_map > 0) {
      MAPCHECK(X.ray_hit.reserve(nr)); MAPCHECK(X.ray_miss.reserve(nr)); MAPCHECK(X.flag.reserve(nr));
      MAPCHECK(hipMemsetAsync(X.ray_hit.p, 0, sizeof(int) * nr, st));
      MAPCHECK(hipMemsetAsync(X.ray_miss.p, 0, sizeof(uint32_t) * nr, st));
    }
    const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
    sicp::MapCarveArgs A;
    std::memset(&A, 0, sizeof A);
    A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
    matrix34(qt ? qt : ident, A.M);
    A.n = n;
    A.inv_leaf = 1.0f / (float)m->params.leaf_size;
    A.sx = sensor_origin ? (float)sensor_origin[0] : 0.f;
    A.sy = sensor_origin ? (float)sensor_origin[1] : 0.f;
    A.sz = sensor_origin ? (float)sensor_origin[2] : 0.f;
    A.ranged = p->max_range > 0.0 ? 1 : 0;
    A.range_sq = p->max_range * p->max_range;
    A.end_margin = p->end_margin;
    A.key = m->rows[m->cur].key.p; A.n_map = n_map;
    A.hit = X.ray_hit.p; A.miss = X.ray_miss.p; A.stat = X.stat.p; A.res = X.res.p;
    sicp::MapCarveSelectArgs Q;
    std::memset(&Q, 0, sizeof Q);
    Q.n_map = n_map; Q.stride = stride; Q.min_rays = p->min_rays; Q.n_protect = p->n_protect;
    for (int j = 0; j < p->n_protect; ++j) Q.protect[j] = p->protect[j];
    Q.hist = stride > 0 ? m->rows[m->cur].hist.p : nullptr;
    Q.hit = X.ray_hit.p; Q.miss = X.ray_miss.p; Q.flag = X.flag.p; Q.stat = X.stat.p;
    log.mark("begin");
    MAPCHECK(hipMemsetAsync(X.res.p, 0, sizeof(int) * sicp::kMapRes, st));
    MAPCHECK(hipMemsetAsync(X.stat.p, 0, sizeof stat, st));
    MAPCHECK(sicp::launch_map_carve_hits(A, st));
    log.mark("hits");
    MAPCHECK(sicp::launch_map_carve_walk(A, st));
    log.mark("walk");
    MAPCHECK(sicp::launch_map_carve_select(Q, st));
    log.mark("select");
    int res[sicp::kMapRes];
    MAPCHECK(hipMemcpyAsync(m->stage.data(), X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipMemcpyAsync(m->stage.data() + sizeof res, X.stat.p, sizeof stat, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipStreamSynchronize(st));
    std::memcpy(res, m->stage.data(), sizeof res);
    std::memcpy(stat, m->stage.data() + sizeof res, sizeof stat);
    X.idle = true;
    if (res[sicp::kMapRange])
      return refuse("leaf size " + std::to_string(m->params.leaf_size) + " is too small for the sensor origin: a voxel coordinate reaches 2^20");
  }
  I.n_rays = (int64_t)stat[sicp::kCarveRays];
  I.n_steps = (int64_t)stat[sicp::kCarveSteps];
  I.n_touched = (int32_t)stat[sicp::kCarveTouched];
  I.n_hit = (int32_t)stat[sicp::kCarveHit];
  I.n_removed = (int32_t)stat[sicp::kCarveRemoved];
  I.n_spared_hit = (int32_t)stat[sicp::kCarveSparedHit];
  I.n_spared_label = (int32_t)stat[sicp::kCarveSparedLabel];
  if (short_miss) return capacity_refusal();  // (every refusal lies before the first write to a row)
  const bool carve = !p->dry_run && I.n_removed > 0;
  if (carve) {  // prune's compaction of the rows the select kernel flagged
    sicp_map_ctx::Rows& cur = m->rows[m->cur];
    sicp_map_ctx::Rows& spare = m->rows[m->cur ^ 1];
    X.idle = false;
    MAPCHECK(reserve_rows(spare, nr, stride));
    MAPCHECK(X.pos.reserve(nr)); MAPCHECK(X.src_of.reserve(nr)); MAPCHECK(X.total.reserve(1));
    MAPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, n_map, st));
    MAPCHECK(X.temp.reserve(scan_bytes + 256));
    if (miss) MAPCHECK(m->out.resize(nr));
    S.n_map = n_map; S.stride = stride;
    S.rows = rows_of(cur, stride > 0);
    S.to = rows_of(spare, stride > 0);
    S.flag = X.flag.p; S.pos = X.pos.p; S.src_of = X.src_of.p;
    S.kept_points = X.total.p; S.res = X.res.p;
  } else if (miss && n_map > 0) {
    MAPCHECK(m->out.resize(nr));
  }
  if (miss && n_map > 0) {  // (on the host before the map changes: a failed copy leaves the map as it was)
    X.idle = false;
    MAPCHECK(hipMemcpyAsync(m->out.data(), X.ray_miss.p, sizeof(uint32_t) * nr, hipMemcpyDeviceToHost, st));
    log.mark("result");
    MAPCHECK(hipStreamSynchronize(st));
    X.idle = true;
  }
  if (carve) {
    const int rc = keep_flagged_rows(m, X, S, scan_bytes);
    if (rc != SICP_OK) return rc;
    log.mark("compact");
    if (log.on) MAPCHECK(hipStreamSynchronize(st));  // (the log reads the mark's event)
  }
  if (miss && n_map > 0) std::memcpy(miss, m->out.data(), sizeof(uint32_t) * nr);
  I.n_voxels = m->n_voxels;
  log.print("sicp_map_carve: n_in=" + std::to_string(n) + " n_map=" + std::to_string(n_map) + " n_removed=" + std::to_string(I.n_removed));
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

// sicp_map_extract and sicp_map_extract_fused (`confidence_wanted`): the selection, the order, the centroids and counts, the
// capacity rule, dst and info are one code; the fused call replaces the arg-max label by the posterior's and adds its probability
// `given_flag` (sicp_map_raycast: the rows its rays hit; [n_map] on the device, written on the map's stream) takes the place of
// the selection by min_count and crop
static int extract_rows(sicp_map_ctx* m, const char* call, bool fused, const sicp_map_extract_params* p, sicp_context* dst, int dst_which,
                        int32_t capacity, float* x, float* y, float* z, uint32_t* label, uint32_t* count, uint32_t* hist,
                        double* confidence, sicp_map_extract_info* info, int* given_flag = nullptr) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  const std::string name = call;
  auto refuse = [&](const std::string& why) {
    m->last_error = name + ": " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!p) return refuse("the params are NULL");
  if (dst && !slot_ok(dst_which)) return refuse("dst_which is neither SICP_SOURCE nor SICP_TARGET");
  if (dst && dst->device != m->device) return refuse("dst is on device " + std::to_string(dst->device) + ", the map on " + std::to_string(m->device));
  if (!(p->crop_range >= 0.0)) return refuse("crop_range must be >= 0 (+inf is allowed)");
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(p->crop_center[d])) return refuse("crop_center must be finite");
  const int C = m->params.num_classes, stride = stride_of(m);
  if (hist && C == 0) return refuse("the map keeps no labels: there are no histograms");
  if (fused && C == 0) return refuse("the map keeps no labels: there is nothing to fuse");
  if (fused && !m->has_cm) {
    m->last_error = name + ": no confusion matrix has been set (sicp_map_set_confusion)";
    return SICP_ERR_NOT_READY;
  }
  const double t_begin = now_ms();
  MAPCHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  StageLog log(log_enabled(), st);
  const int n_map = (int)m->n_voxels;
  const size_t nr = (size_t)n_map;
  int res[sicp::kMapRes] = {};
  MapScratch X;
  sicp::MapSelectArgs S;
  std::memset(&S, 0, sizeof S);
  if (n_map > 0) {
    X.device = m->device;
    X.idle = false;
    MAPCHECK(m->stage.resize(sizeof res));
    if (!given_flag) MAPCHECK(X.flag.reserve(nr));
    MAPCHECK(X.pos.reserve(nr)); MAPCHECK(X.src_of.reserve(nr));
    MAPCHECK(X.ox.reserve(nr)); MAPCHECK(X.oy.reserve(nr)); MAPCHECK(X.oz.reserve(nr)); MAPCHECK(X.oc.reserve(nr));
    if (C > 0) MAPCHECK(X.ol.reserve(nr));
    if (fused) MAPCHECK(X.oconf.reserve(nr));
    MAPCHECK(X.res.reserve(sicp::kMapRes));
    size_t scan_bytes = 0;
    int* const flag = given_flag ? given_flag : X.flag.p;
    MAPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, flag, X.pos.p, n_map, st));
    MAPCHECK(X.temp.reserve(scan_bytes + 256));
    const Crop crop = make_crop(p->crop_center, p->crop_range);
    S.n_map = n_map; S.stride = stride; S.min_count = p->min_count; S.crop = crop.on;
    S.cx = crop.c[0]; S.cy = crop.c[1]; S.cz = crop.c[2]; S.range_sq = crop.range_sq;
    S.rows = rows_of(m->rows[m->cur], stride > 0);
    S.flag = flag; S.pos = X.pos.p; S.src_of = X.src_of.p;
    S.ox = X.ox.p; S.oy = X.oy.p; S.oz = X.oz.p; S.ocount = X.oc.p;
    S.olabel = C > 0 ? X.ol.p : nullptr;
    S.res = X.res.p;
    log.mark("begin");
    MAPCHECK(hipMemsetAsync(X.res.p, 0, sizeof res, st));
    if (!given_flag) MAPCHECK(sicp::launch_map_select(S, st));
    MAPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, flag, X.pos.p, n_map, st));
    MAPCHECK(sicp::launch_map_extract(S, st));
    log.mark("select_gather");
    if (fused) {  // (the rows' number is on the device: the kernel reads it there)
      sicp::MapFuseArgs A;
      std::memset(&A, 0, sizeof A);
      A.logcm = m->logcm.p; A.C = C; A.stride = stride;
      A.rows = S.rows; A.n_map = n_map;
      A.src_of = X.src_of.p; A.res_in = X.res.p;
      A.olabel = X.ol.p; A.oconf = X.oconf.p;
      MAPCHECK(sicp::launch_map_posterior(A, st));
      log.mark("posterior");
    }
    MAPCHECK(hipMemcpyAsync(m->stage.data(), X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipStreamSynchronize(st));
    std::memcpy(res, m->stage.data(), sizeof res);
    X.idle = true;
  }
  const int n_out = res[sicp::kMapOut];
  sicp_map_extract_info I;
  std::memset(&I, 0, sizeof I);
  I.n_voxels = m->n_voxels;
  I.n_out = n_out;
  I.max_voxel_points = res[sicp::kMapMaxCount];
  I.has_label = C > 0 ? 1 : 0;
  const bool want_arrays = x || y || z || label || count || hist || confidence;
  if (want_arrays && capacity < n_out) {
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    m->last_error = name + ": the result has " + std::to_string(n_out) + " points, the output arrays hold " + std::to_string(capacity);
    return SICP_ERR_INVALID_ARGUMENT;
  }
  if (dst && n_out == 0) {
    m->last_error = name + ": the result is empty; dst keeps its cloud";
    return SICP_ERR_TOO_FEW_POINTS;
  }
  // the result -> pinned memory: the whole of it is on the host before dst's slot lets go of its old cloud
  const size_t mo = (size_t)n_out;
  const size_t hist_words = hist ? mo * (size_t)stride : 0;
  const size_t conf_at = (mo * 5 + hist_words + 1) & ~(size_t)1;  // (doubles: an even word)
  if (n_out > 0 && (want_arrays || dst)) {
    X.idle = false;
    MAPCHECK(m->out.resize(conf_at + (fused ? 2 * mo : 0)));
    uint32_t* o = m->out.data();
    if (fused) MAPCHECK(hipMemcpyAsync(o + conf_at, X.oconf.p, 8 * mo, hipMemcpyDeviceToHost, st));
    if (hist) {
      MAPCHECK(X.ohist.reserve(hist_words));
      MAPCHECK(sicp::launch_map_move_hist(S.rows.hist, X.ohist.p, S.src_of, n_out, stride, st));
      MAPCHECK(hipMemcpyAsync(o + 5 * mo, X.ohist.p, 4 * hist_words, hipMemcpyDeviceToHost, st));
    }
    MAPCHECK(hipMemcpyAsync(o, X.ox.p, 4 * mo, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipMemcpyAsync(o + mo, X.oy.p, 4 * mo, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipMemcpyAsync(o + 2 * mo, X.oz.p, 4 * mo, hipMemcpyDeviceToHost, st));
    if (C > 0) MAPCHECK(hipMemcpyAsync(o + 3 * mo, X.ol.p, 4 * mo, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipMemcpyAsync(o + 4 * mo, X.oc.p, 4 * mo, hipMemcpyDeviceToHost, st));
    log.mark("result");
    MAPCHECK(hipStreamSynchronize(st));
    X.idle = true;
  }
  log.print(name + ": n_map=" + std::to_string(n_map) + " n_out=" + std::to_string(n_out));
  const uint32_t* o = m->out.data();
  if (dst) {
    const StridedCloud in = {(const char*)o, (const char*)(o + mo), (const char*)(o + 2 * mo), C > 0 ? (const char*)(o + 3 * mo) : nullptr, 4, 4};
    const int rc = set_cloud_common(dst, dst_which, n_out, in);
    if (rc != SICP_OK) {
      m->last_error = name + ": dst: " + dst->last_error;
      return rc;
    }
  }
  if (n_out > 0) {
    if (x) std::memcpy(x, o, 4 * mo);
    if (y) std::memcpy(y, o + mo, 4 * mo);
    if (z) std::memcpy(z, o + 2 * mo, 4 * mo);
    if (label && C > 0) std::memcpy(label, o + 3 * mo, 4 * mo);
    if (count) std::memcpy(count, o + 4 * mo, 4 * mo);
    if (hist) std::memcpy(hist, o + 5 * mo, 4 * mo * (size_t)stride);
    if (confidence) std::memcpy(confidence, o + conf_at, 8 * mo);
  }
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

int map_extract(sicp_map_ctx* m, const sicp_map_extract_params* p, sicp_context* dst, int dst_which, int32_t capacity, float* x,
                float* y, float* z, uint32_t* label, uint32_t* count, uint32_t* hist, sicp_map_extract_info* info) {
  return extract_rows(m, "sicp_map_extract", false, p, dst, dst_which, capacity, x, y, z, label, count, hist, nullptr, info);
}

int map_extract_fused(sicp_map_ctx* m, const sicp_map_extract_params* p, sicp_context* dst, int dst_which, int32_t capacity, float* x,
                      float* y, float* z, uint32_t* label, uint32_t* count, double* confidence, sicp_map_extract_info* info) {
  return extract_rows(m, "sicp_map_extract_fused", true, p, dst, dst_which, capacity, x, y, z, label, count, nullptr, confidence, info);
}

void map_default_raycast_params(sicp_map_raycast_params* p) {
  std::memset(p, 0, sizeof *p);
  p->min_count = 1;
  p->start_margin = 1;
}

// sicp_map_raycast (include/sicp.h, "ray casting"): the ends go up through pinned staging, one lane per row writes its opaque
// byte, the walk answers every ray and marks the rows hit, and the per-ray results are on the host before dst -- through
// extract_rows, with the marks as the selection -- or a caller's array is touched.
int map_raycast(sicp_map_ctx* m, const double* qt, const double* sensor_origin, int32_t n, const float* ex, const float* ey,
                const float* ez, const sicp_map_raycast_params* p, sicp_context* dst, int dst_which, int32_t* row, int32_t* step,
                int32_t* length, float* x, float* y, float* z, uint32_t* label, uint32_t* count, double* range_sq,
                sicp_map_raycast_info* info) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_raycast: " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!p) return refuse("the params are NULL");
  if (!ex || !ey || !ez) return refuse("an end array is NULL");
  if (n < 0) return refuse("n is negative");
  if (dst && !slot_ok(dst_which)) return refuse("dst_which is neither SICP_SOURCE nor SICP_TARGET");
  if (dst && dst->device != m->device) return refuse("dst is on device " + std::to_string(dst->device) + ", the map on " + std::to_string(m->device));
  if (!(p->max_range >= 0.0)) return refuse("max_range must be >= 0 (+inf is allowed)");
  if (p->min_count < 1) return refuse("min_count must be >= 1");
  if (p->start_margin < 0) return refuse("start_margin must be >= 0");
  const int C = m->params.num_classes, stride = stride_of(m);
  if (p->n_ignore < 0 || p->n_ignore > SICP_MAP_RAYCAST_MAX_IGNORE) return refuse("n_ignore must be 0.." + std::to_string(SICP_MAP_RAYCAST_MAX_IGNORE));
  if (p->n_ignore > 0 && C == 0) return refuse("the map keeps no labels: there is nothing to ignore");
  for (int j = 0; j < p->n_ignore; ++j)
    if (p->ignore[j] > (uint32_t)C) return refuse("ignore[" + std::to_string(j) + "] = " + std::to_string(p->ignore[j]) + " is above num_classes = " + std::to_string(C));
  if (sensor_origin)
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(sensor_origin[d])) return refuse("sensor_origin must be finite");
  if (qt)
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(qt[k])) return refuse("the pose is not finite");
  const double t_begin = now_ms();
  MAPCHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  StageLog log(log_enabled(), st);
  const int n_map = (int)m->n_voxels;
  const size_t nr = (size_t)n_map, np = (size_t)n;
  sicp_map_raycast_info I;
  std::memset(&I, 0, sizeof I);
  I.n_in = n;
  I.n_voxels = m->n_voxels;
  MapScratch X;
  X.device = m->device;
  X.idle = false;
  unsigned long long stat[sicp::kRaycastStats] = {};
  const size_t head = sizeof(int) * sicp::kMapRes + sizeof stat;
  MAPCHECK(m->stage.resize(head));
  MAPCHECK(m->rays.resize(10 * np));  // the ends on their way up, then: range_sq (doubles first) | row | step | length | x | y | z | label | count
  MAPCHECK(X.res.reserve(sicp::kMapRes)); MAPCHECK(X.stat.reserve(sicp::kRaycastStats));
  if (n_map > 0) { MAPCHECK(X.temp.reserve(nr)); MAPCHECK(X.flag.reserve(nr)); }
  if (n > 0) {
    MAPCHECK(X.tx.reserve(np)); MAPCHECK(X.ty.reserve(np)); MAPCHECK(X.tz.reserve(np));
    MAPCHECK(X.val.reserve(np)); MAPCHECK(X.val2.reserve(np)); MAPCHECK(X.rank.reserve(np));
    MAPCHECK(X.ox.reserve(np)); MAPCHECK(X.oy.reserve(np)); MAPCHECK(X.oz.reserve(np));
    MAPCHECK(X.ol.reserve(np)); MAPCHECK(X.oc.reserve(np)); MAPCHECK(X.oconf.reserve(np));
  }
  const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
  sicp::MapRaycastArgs A;
  std::memset(&A, 0, sizeof A);
  A.x = X.tx.p; A.y = X.ty.p; A.z = X.tz.p;
  matrix34(qt ? qt : ident, A.M);
  A.n = n;
  A.inv_leaf = 1.0f / (float)m->params.leaf_size;
  A.sx = sensor_origin ? (float)sensor_origin[0] : 0.f;
  A.sy = sensor_origin ? (float)sensor_origin[1] : 0.f;
  A.sz = sensor_origin ? (float)sensor_origin[2] : 0.f;
  A.ranged = p->max_range > 0.0 ? 1 : 0;
  A.range_sq = p->max_range * p->max_range;
  A.start_margin = p->start_margin;
  A.min_count = p->min_count;
  A.n_ignore = p->n_ignore;
  for (int j = 0; j < p->n_ignore; ++j) A.ignore[j] = p->ignore[j];
  A.rows = rows_of(m->rows[m->cur], stride > 0);
  A.n_map = n_map; A.stride = stride;
  A.opaque = X.temp.p; A.visible = X.flag.p;
  A.orow = X.val.p; A.ostep = X.val2.p; A.olength = X.rank.p;
  A.ox = X.ox.p; A.oy = X.oy.p; A.oz = X.oz.p;
  A.olabel = X.ol.p; A.ocount = X.oc.p; A.orange_sq = X.oconf.p;
  A.stat = X.stat.p; A.res = X.res.p;
  uint32_t* const o = m->rays.data();
  log.mark("begin");
  if (n > 0) {
    std::memcpy(o, ex, 4 * np); std::memcpy(o + np, ey, 4 * np); std::memcpy(o + 2 * np, ez, 4 * np);
    MAPCHECK(hipMemcpyAsync(X.tx.p, o, 4 * np, hipMemcpyHostToDevice, st));
    MAPCHECK(hipMemcpyAsync(X.ty.p, o + np, 4 * np, hipMemcpyHostToDevice, st));
    MAPCHECK(hipMemcpyAsync(X.tz.p, o + 2 * np, 4 * np, hipMemcpyHostToDevice, st));
  }
  MAPCHECK(hipMemsetAsync(X.res.p, 0, sizeof(int) * sicp::kMapRes, st));
  MAPCHECK(hipMemsetAsync(X.stat.p, 0, sizeof stat, st));
  if (n_map > 0) MAPCHECK(hipMemsetAsync(X.flag.p, 0, sizeof(int) * nr, st));
  log.mark("ends");
  MAPCHECK(sicp::launch_map_raycast_opaque(A, st));
  log.mark("opaque");
  MAPCHECK(sicp::launch_map_raycast_walk(A, st));
  log.mark("walk");
  MAPCHECK(sicp::launch_map_raycast_visible(A, st));
  int res[sicp::kMapRes];
  MAPCHECK(hipMemcpyAsync(m->stage.data(), X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
  MAPCHECK(hipMemcpyAsync(m->stage.data() + sizeof res, X.stat.p, sizeof stat, hipMemcpyDeviceToHost, st));
  if (n > 0) {  // (the ends have been read by then: the stream keeps the order)
    MAPCHECK(hipMemcpyAsync(o, X.oconf.p, 8 * np, hipMemcpyDeviceToHost, st));
    const void* from[8] = {X.val.p, X.val2.p, X.rank.p, X.ox.p, X.oy.p, X.oz.p, X.ol.p, X.oc.p};
    const void* wanted[8] = {row, step, length, x, y, z, label, count};
    for (int k = 0; k < 8; ++k)
      if (wanted[k]) MAPCHECK(hipMemcpyAsync(o + (2 + k) * np, from[k], 4 * np, hipMemcpyDeviceToHost, st));
  }
  log.mark("result");
  MAPCHECK(hipStreamSynchronize(st));
  std::memcpy(res, m->stage.data(), sizeof res);
  std::memcpy(stat, m->stage.data() + sizeof res, sizeof stat);
  X.idle = true;
  if (res[sicp::kMapRange])
    return refuse("leaf size " + std::to_string(m->params.leaf_size) + " is too small for the sensor origin: a voxel coordinate reaches 2^20");
  I.n_rays = (int64_t)stat[sicp::kRaycastRays];
  I.n_steps = (int64_t)stat[sicp::kRaycastSteps];
  I.n_hits = (int64_t)stat[sicp::kRaycastHits];
  I.n_visible = (int32_t)stat[sicp::kRaycastVisible];
  log.print("sicp_map_raycast: n_in=" + std::to_string(n) + " n_map=" + std::to_string(n_map) + " n_steps=" + std::to_string(I.n_steps) +
            " n_hits=" + std::to_string(I.n_hits));
  if (dst && I.n_visible == 0) {
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    m->last_error = "sicp_map_raycast: no ray hit the map; dst keeps its cloud";
    return SICP_ERR_TOO_FEW_POINTS;
  }
  if (dst) {  // the rows marked visible are the selection: extract's scan, gather and way into the slot
    sicp_map_extract_params E;
    map_default_extract_params(&E);
    const int rc = extract_rows(m, "sicp_map_raycast (visible rows)", false, &E, dst, dst_which, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, X.flag.p);
    if (rc != SICP_OK) return rc;
  }
  if (n > 0) {
    if (range_sq) std::memcpy(range_sq, o, 8 * np);
    void* to[8] = {row, step, length, x, y, z, label, count};
    for (int k = 0; k < 8; ++k)
      if (to[k]) std::memcpy(to[k], o + (2 + k) * np, 4 * np);
  }
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

int map_set_confusion(sicp_map_ctx* m, int32_t C, const double* cm) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_set_confusion: " + why + "; the map keeps the matrix it had";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!cm) return refuse("the matrix is NULL");
  const int classes = m->params.num_classes;
  if (classes == 0) return refuse("the map keeps no labels");
  if (C != classes) return refuse("the matrix has " + std::to_string(C) + " classes, the map " + std::to_string(classes));
  const size_t nn = (size_t)C * (size_t)C;
  for (size_t e = 0; e < nn; ++e)
    if (!std::isfinite(cm[e]) || cm[e] < 0.0)
      return refuse("entry [" + std::to_string(e / (size_t)C) + "][" + std::to_string(e % (size_t)C) + "] = " + std::to_string(cm[e]) +
                    " is negative or not finite");
  MAPCHECK(hipSetDevice(m->device));
  MAPCHECK(m->stage.resize(sizeof(double) * nn));
  MAPCHECK(m->logcm.reserve(nn));
  double* L = reinterpret_cast<double*>(m->stage.data());
  for (size_t e = 0; e < nn; ++e) L[e] = std::log(cm[e]);  // (log 0 = -inf: a class that never shows as that label)
  m->has_cm = false;  // (nothing can refuse any more; a failed copy leaves no matrix)
  MAPCHECK(hipMemcpyAsync(m->logcm.p, L, sizeof(double) * nn, hipMemcpyHostToDevice, m->stream));
  MAPCHECK(hipStreamSynchronize(m->stream));
  m->has_cm = true;
  return SICP_OK;
}

int map_fused_labels(sicp_map_ctx* m, sicp_context* h, int which, const double* qt, int32_t include_own_label, int32_t min_count,
                     uint32_t* out_labels, double* out_confidence) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_fused_labels: " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!h) return refuse("the handle is NULL");
  if (!out_labels) return refuse("out_labels is NULL");
  if (!slot_ok(which)) return refuse("`which` is neither SICP_SOURCE nor SICP_TARGET");
  if (include_own_label != 0 && include_own_label != 1) return refuse("include_own_label is neither 0 nor 1");
  if (min_count < 1) return refuse("min_count must be >= 1");
  if (qt)
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(qt[k])) return refuse("the pose is not finite");
  if (h->device != m->device) return refuse("the handle is on device " + std::to_string(h->device) + ", the map on " + std::to_string(m->device));
  const int C = m->params.num_classes, stride = stride_of(m);
  if (C == 0) return refuse("the map keeps no labels: there is nothing to fuse");
  if (!m->has_cm) {
    m->last_error = "sicp_map_fused_labels: no confusion matrix has been set (sicp_map_set_confusion)";
    return SICP_ERR_NOT_READY;
  }
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    m->last_error = "sicp_map_fused_labels: the slot has no cloud";
    return SICP_ERR_NOT_READY;
  }
  MAPCHECK(hipSetDevice(m->device));
  if (c.layout < 0) {  // (prepared as a merge part is: sicp_map_integrate's rule)
    const int rc = prepare_cloud(h, c);
    if (rc != SICP_OK) {
      m->last_error = "sicp_map_fused_labels: the cloud: " + (h->last_error.empty() ? std::string("not ready") : h->last_error);
      return rc;
    }
  }
  if (c.pending && c.ready_ev) {
    MAPCHECK(hipEventSynchronize(c.ready_ev));
    c.pending = false;
  }
  const int n = c.n;
  const size_t np = (size_t)n, n_caller = (size_t)c.n_caller;
  hipStream_t st = m->stream;
  StageLog log(log_enabled(), st);
  MapScratch X;
  if (n > 0) {
    X.device = m->device;
    X.idle = false;
    MAPCHECK(m->stage.resize(sizeof(int) * sicp::kMapRes));
    MAPCHECK(m->out.resize(3 * np));  // confidence (doubles first) | labels
    MAPCHECK(X.ol.reserve(np)); MAPCHECK(X.oconf.reserve(np)); MAPCHECK(X.res.reserve(sicp::kMapRes));
    const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
    sicp::MapFuseArgs A;
    std::memset(&A, 0, sizeof A);
    A.logcm = m->logcm.p; A.C = C; A.stride = stride;
    A.rows = rows_of(m->rows[m->cur], true); A.n_map = (int)m->n_voxels;
    A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
    A.label = c.has_label ? c.rl.p : nullptr;
    matrix34(qt ? qt : ident, A.M);
    A.n = n; A.include_own = include_own_label; A.min_count = min_count;
    A.inv_leaf = 1.0f / (float)m->params.leaf_size;
    A.res = X.res.p; A.olabel = X.ol.p; A.oconf = X.oconf.p;
    log.mark("begin");
    MAPCHECK(hipMemsetAsync(X.res.p, 0, sizeof(int) * sicp::kMapRes, st));
    MAPCHECK(sicp::launch_map_relabel(A, st));
    log.mark("relabel");
    uint32_t* o = m->out.data();
    MAPCHECK(hipMemcpyAsync(m->stage.data(), X.res.p, sizeof(int) * sicp::kMapRes, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipMemcpyAsync(o, X.oconf.p, 8 * np, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipMemcpyAsync(o + 2 * np, X.ol.p, 4 * np, hipMemcpyDeviceToHost, st));
    log.mark("result");
    MAPCHECK(hipStreamSynchronize(st));
    X.idle = true;
    log.print("sicp_map_fused_labels: n=" + std::to_string(n) + " n_map=" + std::to_string(m->n_voxels));
    int res[sicp::kMapRes];
    std::memcpy(res, m->stage.data(), sizeof res);
    if (res[sicp::kMapBadLabel]) {
      m->last_error = "sicp_map_fused_labels: a label above num_classes = " + std::to_string(C) + "; nothing was written";
      return SICP_ERR_BAD_LABEL;
    }
  }
  // caller order: a point that is not finite (it is not on the device) keeps label 0 and confidence 0
  const uint32_t* o = m->out.data();
  const double* conf = reinterpret_cast<const double*>(o);
  if (np == n_caller) {
    if (n > 0) {
      std::memcpy(out_labels, o + 2 * np, 4 * np);
      if (out_confidence) std::memcpy(out_confidence, conf, 8 * np);
    }
  } else {
    std::memset(out_labels, 0, 4 * n_caller);
    if (out_confidence) std::fill(out_confidence, out_confidence + n_caller, 0.0);
    for (size_t i = 0; i < np; ++i) {
      out_labels[c.keep[i]] = o[2 * np + i];
      if (out_confidence) out_confidence[c.keep[i]] = conf[i];
    }
  }
  return SICP_OK;
}

void map_default_merge_params(sicp_map_merge_params* p) {
  std::memset(p, 0, sizeof *p);
  p->min_count = 1;
}

// sicp_map_merge (include/sicp.h, "fusing maps"): src's rows are keyed on dst's grid and sorted, their runs go through
// integrate's rank merge into dst's spare set, and two fold launches add the runs' sums and histograms.  `m` is dst; src is
// only read (both maps are idle between calls, so dst's stream may read src's rows).
int map_merge(sicp_map_ctx* m, sicp_map_ctx* src, const double* qt, const sicp_map_merge_params* p, sicp_map_merge_info* info) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_merge: " + why + "; dst is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!src) return refuse("src is NULL");
  if (src == m) return refuse("src and dst are the same map");
  if (src->device != m->device) return refuse("src is on device " + std::to_string(src->device) + ", dst on " + std::to_string(m->device));
  sicp_map_merge_params P;
  if (p) P = *p; else map_default_merge_params(&P);
  if (P.min_count < 1) return refuse("min_count must be >= 1");
  if (!(P.crop_range >= 0.0)) return refuse("crop_range must be >= 0 (+inf is allowed)");
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(P.crop_center[d])) return refuse("crop_center must be finite");
  if (qt)
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(qt[k])) return refuse("the pose is not finite");
  const int C = m->params.num_classes, stride = stride_of(m);
  if (C > 0 && src->params.num_classes != C)
    return refuse("src keeps " + std::to_string(src->params.num_classes) + " classes, dst " + std::to_string(C));
  const double t_begin = now_ms();
  const int n = (int)src->n_voxels;
  const int n_map = (int)m->n_voxels;
  sicp_map_merge_info I;
  std::memset(&I, 0, sizeof I);
  I.n_src_rows = n;
  I.n_voxels = m->n_voxels;
  if (n == 0) {
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    return SICP_OK;
  }
  MAPCHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  StageLog log(log_enabled(), st);
  MapScratch X;
  X.device = m->device;
  X.idle = false;
  const size_t np = (size_t)n;
  MAPCHECK(m->stage.resize(sizeof(int) * sicp::kMapRes + sizeof(unsigned long long)));
  MAPCHECK(X.mx.reserve(np)); MAPCHECK(X.my.reserve(np)); MAPCHECK(X.mz.reserve(np));
  MAPCHECK(X.key.reserve(np)); MAPCHECK(X.key2.reserve(np));
  MAPCHECK(X.val.reserve(np)); MAPCHECK(X.val2.reserve(np));
  MAPCHECK(X.flag.reserve(np)); MAPCHECK(X.pos.reserve(np)); MAPCHECK(X.heads.reserve(np));
  MAPCHECK(X.rank.reserve(np)); MAPCHECK(X.miss.reserve(np)); MAPCHECK(X.mpos.reserve(np));
  MAPCHECK(X.miss_key.reserve(np)); MAPCHECK(X.miss_rank.reserve(np));
  MAPCHECK(X.res.reserve(sicp::kMapRes)); MAPCHECK(X.total.reserve(1));
  size_t pair_bytes = 0, scan_bytes = 0;
  MAPCHECK(sicp::prim_sort_pairs(nullptr, pair_bytes, X.key.p, X.key2.p, X.val.p, X.val2.p, n, 0, 64, st));
  MAPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, n, st));
  MAPCHECK(X.temp.reserve(std::max(pair_bytes, scan_bytes) + 256));

  const Crop crop = make_crop(P.crop_center, P.crop_range);
  const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
  sicp_map_ctx::Rows& cur = m->rows[m->cur];
  sicp_map_ctx::Rows& spare = m->rows[m->cur ^ 1];
  sicp::MapMergeArgs A;
  std::memset(&A, 0, sizeof A);
  A.n = n; A.n_map = n_map; A.stride = stride;
  A.crop = crop.on; A.min_count = P.min_count;
  matrix34(qt ? qt : ident, A.M);
  A.inv_leaf = 1.0f / (float)m->params.leaf_size;
  A.cx = crop.c[0]; A.cy = crop.c[1]; A.cz = crop.c[2];
  A.range_sq = crop.range_sq;
  A.src = rows_of(src->rows[src->cur], stride > 0);
  A.mx = X.mx.p; A.my = X.my.p; A.mz = X.mz.p;
  A.key = X.key.p; A.val = X.val.p;
  A.skey = X.key2.p; A.sval = X.val2.p;
  A.flag = X.flag.p; A.pos = X.pos.p; A.heads = X.heads.p;
  A.rank = X.rank.p; A.mpos = X.mpos.p;
  A.kept_points = X.total.p; A.res = X.res.p;
  sicp::MergeReduceArgs R;  // (the flags of the runs' first pairs: merge's heads launch)
  std::memset(&R, 0, sizeof R);
  R.n = n; R.voxel = 1;
  R.skey = X.key2.p; R.flag = X.flag.p;
  sicp::MapFoldArgs F;  // (the runs' keys among dst's: integrate's rank merge)
  std::memset(&F, 0, sizeof F);
  F.n = n; F.n_map = n_map; F.n_new = 0; F.stride = stride;
  F.skey = X.key2.p; F.heads = X.heads.p;
  F.rank = X.rank.p; F.miss = X.miss.p; F.mpos = X.mpos.p;
  F.miss_key = X.miss_key.p; F.miss_rank = X.miss_rank.p;
  F.res = X.res.p;
  F.from = rows_of(cur, stride > 0);

  log.mark("begin");
  MAPCHECK(hipMemsetAsync(X.res.p, 0, sizeof(int) * sicp::kMapRes, st));
  MAPCHECK(hipMemsetAsync(X.total.p, 0, sizeof(unsigned long long), st));
  MAPCHECK(sicp::launch_map_merge_keys(A, st));
  log.mark("key");
  MAPCHECK(sicp::prim_sort_pairs(X.temp.p, pair_bytes, X.key.p, X.key2.p, X.val.p, X.val2.p, n, 0, 64, st));
  log.mark("sort");
  MAPCHECK(sicp::launch_merge_heads(R, st));
  MAPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, n, st));
  MAPCHECK(sicp::launch_map_merge_runs(A, st));
  log.mark("runs");
  MAPCHECK(sicp::launch_map_lookup(F, st));
  MAPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.miss.p, X.mpos.p, n, st));
  MAPCHECK(sicp::launch_map_misses(F, st));
  log.mark("lookup");
  int res[sicp::kMapRes];
  unsigned long long kept_points = 0;
  MAPCHECK(hipMemcpyAsync(m->stage.data(), X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
  MAPCHECK(hipMemcpyAsync(m->stage.data() + sizeof res, X.total.p, sizeof kept_points, hipMemcpyDeviceToHost, st));
  MAPCHECK(hipStreamSynchronize(st));
  std::memcpy(res, m->stage.data(), sizeof res);
  std::memcpy(&kept_points, m->stage.data() + sizeof res, sizeof kept_points);
  X.idle = true;
  // every refusal lies before the first write to a row
  if (res[sicp::kMapRange])
    return refuse("dst's leaf size " + std::to_string(m->params.leaf_size) + " is too small for the moved rows: a voxel coordinate reaches 2^20");
  const int n_kept = res[sicp::kMapKept], n_runs = res[sicp::kMapScanVoxels], n_new = res[sicp::kMapNew];
  I.n_kept_rows = n_kept;
  I.n_kept_points = (int64_t)kept_points;
  I.n_touched = n_runs;
  I.n_new_voxels = n_new;
  if (n_kept == 0) {
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    return SICP_OK;
  }
  if (m->n_voxels + (long long)n_new > 0x7fffffffll) return refuse("dst would hold more than 2^31 - 1 voxels");
  if (m->n_points + kept_points > 0xffffffffull) return refuse("dst would hold more than 2^32 - 1 points");
  const size_t rows = (size_t)n_map + (size_t)n_new;
  X.idle = false;
  MAPCHECK(reserve_rows(spare, rows, stride));
  MAPCHECK(X.src_of.reserve(rows));
  F.n_new = n_new;
  F.src_of = X.src_of.p;
  F.to = rows_of(spare, stride > 0);
  A.n_new = n_new; A.n_runs = n_runs; A.n_kept = n_kept;
  A.to = F.to;
  MAPCHECK(sicp::launch_map_scatter(F, st));
  if (stride > 0) MAPCHECK(sicp::launch_map_move_hist(F.from.hist, F.to.hist, F.src_of, (long long)rows, stride, st));
  log.mark("scatter");
  MAPCHECK(sicp::launch_map_merge_fold_sums(A, st));
  log.mark("fold_sums");
  if (stride > 0) {
    MAPCHECK(sicp::launch_map_merge_fold_hist(A, st));
    log.mark("fold_hist");
  }
  MAPCHECK(hipMemcpyAsync(m->stage.data(), X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
  MAPCHECK(hipStreamSynchronize(st));
  std::memcpy(res, m->stage.data(), sizeof res);
  X.idle = true;
  m->cur ^= 1;
  m->n_voxels = (long long)rows;
  m->n_points += kept_points;
  I.max_run = res[sicp::kMapMaxCount];
  I.n_voxels = m->n_voxels;
  log.print("sicp_map_merge: n_src=" + std::to_string(n) + " n_kept=" + std::to_string(n_kept) + " n_map=" + std::to_string(n_map) +
            " n_touched=" + std::to_string(n_runs) + " n_new=" + std::to_string(n_new));
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

// sicp_map_get_state: the stored rows through pinned memory -- key | sx | sy | sz (the 8-byte arrays first) | count | hist
int map_get_state(sicp_map_ctx* m, int64_t capacity, uint64_t* key, double* sums, uint32_t* count, uint32_t* hist, int64_t* n_rows) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  const long long n = m->n_voxels;
  if (n_rows) *n_rows = n;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_get_state: " + why + "; no array was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  const int stride = stride_of(m);
  if (hist && stride == 0) return refuse("the map keeps no labels: there are no histograms");
  const bool want_arrays = key || sums || count || hist;
  if (want_arrays && capacity < n) return refuse("the map has " + std::to_string(n) + " rows, the arrays hold " + std::to_string(capacity));
  if (!want_arrays || n == 0) return SICP_OK;
  MAPCHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t nr = (size_t)n;
  const size_t hist_words = hist ? nr * (size_t)stride : 0;
  MAPCHECK(m->out.resize(9 * nr + hist_words));
  uint32_t* const o = m->out.data();
  sicp_map_ctx::Rows& cur = m->rows[m->cur];
  if (key) MAPCHECK(hipMemcpyAsync(o, cur.key.p, 8 * nr, hipMemcpyDeviceToHost, st));
  if (sums) {
    MAPCHECK(hipMemcpyAsync(o + 2 * nr, cur.sx.p, 8 * nr, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipMemcpyAsync(o + 4 * nr, cur.sy.p, 8 * nr, hipMemcpyDeviceToHost, st));
    MAPCHECK(hipMemcpyAsync(o + 6 * nr, cur.sz.p, 8 * nr, hipMemcpyDeviceToHost, st));
  }
  if (count) MAPCHECK(hipMemcpyAsync(o + 8 * nr, cur.cnt.p, 4 * nr, hipMemcpyDeviceToHost, st));
  if (hist) MAPCHECK(hipMemcpyAsync(o + 9 * nr, cur.hist.p, 4 * hist_words, hipMemcpyDeviceToHost, st));
  MAPCHECK(hipStreamSynchronize(st));
  if (key) std::memcpy(key, o, 8 * nr);
  if (sums) {
    const double* s = reinterpret_cast<const double*>(o + 2 * nr);
    for (size_t r = 0; r < nr; ++r) {
      sums[3 * r + 0] = s[r]; sums[3 * r + 1] = s[nr + r]; sums[3 * r + 2] = s[2 * nr + r];
    }
  }
  if (count) std::memcpy(count, o + 8 * nr, 4 * nr);
  if (hist) std::memcpy(hist, o + 9 * nr, 4 * hist_words);
  return SICP_OK;
}

// sicp_map_set_state: every row is checked on the host, then the arrays go up through pinned memory into the spare set
int map_set_state(sicp_map_ctx* m, int64_t n, const uint64_t* key, const double* sums, const uint32_t* count, const uint32_t* hist) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_set_state: " + why + "; the map is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  const int stride = stride_of(m);
  if (n < 0) return refuse("n is negative");
  if (n > 0x7fffffffll) return refuse("more than 2^31 - 1 rows");
  if (hist && stride == 0) return refuse("the map keeps no labels: it takes no histograms");
  if (n > 0 && (!key || !sums || !count)) return refuse("key, sums or count is NULL");
  if (n > 0 && stride > 0 && !hist) return refuse("hist is NULL and the map keeps " + std::to_string(m->params.num_classes) + " classes");
  const size_t nr = (size_t)n;
  unsigned long long points = 0;
  for (size_t r = 0; r < nr; ++r) {
    const std::string row = "row " + std::to_string(r);
    const uint64_t k = key[r];
    if (r > 0 && !(key[r - 1] < k)) return refuse(row + ": the keys do not ascend strictly");
    if ((k >> 63) != 0 || (k & 0x1fffffull) == 0 || ((k >> 21) & 0x1fffffull) == 0 || ((k >> 42) & 0x1fffffull) == 0)
      return refuse(row + ": no point has the key " + std::to_string(k) + " (its top bit is set or a 21-bit field is 0)");
    if (count[r] == 0u) return refuse(row + ": the count is 0");
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(sums[3 * r + d])) return refuse(row + ": a sum is not finite");
    if (stride > 0) {
      unsigned long long h = 0;
      for (int b = 0; b < stride; ++b) h += hist[r * (size_t)stride + b];
      if (h != count[r]) return refuse(row + ": the histogram adds up to " + std::to_string(h) + ", the count is " + std::to_string(count[r]));
    }
    points += count[r];
    if (points > 0xffffffffull) return refuse(row + ": more than 2^32 - 1 points up to this row");
  }
  if (n == 0) {
    m->n_voxels = 0;
    m->n_points = 0;
    return SICP_OK;
  }
  MAPCHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  sicp_map_ctx::Rows& spare = m->rows[m->cur ^ 1];
  const size_t hist_words = nr * (size_t)stride;
  MAPCHECK(m->out.resize(9 * nr + hist_words));
  MAPCHECK(reserve_rows(spare, nr, stride));
  uint32_t* const o = m->out.data();
  std::memcpy(o, key, 8 * nr);
  double* const s = reinterpret_cast<double*>(o + 2 * nr);
  for (size_t r = 0; r < nr; ++r) {
    s[r] = sums[3 * r + 0]; s[nr + r] = sums[3 * r + 1]; s[2 * nr + r] = sums[3 * r + 2];
  }
  std::memcpy(o + 8 * nr, count, 4 * nr);
  if (stride > 0) std::memcpy(o + 9 * nr, hist, 4 * hist_words);
  MAPCHECK(hipMemcpyAsync(spare.key.p, o, 8 * nr, hipMemcpyHostToDevice, st));
  MAPCHECK(hipMemcpyAsync(spare.sx.p, o + 2 * nr, 8 * nr, hipMemcpyHostToDevice, st));
  MAPCHECK(hipMemcpyAsync(spare.sy.p, o + 4 * nr, 8 * nr, hipMemcpyHostToDevice, st));
  MAPCHECK(hipMemcpyAsync(spare.sz.p, o + 6 * nr, 8 * nr, hipMemcpyHostToDevice, st));
  MAPCHECK(hipMemcpyAsync(spare.cnt.p, o + 8 * nr, 4 * nr, hipMemcpyHostToDevice, st));
  if (stride > 0) MAPCHECK(hipMemcpyAsync(spare.hist.p, o + 9 * nr, 4 * hist_words, hipMemcpyHostToDevice, st));
  MAPCHECK(hipStreamSynchronize(st));
  m->cur ^= 1;
  m->n_voxels = n;
  m->n_points = points;
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
