// elevation.cpp -- sicp_map_elevation (include/sicp.h, "elevation"): argument checks, the window and the level bounds formed on
// the host, then the kernels of elevation_kernels.hip queued on the map's stream -- init, keys, the stable sort, heads, their
// scan, the occupied cells, the cell walk, the stencil and, with a handle, the points -- with no host synchronisation between
// them.  One read-back through the map's pinned buffer ends the call; a caller's array is touched only after it.  The map is
// only read; the handle's caller-order arrays are read (valid in every layout) and nothing it holds for align() is touched.
#include <limits>

#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

#define ELEVCHECK(expr)                                                                        \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      m->last_error = std::string("sicp_map_elevation: ") + #expr + ": " + hipGetErrorString(_e) + "; nothing was written"; \
      return _e == hipErrorOutOfMemory ? SICP_ERR_OUT_OF_MEMORY : SICP_ERR_HIP;                \
    }                                                                                          \
  } while (0)

// A call's device scratch: taken from the arena, given back at the end (`idle`: the stream has been synchronised behind the
// call's launches).
struct ElevationScratch {
  DevBuf<unsigned char> temp, state, neighbors, cls;
  DevBuf<unsigned long long> key, skey;
  DevBuf<int> val, sval, flag, pos, occ_cell, occ_begin, ctl, level_top, level_bottom, n_levels, keep, point_cell;
  DevBuf<float> elevation, bottom, ceiling, step, point_height;
  DevBuf<uint32_t> label, count;
  int device = -1;
  bool idle = true;
  ~ElevationScratch() {
    DevArena::release_scratch(device, idle, temp, state, neighbors, cls, key, skey, val, sval, flag, pos, occ_cell, occ_begin, ctl, level_top,
                              level_bottom, n_levels, keep, point_cell, elevation, bottom, ceiling, step, point_height, label, count);
  }
};

constexpr int kLevelMax = sicp::kMergeBias - 1;  // |voxel coordinate| < 2^20

// floorf((float)v * inv_leaf) clamped to lo .. hi (v is not NaN; an infinity goes to its end)
int level_of(double v, float inv_leaf, int lo, int hi) {
  const float f = std::floor((float)v * inv_leaf);
  if (!(f > (float)lo)) return lo;
  if (!(f < (float)hi)) return hi;
  return (int)f;
}

int fdiv(int a, int b) {
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

constexpr size_t kKeepPinnedWords = (size_t)16 << 20;  // 64 MB: a pinned read-back buffer above this is not kept between calls

size_t words(size_t bytes) { return (bytes + 7) / 8 * 2; }  // a read-back region in 32-bit words, 8-byte aligned

}  // namespace

void map_default_elevation_params(sicp_map_elevation_params* p) {
  std::memset(p, 0, sizeof *p);
  p->z_min = -std::numeric_limits<double>::infinity();
  p->z_max = std::numeric_limits<double>::infinity();
  p->max_step = std::numeric_limits<double>::infinity();
  p->cell_voxels = 1;
  p->min_count = 1;
  p->clearance_voxels = 10;
  p->max_extent_voxels = 2;
}

int map_elevation(sicp_map_ctx* m, const double* center, const sicp_map_elevation_params* p, const sicp_map_elevation_out* out,
                  sicp_context* h, int which, const double* qt, sicp_map_elevation_info* info) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_elevation: " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!p) return refuse("the params are NULL");
  if (!center) return refuse("the centre is NULL");
  if (p->width < 1 || p->width > 2048 || p->height < 1 || p->height > 2048) return refuse("width and height must be 1..2048");
  if (p->cell_voxels < 1 || p->cell_voxels > 8) return refuse("cell_voxels must be 1..8");
  if (p->min_count < 1) return refuse("min_count must be >= 1");
  if (std::isnan(p->z_min) || std::isnan(p->z_max) || !(p->z_min <= p->z_max)) return refuse("z_min and z_max must not be NaN, and z_min <= z_max");
  if (p->clearance_voxels < 1) return refuse("clearance_voxels must be >= 1");
  if (p->use_ref_z != 0 && p->use_ref_z != 1) return refuse("use_ref_z is neither 0 nor 1");
  if (p->use_ref_z && !std::isfinite(p->ref_z)) return refuse("ref_z must be finite with use_ref_z = 1");
  if (p->max_extent_voxels < 0) return refuse("max_extent_voxels must be >= 0");
  if (!(p->min_clearance >= 0.0)) return refuse("min_clearance must be >= 0 (0: the test is off)");
  if (!(p->max_step >= 0.0)) return refuse("max_step must be >= 0 (+inf: the test is off)");
  if (p->min_neighbors < 0 || p->min_neighbors > 8) return refuse("min_neighbors must be 0..8");
  const int C = m->params.num_classes, stride = C > 0 ? C + 1 : 0;
  const struct { const char* name; int n; const uint32_t* l; } lists[3] = {
      {"ignore", p->n_ignore, p->ignore}, {"blocked", p->n_blocked, p->blocked}, {"drivable", p->n_drivable, p->drivable}};
  for (const auto& L : lists) {
    const std::string name = L.name;
    if (L.n < 0 || L.n > SICP_MAP_ELEVATION_MAX_LABELS) return refuse("n_" + name + " must be 0.." + std::to_string(SICP_MAP_ELEVATION_MAX_LABELS));
    if (L.n > 0 && C == 0) return refuse("the map keeps no labels: " + name + " must be empty");
    for (int j = 0; j < L.n; ++j)
      if (L.l[j] > (uint32_t)C) return refuse(name + "[" + std::to_string(j) + "] = " + std::to_string(L.l[j]) + " is above num_classes = " + std::to_string(C));
  }
  for (int d = 0; d < 2; ++d)
    if (!std::isfinite(center[d])) return refuse("the centre must be finite");
  const float inv_leaf = 1.0f / (float)m->params.leaf_size;
  int vc[2];
  for (int d = 0; d < 2; ++d) {
    const float f = std::floor((float)center[d] * inv_leaf);
    if (!(std::fabs(f) < (float)sicp::kMergeBias)) return refuse("the centre lies beyond the key's range: a voxel coordinate reaches 2^20");
    vc[d] = (int)f;
  }
  if (qt)
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(qt[k])) return refuse("the pose is not finite");
  const bool point_out = out && (out->point_cell || out->point_height);
  if (point_out && !h) return refuse("point outputs need a handle");
  Cloud* cloud = nullptr;
  if (h) {
    if (which != SICP_SOURCE && which != SICP_TARGET) return refuse("`which` is neither SICP_SOURCE nor SICP_TARGET");
    if (h->device != m->device) return refuse("the handle is on device " + std::to_string(h->device) + ", the map on " + std::to_string(m->device));
    cloud = &h->cloud(which);
    if (!cloud->is_set) {
      m->last_error = "sicp_map_elevation: the slot has no cloud; nothing was written";
      return SICP_ERR_NOT_READY;
    }
  }
  const double t_begin = now_ms();
  ELEVCHECK(hipSetDevice(m->device));
  if (cloud) {  // the slot's device copy: the finite points in caller order, prepared as a merge part is (sicp_map_integrate's rule)
    if (cloud->layout < 0) {
      const int rc = prepare_cloud(h, *cloud);
      if (rc != SICP_OK) {
        m->last_error = "sicp_map_elevation: the cloud: " + (h->last_error.empty() ? std::string("not ready") : h->last_error);
        return rc;
      }
    }
    if (cloud->pending && cloud->ready_ev) {  // (the upload runs on the handle's stream, the kernels below on the map's)
      ELEVCHECK(hipEventSynchronize(cloud->ready_ev));
      cloud->pending = false;
    }
  }
  const int W = p->width, H = p->height, B = p->cell_voxels;
  const size_t cells = (size_t)W * (size_t)H;
  const int n_map = (int)m->n_voxels;
  const size_t nr = (size_t)std::max(n_map, 1);
  const int n = cloud ? cloud->n : 0, nc = cloud ? cloud->n_caller : 0;
  const bool mapped = cloud && !cloud->keep.empty();
  hipStream_t st = m->stream;

  sicp::MapElevationArgs A;
  std::memset(&A, 0, sizeof A);
  A.rows.key = m->rows[m->cur].key.p; A.rows.sx = m->rows[m->cur].sx.p; A.rows.sy = m->rows[m->cur].sy.p; A.rows.sz = m->rows[m->cur].sz.p;
  A.rows.cnt = m->rows[m->cur].cnt.p; A.rows.hist = stride > 0 ? m->rows[m->cur].hist.p : nullptr;
  A.n_map = n_map; A.stride = stride;
  A.W = W; A.H = H; A.B = B;
  A.x0 = fdiv(vc[0], B) - W / 2; A.y0 = fdiv(vc[1], B) - H / 2;
  A.lo = level_of(p->z_min, inv_leaf, -kLevelMax, kLevelMax);
  A.hi = level_of(p->z_max, inv_leaf, -kLevelMax, kLevelMax);
  A.min_count = p->min_count;
  A.clearance = p->clearance_voxels;
  A.use_ref = p->use_ref_z;
  A.vref = p->use_ref_z ? level_of(p->ref_z, inv_leaf, -sicp::kMergeBias, sicp::kMergeBias) : 0;
  A.max_extent = p->max_extent_voxels; A.min_neighbors = p->min_neighbors;
  A.min_clearance = p->min_clearance; A.max_step = p->max_step;
  A.n_ignore = p->n_ignore; A.n_blocked = p->n_blocked; A.n_drivable = p->n_drivable;
  for (int j = 0; j < p->n_ignore; ++j) A.ignore[j] = p->ignore[j];
  for (int j = 0; j < p->n_blocked; ++j) A.blocked[j] = p->blocked[j];
  for (int j = 0; j < p->n_drivable; ++j) A.drivable[j] = p->drivable[j];
  const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
  matrix34(qt ? qt : ident, A.M);
  A.n = n; A.n_caller = nc; A.inv_leaf = inv_leaf;

  // the read-back's places in the pinned buffer: the control words, then every array somebody asked for
  void* wanted[14] = {};
  if (out) {
    void* w[14] = {out->state, out->elevation, out->bottom, out->ceiling, out->label, out->count, out->level_top,
                         out->level_bottom, out->n_levels, out->step, out->neighbors, out->cell_class, out->point_cell, out->point_height};
    std::memcpy(wanted, w, sizeof w);
  }
  const size_t elem[14] = {1, 4, 4, 4, 4, 4, 4, 4, 4, 4, 1, 1, 4, 4};
  size_t at[15];
  at[0] = words(sizeof(int) * sicp::kElevCtl);
  for (int k = 0; k < 14; ++k) {
    const size_t count = k < 12 ? cells : (size_t)nc;
    at[k + 1] = at[k] + (wanted[k] ? words(elem[k] * count) : 0);
  }

  ElevationScratch X;
  X.device = m->device;
  X.idle = false;
  ELEVCHECK(X.ctl.reserve(sicp::kElevCtl));
  ELEVCHECK(X.state.reserve(cells)); ELEVCHECK(X.neighbors.reserve(cells)); ELEVCHECK(X.cls.reserve(cells));
  ELEVCHECK(X.elevation.reserve(cells)); ELEVCHECK(X.bottom.reserve(cells)); ELEVCHECK(X.ceiling.reserve(cells)); ELEVCHECK(X.step.reserve(cells));
  ELEVCHECK(X.label.reserve(cells)); ELEVCHECK(X.count.reserve(cells));
  ELEVCHECK(X.level_top.reserve(cells)); ELEVCHECK(X.level_bottom.reserve(cells)); ELEVCHECK(X.n_levels.reserve(cells));
  const int sort_bits = sicp::kElevLevelBits + sicp::elevation_cell_bits((long long)cells);
  size_t pair_bytes = 0, scan_bytes = 0;
  if (n_map > 0) {
    ELEVCHECK(X.key.reserve(nr)); ELEVCHECK(X.skey.reserve(nr)); ELEVCHECK(X.val.reserve(nr)); ELEVCHECK(X.sval.reserve(nr));
    ELEVCHECK(X.flag.reserve(nr)); ELEVCHECK(X.pos.reserve(nr));
    const size_t occ = std::min(nr, cells);
    ELEVCHECK(X.occ_cell.reserve(occ)); ELEVCHECK(X.occ_begin.reserve(occ));
    ELEVCHECK(sicp::prim_sort_pairs(nullptr, pair_bytes, X.key.p, X.skey.p, X.val.p, X.sval.p, n_map, 0, sort_bits, st));
    ELEVCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, n_map, st));
    ELEVCHECK(X.temp.reserve(std::max(pair_bytes, scan_bytes) + 256));
  }
  if (nc > 0) {
    ELEVCHECK(X.point_cell.reserve((size_t)nc)); ELEVCHECK(X.point_height.reserve((size_t)nc));
    if (mapped) ELEVCHECK(X.keep.reserve((size_t)n));
  }
  A.key = X.key.p; A.skey = X.skey.p; A.val = X.val.p; A.sval = X.sval.p;
  A.flag = X.flag.p; A.pos = X.pos.p; A.occ_cell = X.occ_cell.p; A.occ_begin = X.occ_begin.p;
  A.ctl = X.ctl.p;
  A.state = X.state.p; A.neighbors = X.neighbors.p; A.cls = X.cls.p;
  A.elevation = X.elevation.p; A.bottom = X.bottom.p; A.ceiling = X.ceiling.p; A.step = X.step.p;
  A.label = X.label.p; A.count = X.count.p;
  A.level_top = X.level_top.p; A.level_bottom = X.level_bottom.p; A.n_levels = X.n_levels.p;
  if (cloud) {
    A.px = cloud->rx.p; A.py = cloud->ry.p; A.pz = cloud->rz.p;
    A.point_cell = X.point_cell.p; A.point_height = X.point_height.p;
  }
  // The pinned buffer comes last, once the arena has granted the scratch.  One that a large window made larger than
  // kKeepPinnedWords goes back at the call's end (the stream is idle then), so that a 2048 x 2048 call does not leave 160 MB of
  // pinned memory with the map.
  struct PinnedGuard {
    HostBuf<uint32_t>& b;
    const bool& idle;
    ~PinnedGuard() {
      if (b.cap > kKeepPinnedWords && idle) {
        (void)hipHostFree(b.p);
        b.p = nullptr;
        b.cap = b.n = 0;
      }
    }
  } pinned_guard{m->out, X.idle};
  ELEVCHECK(m->out.resize(at[14]));
  uint32_t* const o = m->out.data();
  if (mapped && n > 0) {  // points were dropped: the finite points' caller indices go up through the pinned stage
    ELEVCHECK(m->stage.resize(sizeof(int) * (size_t)n));
    std::memcpy(m->stage.data(), cloud->keep.data(), sizeof(int) * (size_t)n);
    ELEVCHECK(hipMemcpyAsync(X.keep.p, m->stage.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
    A.keep = X.keep.p;
  }
  ELEVCHECK(hipMemsetAsync(X.ctl.p, 0, sizeof(int) * sicp::kElevCtl, st));
  ELEVCHECK(sicp::launch_elevation_init(A, st));
  if (n_map > 0) {
    ELEVCHECK(sicp::launch_elevation_keys(A, st));
    ELEVCHECK(sicp::prim_sort_pairs(X.temp.p, pair_bytes, X.key.p, X.skey.p, X.val.p, X.sval.p, n_map, 0, sort_bits, st));
    ELEVCHECK(sicp::launch_elevation_heads(A, st));
    ELEVCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, n_map, st));
    ELEVCHECK(sicp::launch_elevation_segments(A, st));
    ELEVCHECK(sicp::launch_elevation_cells(A, st));
  }
  ELEVCHECK(sicp::launch_elevation_stencil(A, st));
  if (cloud) ELEVCHECK(sicp::launch_elevation_points(A, st));
  ELEVCHECK(hipMemcpyAsync(o, X.ctl.p, sizeof(int) * sicp::kElevCtl, hipMemcpyDeviceToHost, st));
  const void* from[14] = {X.state.p, X.elevation.p, X.bottom.p, X.ceiling.p, X.label.p, X.count.p, X.level_top.p,
                          X.level_bottom.p, X.n_levels.p, X.step.p, X.neighbors.p, X.cls.p, X.point_cell.p, X.point_height.p};
  for (int k = 0; k < 14; ++k) {
    const size_t bytes = elem[k] * (k < 12 ? cells : (size_t)nc);
    if (wanted[k] && bytes > 0) ELEVCHECK(hipMemcpyAsync(o + at[k], from[k], bytes, hipMemcpyDeviceToHost, st));
  }
  ELEVCHECK(hipStreamSynchronize(st));
  X.idle = true;
  int ctl[sicp::kElevCtl];
  std::memcpy(ctl, o, sizeof ctl);
  for (int k = 0; k < 14; ++k) {
    const size_t bytes = elem[k] * (k < 12 ? cells : (size_t)nc);
    if (wanted[k] && bytes > 0) std::memcpy(wanted[k], o + at[k], bytes);
  }
  if (info) {
    sicp_map_elevation_info I;
    std::memset(&I, 0, sizeof I);
    I.n_voxels = m->n_voxels;
    I.n_points = nc;
    I.x0 = A.x0; I.y0 = A.y0;
    I.width = W; I.height = H;
    for (int k = 0; k < 8; ++k) I.n_class[k] = ctl[sicp::kElevClass + k];
    I.cell_size = (double)B * m->params.leaf_size;
    I.t_total_ms = now_ms() - t_begin;
    *info = I;
  }
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
