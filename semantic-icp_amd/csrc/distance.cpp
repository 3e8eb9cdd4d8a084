// distance.cpp -- sicp_map_distance (include/sicp.h, "distance"): argument checks, the window and the band formed on the host,
// then the kernels of distance_kernels.hip queued on the map's stream -- init, seed, one sweep per axis longer than one cell
// between two key buffers, the unpacking pass and, with a handle, the points -- with no host synchronisation between them.
// One read-back through the map's pinned buffer ends the call; a caller's array is touched only after it.  The map is only
// read; the handle's caller-order arrays are read (valid in every layout) and nothing it holds for align() is touched.
#include <limits>

#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

#define DISTCHECK(expr)                                                                        \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      m->last_error = std::string("sicp_map_distance: ") + #expr + ": " + hipGetErrorString(_e) + "; nothing was written"; \
      return _e == hipErrorOutOfMemory ? SICP_ERR_OUT_OF_MEMORY : SICP_ERR_HIP;                \
    }                                                                                          \
  } while (0)

// A call's device scratch: taken from the arena, given back at the end (`idle`: the stream has been synchronised behind the
// call's launches).
struct DistanceScratch {
  DevBuf<unsigned long long> key_a, key_b;
  DevBuf<int> dist_sq, nearest, ctl, keep, point_cell, point_dist_sq, point_nearest;
  DevBuf<uint32_t> label, row_label;
  DevBuf<float> point_range_sq;
  int device = -1;
  bool idle = true;
  ~DistanceScratch() {
    DevArena::release_scratch(device, idle, key_a, key_b, dist_sq, nearest, ctl, keep, point_cell, point_dist_sq, point_nearest, label, row_label,
                              point_range_sq);
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

constexpr size_t kKeepPinnedWords = (size_t)16 << 20;  // 64 MB: a pinned read-back buffer above this is not kept between calls
constexpr long long kMaxCells = 1ll << 24;
constexpr int kArrays = 7;

size_t words(size_t bytes) { return (bytes + 7) / 8 * 2; }  // a read-back region in 32-bit words, 8-byte aligned

}  // namespace

void map_default_distance_params(sicp_map_distance_params* p) {
  std::memset(p, 0, sizeof *p);
  p->z_min = -std::numeric_limits<double>::infinity();
  p->z_max = std::numeric_limits<double>::infinity();
  p->max_dist_voxels = 10;
  p->min_count = 1;
}

int map_distance(sicp_map_ctx* m, const double* center, const sicp_map_distance_params* p, const sicp_map_distance_out* out,
                 sicp_context* h, int which, const double* qt, sicp_map_distance_info* info) {
  if (!m) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    m->last_error = "sicp_map_distance: " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!p) return refuse("the params are NULL");
  if (!center) return refuse("the centre is NULL");
  if (p->nx < 1 || p->nx > 1024 || p->ny < 1 || p->ny > 1024) return refuse("nx and ny must be 1..1024");
  if (p->nz < 1 || p->nz > 256) return refuse("nz must be 1..256");
  if ((long long)p->nx * p->ny * p->nz > kMaxCells) return refuse("nx * ny * nz must be at most 2^24");
  if (p->max_dist_voxels < 1 || p->max_dist_voxels > sicp::kDistMaxR) return refuse("max_dist_voxels must be 1..64");
  if (p->min_count < 1) return refuse("min_count must be >= 1");
  if (p->planar != 0 && p->planar != 1) return refuse("planar is neither 0 nor 1");
  if (p->planar && p->nz != 1) return refuse("planar = 1 needs nz = 1");
  if (std::isnan(p->z_min) || std::isnan(p->z_max) || !(p->z_min <= p->z_max)) return refuse("z_min and z_max must not be NaN, and z_min <= z_max");
  const int C = m->params.num_classes, stride = C > 0 ? C + 1 : 0;
  const struct { const char* name; int n; const uint32_t* l; } lists[2] = {{"ignore", p->n_ignore, p->ignore}, {"only", p->n_only, p->only}};
  for (const auto& L : lists) {
    const std::string name = L.name;
    if (L.n < 0 || L.n > SICP_MAP_DISTANCE_MAX_LABELS) return refuse("n_" + name + " must be 0.." + std::to_string(SICP_MAP_DISTANCE_MAX_LABELS));
    if (L.n > 0 && C == 0) return refuse("the map keeps no labels: " + name + " must be empty");
    for (int j = 0; j < L.n; ++j)
      if (L.l[j] > (uint32_t)C) return refuse(name + "[" + std::to_string(j) + "] = " + std::to_string(L.l[j]) + " is above num_classes = " + std::to_string(C));
  }
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(center[d])) return refuse("the centre must be finite");
  const float inv_leaf = 1.0f / (float)m->params.leaf_size;
  int vc[3] = {0, 0, 0};
  for (int d = 0; d < (p->planar ? 2 : 3); ++d) {
    const float f = std::floor((float)center[d] * inv_leaf);
    if (!(std::fabs(f) < (float)sicp::kMergeBias)) return refuse("the centre lies beyond the key's range: a voxel coordinate reaches 2^20");
    vc[d] = (int)f;
  }
  if (qt)
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(qt[k])) return refuse("the pose is not finite");
  const bool point_out = out && (out->point_cell || out->point_dist_sq || out->point_nearest || out->point_range_sq);
  if (point_out && !h) return refuse("point outputs need a handle");
  if (out && out->point_range_sq && p->planar) return refuse("point_range_sq is a 3-D output: planar must be 0");
  Cloud* cloud = nullptr;
  if (h) {
    if (which != SICP_SOURCE && which != SICP_TARGET) return refuse("`which` is neither SICP_SOURCE nor SICP_TARGET");
    if (h->device != m->device) return refuse("the handle is on device " + std::to_string(h->device) + ", the map on " + std::to_string(m->device));
    cloud = &h->cloud(which);
    if (!cloud->is_set) {
      m->last_error = "sicp_map_distance: the slot has no cloud; nothing was written";
      return SICP_ERR_NOT_READY;
    }
  }
  const double t_begin = now_ms();
  DISTCHECK(hipSetDevice(m->device));
  if (cloud) {  // the slot's device copy: the finite points in caller order, prepared as a merge part is (sicp_map_integrate's rule)
    if (cloud->layout < 0) {
      const int rc = prepare_cloud(h, *cloud);
      if (rc != SICP_OK) {
        m->last_error = "sicp_map_distance: the cloud: " + (h->last_error.empty() ? std::string("not ready") : h->last_error);
        return rc;
      }
    }
    if (cloud->pending && cloud->ready_ev) {  // (the upload runs on the handle's stream, the kernels below on the map's)
      DISTCHECK(hipEventSynchronize(cloud->ready_ev));
      cloud->pending = false;
    }
  }
  const size_t cells = (size_t)p->nx * (size_t)p->ny * (size_t)p->nz;
  const int n_map = (int)m->n_voxels;
  const int n = cloud ? cloud->n : 0, nc = cloud ? cloud->n_caller : 0;
  const bool mapped = cloud && !cloud->keep.empty();
  hipStream_t st = m->stream;

  sicp::MapDistanceArgs A;
  std::memset(&A, 0, sizeof A);
  A.rows.key = m->rows[m->cur].key.p; A.rows.sx = m->rows[m->cur].sx.p; A.rows.sy = m->rows[m->cur].sy.p; A.rows.sz = m->rows[m->cur].sz.p;
  A.rows.cnt = m->rows[m->cur].cnt.p; A.rows.hist = stride > 0 ? m->rows[m->cur].hist.p : nullptr;
  A.n_map = n_map; A.stride = stride;
  A.nx = p->nx; A.ny = p->ny; A.nz = p->nz;
  A.x0 = vc[0] - p->nx / 2; A.y0 = vc[1] - p->ny / 2; A.z0 = p->planar ? 0 : vc[2] - p->nz / 2;
  A.planar = p->planar;
  A.lo = level_of(p->z_min, inv_leaf, -kLevelMax, kLevelMax);
  A.hi = level_of(p->z_max, inv_leaf, -kLevelMax, kLevelMax);
  A.R = p->max_dist_voxels;
  A.min_count = p->min_count;
  A.n_ignore = p->n_ignore; A.n_only = p->n_only;
  for (int j = 0; j < p->n_ignore; ++j) A.ignore[j] = p->ignore[j];
  for (int j = 0; j < p->n_only; ++j) A.only[j] = p->only[j];
  const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
  matrix34(qt ? qt : ident, A.M);
  A.n = n; A.n_caller = nc; A.inv_leaf = inv_leaf;

  // the read-back's places in the pinned buffer: the control words, then every array somebody asked for
  void* wanted[kArrays] = {};
  if (out) {
    void* w[kArrays] = {out->dist_sq, out->nearest, out->label, out->point_cell, out->point_dist_sq, out->point_nearest, out->point_range_sq};
    std::memcpy(wanted, w, sizeof w);
  }
  size_t at[kArrays + 1];
  at[0] = words(sizeof(int) * sicp::kDistCtl);
  for (int k = 0; k < kArrays; ++k) {
    const size_t count = k < 3 ? cells : (size_t)nc;
    at[k + 1] = at[k] + (wanted[k] ? words(4 * count) : 0);
  }

  DistanceScratch X;
  X.device = m->device;
  X.idle = false;
  DISTCHECK(X.ctl.reserve(sicp::kDistCtl));
  DISTCHECK(X.key_a.reserve(cells)); DISTCHECK(X.key_b.reserve(cells));
  DISTCHECK(X.dist_sq.reserve(cells)); DISTCHECK(X.nearest.reserve(cells)); DISTCHECK(X.label.reserve(cells));
  if (n_map > 0 && stride > 0) DISTCHECK(X.row_label.reserve((size_t)n_map));
  if (nc > 0) {
    DISTCHECK(X.point_cell.reserve((size_t)nc)); DISTCHECK(X.point_dist_sq.reserve((size_t)nc));
    DISTCHECK(X.point_nearest.reserve((size_t)nc)); DISTCHECK(X.point_range_sq.reserve((size_t)nc));
    if (mapped) DISTCHECK(X.keep.reserve((size_t)n));
  }
  A.key = X.key_a.p;
  A.row_label = X.row_label.p;
  A.ctl = X.ctl.p;
  A.dist_sq = X.dist_sq.p; A.nearest = X.nearest.p; A.label = X.label.p;
  if (cloud) {
    A.px = cloud->rx.p; A.py = cloud->ry.p; A.pz = cloud->rz.p;
    A.point_cell = X.point_cell.p; A.point_dist_sq = X.point_dist_sq.p; A.point_nearest = X.point_nearest.p;
    A.point_range_sq = X.point_range_sq.p;
  }
  // The pinned buffer comes last, once the arena has granted the scratch.  One that a large window made larger than
  // kKeepPinnedWords goes back at the call's end (the stream is idle then), so that a 2^24-cell call does not leave 200 MB of
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
  DISTCHECK(m->out.resize(at[kArrays]));
  uint32_t* const o = m->out.data();
  if (mapped && n > 0) {  // points were dropped: the finite points' caller indices go up through the pinned stage
    DISTCHECK(m->stage.resize(sizeof(int) * (size_t)n));
    std::memcpy(m->stage.data(), cloud->keep.data(), sizeof(int) * (size_t)n);
    DISTCHECK(hipMemcpyAsync(X.keep.p, m->stage.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
    A.keep = X.keep.p;
  }
  DISTCHECK(hipMemsetAsync(X.ctl.p, 0, sizeof(int) * sicp::kDistCtl, st));
  DISTCHECK(sicp::launch_distance_init(A, st));
  DISTCHECK(sicp::launch_distance_seed(A, st));
  // a sweep along an axis of one cell is the identity (the cell itself is its only neighbour inside the window): it is skipped
  unsigned long long *src = X.key_a.p, *dst = X.key_b.p;
  const int extent[3] = {p->nx, p->ny, p->nz};
  for (int axis = 0; axis < 3; ++axis) {
    if (extent[axis] == 1) continue;
    DISTCHECK(sicp::launch_distance_sweep(A, axis, src, dst, st));
    std::swap(src, dst);
  }
  DISTCHECK(sicp::launch_distance_final(A, src, st));
  if (cloud) DISTCHECK(sicp::launch_distance_points(A, st));
  DISTCHECK(hipMemcpyAsync(o, X.ctl.p, sizeof(int) * sicp::kDistCtl, hipMemcpyDeviceToHost, st));
  const void* from[kArrays] = {X.dist_sq.p, X.nearest.p, X.label.p, X.point_cell.p, X.point_dist_sq.p, X.point_nearest.p, X.point_range_sq.p};
  for (int k = 0; k < kArrays; ++k) {
    const size_t bytes = 4 * (k < 3 ? cells : (size_t)nc);
    if (wanted[k] && bytes > 0) DISTCHECK(hipMemcpyAsync(o + at[k], from[k], bytes, hipMemcpyDeviceToHost, st));
  }
  DISTCHECK(hipStreamSynchronize(st));
  X.idle = true;
  int ctl[sicp::kDistCtl];
  std::memcpy(ctl, o, sizeof ctl);
  for (int k = 0; k < kArrays; ++k) {
    const size_t bytes = 4 * (k < 3 ? cells : (size_t)nc);
    if (wanted[k] && bytes > 0) std::memcpy(wanted[k], o + at[k], bytes);
  }
  if (info) {
    sicp_map_distance_info I;
    std::memset(&I, 0, sizeof I);
    I.n_voxels = m->n_voxels;
    I.n_points = nc;
    I.n_points_inside = ctl[sicp::kDistInside];
    I.x0 = A.x0; I.y0 = A.y0; I.z0 = A.z0;
    I.nx = p->nx; I.ny = p->ny; I.nz = p->nz;
    I.n_obstacles = ctl[sicp::kDistObstacles];
    I.n_reached = ctl[sicp::kDistReached];
    I.max_dist_sq = ctl[sicp::kDistMaxPlus1] - 1;
    I.voxel_size = m->params.leaf_size;
    I.t_total_ms = now_ms() - t_begin;
    *info = I;
  }
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
