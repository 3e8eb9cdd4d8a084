// ground.cpp -- sicp_segment_ground (include/sicp.h, "ground of a cloud"): argument checks, the ring and sector tables formed
// on the host, then the kernels of ground_kernels.hip queued on the handle's stream -- keys, the stable sort, the segments and
// the dense sorted coordinates, the fit (a wave per cell), the per-point flag and height, with select a scan and a gather --
// with no host synchronisation between them.  One read-back of the control block, the cell rows and the per-point outputs
// ends the call; with dst one more of the selected points, staged into dst's slot through the path of sicp_set_cloud
// (filter.cpp).  Without dst nothing the handle holds for align() is touched: the call reads the cloud's caller-order arrays
// (valid in every layout) and writes scratch of its own.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

// A call's device scratch: taken from the arena, given back at the end (DevArena::release_scratch: `idle` once the stream
// has been synchronised behind the call's launches).
struct GroundScratch {
  DevBuf<unsigned char> temp, mask, cand, oground;
  DevBuf<unsigned long long> key, skey;
  DevBuf<int> finv, val, sval, cellv, seg, flag, pos;
  DevBuf<float> sx, sy, sz, gx, gy, gz;
  DevBuf<uint32_t> gl;
  DevBuf<double> tables, oheight;
  DevBuf<sicp::GroundCell> cells;
  DevBuf<sicp::GroundCtl> ctl;
  int device = -1;
  bool idle = true;
  ~GroundScratch() {
    DevArena::release_scratch(device, idle, temp, mask, cand, oground, key, skey, finv, val, sval, cellv, seg, flag, pos, sx, sy, sz, gx, gy,
                              gz, gl, tables, oheight, cells, ctl);
  }
};

constexpr double kTwoPi = 6.283185307179586;

bool slot_ok(int which) { return which == SICP_SOURCE || which == SICP_TARGET; }
size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

// rule 9's checks of the parameters and the ring table; an empty string: accepted
std::string params_refused(const sicp_ground_params* p, const double* ring_edge) {
  const double d[9] = {p->min_range, p->max_range, p->sensor_height, p->max_below, p->th_seeds, p->th_dist, p->min_cos, p->max_elevation,
                       p->max_thickness};
  for (double v : d)
    if (!std::isfinite(v)) return "every double of the params must be finite";
  if (p->min_range < 0.0) return "min_range must be >= 0";
  if (!(p->max_range > p->min_range)) return "max_range must be > min_range";
  if (p->n_rings < 1 || p->n_rings > SICP_GROUND_MAX_RINGS) return "n_rings must be in 1 .. " + std::to_string(SICP_GROUND_MAX_RINGS);
  if (p->n_sectors < 4 || p->n_sectors > SICP_GROUND_MAX_SECTORS || p->n_sectors % 2 != 0)
    return "n_sectors must be even and in 4 .. " + std::to_string(SICP_GROUND_MAX_SECTORS);
  if (ring_edge) {
    for (int i = 0; i <= p->n_rings; ++i)
      if (!std::isfinite(ring_edge[i])) return "ring_edge must be finite";
    if (ring_edge[0] < 0.0) return "ring_edge[0] must be >= 0";
    for (int i = 0; i < p->n_rings; ++i)
      if (!(ring_edge[i + 1] > ring_edge[i])) return "ring_edge must be strictly ascending";
  }
  if (p->n_lpr < 1 || p->n_lpr > 64) return "n_lpr must be in 1 .. 64";
  if (p->n_iter < 1 || p->n_iter > 8) return "n_iter must be in 1 .. 8";
  if (p->min_points < 3) return "min_points must be >= 3";
  if (!(p->min_cos > 0.0 && p->min_cos <= 1.0)) return "min_cos must be in (0, 1]";
  if (!(p->th_dist > 0.0)) return "th_dist must be > 0";
  if (!(p->th_seeds > 0.0)) return "th_seeds must be > 0";
  if (p->max_thickness < 0.0) return "max_thickness must be >= 0 (0: the thickness test is off)";
  if (p->elevation_rings < 0 || p->elevation_rings > p->n_rings) return "elevation_rings must be in 0 .. n_rings";
  if (p->n_ignore < 0 || p->n_ignore > SICP_GROUND_MAX_IGNORE) return "n_ignore must be in 0 .. " + std::to_string(SICP_GROUND_MAX_IGNORE);
  if (p->select < 0 || p->select > 2) return "select must be 0, 1 or 2";
  return std::string();
}

// rule 2: edge2 [R+1] | cos_half [S/2] | sin_half [S/2]
void form_tables(const sicp_ground_params* p, const double* ring_edge, double* t) {
  const int R = p->n_rings, S = p->n_sectors;
  const double ring_step = (p->max_range - p->min_range) / (double)R, sector_step = kTwoPi / (double)S;
  for (int i = 0; i <= R; ++i) {
    const double b = ring_edge ? ring_edge[i] : p->min_range + (double)i * ring_step;
    t[i] = b * b;
  }
  double *cos_half = t + R + 1, *sin_half = cos_half + S / 2;
  for (int j = 0; j < S / 2; ++j) {
    const double a = (double)j * sector_step;
    cos_half[j] = std::cos(a);
    sin_half[j] = std::sin(a);
  }
}

}  // namespace

void ground_default_params(sicp_ground_params* p) {
  std::memset(p, 0, sizeof *p);
  p->min_range = 2.7;
  p->max_range = 80.0;
  p->sensor_height = 1.73;
  p->max_below = 1.0;
  p->th_seeds = 0.5;
  p->th_dist = 0.2;
  p->min_cos = 0.707;
  p->max_elevation = 0.5;
  p->max_thickness = 0.0;
  p->n_rings = 16;
  p->n_sectors = 32;
  p->n_lpr = 20;
  p->n_iter = 3;
  p->min_points = 10;
  p->elevation_rings = 4;
  p->select = 0;
  p->n_ignore = 0;
}

int ground_tables(const sicp_ground_params* p, const double* ring_edge, double* cos_half, double* sin_half, double* edge2) {
  if (!p || !params_refused(p, ring_edge).empty()) return SICP_ERR_INVALID_ARGUMENT;
  const int R = p->n_rings, S = p->n_sectors;
  std::vector<double> t((size_t)(R + 1 + S));
  form_tables(p, ring_edge, t.data());
  if (edge2) std::memcpy(edge2, t.data(), sizeof(double) * (size_t)(R + 1));
  if (cos_half) std::memcpy(cos_half, t.data() + R + 1, sizeof(double) * (size_t)(S / 2));
  if (sin_half) std::memcpy(sin_half, t.data() + R + 1 + S / 2, sizeof(double) * (size_t)(S / 2));
  return SICP_OK;
}

int segment_ground(sicp_context* h, int which, const sicp_ground_params* p, const uint8_t* mask, const double* sensor_origin,
                   const double* ring_edge, sicp_context* dst, int dst_which, const sicp_ground_out* out, sicp_ground_info* info) {
  if (!h) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    h->last_error = "sicp_segment_ground: " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!p) return refuse("the params are NULL");
  if (!slot_ok(which)) return refuse("which is neither SICP_SOURCE nor SICP_TARGET");
  if (dst && !slot_ok(dst_which)) return refuse("dst_which is neither SICP_SOURCE nor SICP_TARGET");
  if (dst && dst->device != h->device) return refuse("dst is on device " + std::to_string(dst->device) + ", the handle on " + std::to_string(h->device));
  if (sensor_origin)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(sensor_origin[k])) return refuse("sensor_origin must be finite");
  {
    const std::string why = params_refused(p, ring_edge);
    if (!why.empty()) return refuse(why);
  }
  if (p->select != 0 && !dst) return refuse("select = " + std::to_string(p->select) + " needs a dst");
  if (out && out->capacity < 0) return refuse("capacity must be >= 0");
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    h->last_error = "sicp_segment_ground: the slot holds no cloud";
    return SICP_ERR_NOT_READY;
  }
  if (!c.has_label && p->n_ignore != 0) return refuse("the cloud was set without labels: only an empty ignore list can segment it");
  const double t_begin = now_ms();
  SICPCHECK(set_device(h));
  // the cloud's device copy: the finite points in caller order (Cloud::rx ..., valid in every layout), prepared as a merge part is
  if (c.layout < 0) SICPCHECK(prepare_cloud(h, c));
  SICPCHECK(cloud_wait(h, c));
  const int n = c.n, nc = c.n_caller;
  const int R = p->n_rings, S = p->n_sectors, RS = R * S;
  const bool labels = c.has_label, mapped = !c.keep.empty();
  const bool select = dst != nullptr && p->select != 0;
  hipStream_t st = h->stream;
  GroundScratch X;
  sicp::GroundArgs A;
  std::memset(&A, 0, sizeof A);
  sicp::GroundCtl ctl;
  // pinned: tables | finite positions | mask on their way up; the control block | the cell rows | ground | cell | height on
  // their way back
  const size_t mc = (size_t)std::max(nc, 1), n_tab = (size_t)(R + 1 + S);
  const size_t o_tab = 0, o_finv = o_tab + 8 * n_tab, o_mask = o_finv + up8(mapped ? 4 * mc : 0), o_ctl = o_mask + up8(mask ? mc : 0),
               o_cells = o_ctl + up8(sizeof ctl), o_height = o_cells + sizeof(sicp::GroundCell) * (size_t)RS, o_cell = o_height + 8 * mc,
               o_ground = o_cell + up8(4 * mc), o_end = o_ground + up8(mc);
  HIPCHECK(h->gr_stage.resize(o_end));
  unsigned char* o = h->gr_stage.data();
  X.device = h->device;
  X.idle = false;
  HIPCHECK(X.tables.reserve(n_tab)); HIPCHECK(X.ctl.reserve(1)); HIPCHECK(X.cells.reserve((size_t)RS)); HIPCHECK(X.seg.reserve(2 * (size_t)(RS + 1)));
  HIPCHECK(X.key.reserve(mc)); HIPCHECK(X.skey.reserve(mc)); HIPCHECK(X.val.reserve(mc)); HIPCHECK(X.sval.reserve(mc));
  HIPCHECK(X.cellv.reserve(mc)); HIPCHECK(X.cand.reserve(mc)); HIPCHECK(X.oground.reserve(mc)); HIPCHECK(X.oheight.reserve(mc));
  HIPCHECK(X.sx.reserve(mc)); HIPCHECK(X.sy.reserve(mc)); HIPCHECK(X.sz.reserve(mc));
  size_t pair_bytes = 0, scan_bytes = 0;
  HIPCHECK(sicp::prim_sort_pairs(nullptr, pair_bytes, X.key.p, X.skey.p, X.val.p, X.sval.p, (long long)mc, 0, sicp::kGroundSortBits, st));
  if (select) {
    HIPCHECK(X.flag.reserve(mc)); HIPCHECK(X.pos.reserve(mc));
    HIPCHECK(X.gx.reserve(mc)); HIPCHECK(X.gy.reserve(mc)); HIPCHECK(X.gz.reserve(mc));
    if (labels) HIPCHECK(X.gl.reserve(mc));
    HIPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, (long long)mc, st));
  }
  HIPCHECK(X.temp.reserve(std::max(pair_bytes, scan_bytes) + 256));

  A.n = n; A.n_caller = nc;
  A.labels = labels ? 1 : 0;
  A.R = R; A.S = S;
  A.n_lpr = p->n_lpr; A.n_iter = p->n_iter; A.min_points = p->min_points; A.elevation_rings = p->elevation_rings;
  A.select = select ? p->select : 0;
  A.n_ignore = p->n_ignore;
  for (int k = 0; k < p->n_ignore; ++k) A.ignore[k] = p->ignore[k];
  for (int k = 0; k < 3; ++k) A.org[k] = sensor_origin ? sensor_origin[k] : 0.0;
  A.below = -(p->sensor_height + p->max_below);
  A.elev = -p->sensor_height + p->max_elevation;
  A.th_seeds = p->th_seeds; A.th_dist = p->th_dist; A.min_cos = p->min_cos;
  A.thick2 = p->max_thickness * p->max_thickness;
  A.tables = X.tables.p;
  A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
  A.label = labels ? c.rl.p : nullptr;
  A.key = X.key.p; A.skey = X.skey.p; A.val = X.val.p; A.sval = X.sval.p;
  A.cellv = X.cellv.p; A.cand = X.cand.p;
  A.sx = X.sx.p; A.sy = X.sy.p; A.sz = X.sz.p;
  A.seg_begin = X.seg.p; A.seg_end = X.seg.p + (RS + 1);
  A.cells = X.cells.p;
  A.oground = X.oground.p; A.oheight = X.oheight.p;
  A.flag = X.flag.p; A.pos = X.pos.p;
  A.gx = X.gx.p; A.gy = X.gy.p; A.gz = X.gz.p; A.gl = select && labels ? X.gl.p : nullptr;
  A.ctl = X.ctl.p;
  form_tables(p, ring_edge, reinterpret_cast<double*>(o + o_tab));
  HIPCHECK(hipMemcpyAsync(X.tables.p, o + o_tab, 8 * n_tab, hipMemcpyHostToDevice, st));
  if (mapped) {  // points were dropped: caller index -> position among the finite points
    HIPCHECK(X.finv.reserve(mc));
    int* finv = reinterpret_cast<int*>(o + o_finv);
    for (int i = 0; i < nc; ++i) finv[i] = -1;
    for (int f = 0; f < n; ++f) finv[c.keep[(size_t)f]] = f;
    HIPCHECK(hipMemcpyAsync(X.finv.p, finv, 4 * mc, hipMemcpyHostToDevice, st));
    A.finv = X.finv.p;
  }
  if (mask) {
    HIPCHECK(X.mask.reserve(mc));
    std::memcpy(o + o_mask, mask, (size_t)nc);
    HIPCHECK(hipMemcpyAsync(X.mask.p, o + o_mask, mc, hipMemcpyHostToDevice, st));
    A.mask = X.mask.p;
  }
  HIPCHECK(hipMemsetAsync(X.ctl.p, 0, sizeof ctl, st));
  HIPCHECK(hipMemsetAsync(X.seg.p, 0, 4 * 2 * (size_t)(RS + 1), st));
  HIPCHECK(sicp::launch_ground_keys(A, st));
  if (nc > 0) HIPCHECK(sicp::prim_sort_pairs(X.temp.p, pair_bytes, X.key.p, X.skey.p, X.val.p, X.sval.p, nc, 0, sicp::kGroundSortBits, st));
  HIPCHECK(sicp::launch_ground_segments(A, st));
  HIPCHECK(sicp::launch_ground_fit(A, st));
  HIPCHECK(sicp::launch_ground_points(A, st));
  if (select && nc > 0) {
    HIPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, nc, st));
    HIPCHECK(sicp::launch_ground_select(A, st));
  }
  HIPCHECK(hipMemcpyAsync(o + o_ctl, X.ctl.p, sizeof ctl, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(o + o_cells, X.cells.p, sizeof(sicp::GroundCell) * (size_t)RS, hipMemcpyDeviceToHost, st));
  if (nc > 0 && out) {
    if (out->height) HIPCHECK(hipMemcpyAsync(o + o_height, X.oheight.p, 8 * (size_t)nc, hipMemcpyDeviceToHost, st));
    if (out->cell) HIPCHECK(hipMemcpyAsync(o + o_cell, X.cellv.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, st));
    if (out->ground) HIPCHECK(hipMemcpyAsync(o + o_ground, X.oground.p, (size_t)nc, hipMemcpyDeviceToHost, st));
  }
  HIPCHECK(hipStreamSynchronize(st));
  std::memcpy(&ctl, o + o_ctl, sizeof ctl);
  const sicp::GroundCell* rows = reinterpret_cast<const sicp::GroundCell*>(o + o_cells);
  sicp_ground_info I;
  std::memset(&I, 0, sizeof I);
  I.n_points = nc;
  I.n_finite = n;
  I.n_candidates = ctl.n_candidates;
  I.n_below = ctl.n_below;
  I.n_cells = RS;
  for (int k = 0; k < RS; ++k) {
    I.n_ground += rows[k].n_ground;
    I.cells[rows[k].status] += 1;
  }
  I.n_selected = select ? ctl.n_selected : 0;
  const bool want_table = out && (out->status || out->n_members || out->n_ground || out->n_fit || out->normal || out->centroid ||
                                  out->lambda_min || out->lpr);
  if (want_table && out->capacity < RS) {
    X.idle = true;
    I.n_selected = 0;
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    h->last_error = "sicp_segment_ground: there are " + std::to_string(RS) + " cells, the cell arrays hold " + std::to_string(out->capacity);
    return SICP_ERR_INVALID_ARGUMENT;
  }
  if (select) {
    const int n_sel = ctl.n_selected;
    if (n_sel == 0) {
      X.idle = true;
      h->last_error = "sicp_segment_ground: the selection is empty; dst keeps its cloud";
      return SICP_ERR_TOO_FEW_POINTS;
    }
    // the selected points -> pinned memory: all of them are on the host before dst's slot lets go of its old cloud (filter.cpp)
    const size_t mo = (size_t)n_sel;
    HIPCHECK(h->gr_out.resize(mo * 4));
    uint32_t* q = h->gr_out.data();
    HIPCHECK(hipMemcpyAsync(q, X.gx.p, 4 * mo, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(q + mo, X.gy.p, 4 * mo, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(q + 2 * mo, X.gz.p, 4 * mo, hipMemcpyDeviceToHost, st));
    if (labels) HIPCHECK(hipMemcpyAsync(q + 3 * mo, X.gl.p, 4 * mo, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    X.idle = true;
    const StridedCloud in = {(const char*)q, (const char*)(q + mo), (const char*)(q + 2 * mo), labels ? (const char*)(q + 3 * mo) : nullptr, 4, 4};
    const int rc = set_cloud_common(dst, dst_which, n_sel, in);  // (in place: `c` is the new cloud from here on)
    if (rc != SICP_OK) {
      if (dst != h) h->last_error = "sicp_segment_ground: dst: " + dst->last_error;
      return rc;
    }
  }
  X.idle = true;
  if (out) {
    if (nc > 0) {
      if (out->height) std::memcpy(out->height, o + o_height, 8 * (size_t)nc);
      if (out->cell) std::memcpy(out->cell, o + o_cell, 4 * (size_t)nc);
      if (out->ground) std::memcpy(out->ground, o + o_ground, (size_t)nc);
    }
    for (int k = 0; k < RS && want_table; ++k) {
      const sicp::GroundCell& g = rows[k];
      if (out->status) out->status[k] = (uint8_t)g.status;
      if (out->n_members) out->n_members[k] = g.n_members;
      if (out->n_ground) out->n_ground[k] = g.n_ground;
      if (out->n_fit) out->n_fit[k] = g.n_fit;
      if (out->normal) std::memcpy(out->normal + 3 * k, g.normal, 24);
      if (out->centroid)
        for (int a = 0; a < 3; ++a) out->centroid[3 * k + a] = g.centroid[a] + A.org[a];
      if (out->lambda_min) out->lambda_min[k] = g.lambda_min;
      if (out->lpr) out->lpr[k] = g.lpr;
    }
  }
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
