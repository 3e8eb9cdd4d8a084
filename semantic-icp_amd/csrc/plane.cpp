// plane.cpp -- sicp_segment_planes (include/sicp.h, "planes of a cloud"): argument checks, then every round of
// plane_kernels.hip queued on the handle's stream -- compaction, sampling, the score, the winner, the membership pass, the tree
// sums, the fit and the re-selection, the record -- with no host synchronisation between them: a round's kernels read the
// candidate count and the `done` flag from device memory.  One read-back of the control block, the plane records and the
// per-point states ends the call.  Nothing the handle holds for align() is touched: the call reads the cloud's caller-order
// arrays (valid in every layout) and writes scratch of its own.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

// A call's device scratch: taken from the arena, given back at the end (DevArena::release_scratch: `idle` once the stream
// has been synchronised behind the call's launches).
struct PlaneScratch {
  DevBuf<unsigned char> temp, mask, member;
  DevBuf<int> finv, state, flag, pos, partial, total;
  DevBuf<float> cx, cy, cz;
  DevBuf<double> sum_f, sum_c;
  DevBuf<sicp::PlaneHyp> hyp;
  DevBuf<sicp::PlaneCtl> ctl;
  DevBuf<sicp::PlaneRec> rec;
  int device = -1;
  bool idle = true;
  ~PlaneScratch() {
    DevArena::release_scratch(device, idle, temp, mask, member, finv, state, flag, pos, partial, total, cx, cy, cz, sum_f, sum_c, hyp, ctl, rec);
  }
};

size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

void plane_default_params(sicp_plane_params* p) {
  std::memset(p, 0, sizeof *p);
  p->distance_threshold = 0.2;
  p->min_cos = 0.0;
  p->seed = 1;
  p->num_hypotheses = 1024;
  p->max_planes = 1;
  p->min_inliers = 100;
  p->refine = 1;
  p->n_ignore = 0;
}

int segment_planes(sicp_context* h, int which, const sicp_plane_params* p, const uint8_t* mask, int32_t* plane_id, int32_t capacity,
                   double* coeff, int32_t* count, int32_t* hyp_index, int32_t* hyp_count, double* centroid, double* rms,
                   sicp_plane_info* info) {
  if (!h) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    h->last_error = "sicp_segment_planes: " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  auto too_few = [&](long long have) {
    h->last_error = "sicp_segment_planes: a plane needs 3 candidate points, the cloud has " + std::to_string(have);
    return SICP_ERR_TOO_FEW_POINTS;
  };
  if (!p) return refuse("the params are NULL");
  if (which != SICP_SOURCE && which != SICP_TARGET) return refuse("which is neither SICP_SOURCE nor SICP_TARGET");
  if (!std::isfinite(p->distance_threshold) || !(p->distance_threshold > 0.0)) return refuse("distance_threshold must be finite and > 0");
  bool axis_finite = true, axis_zero = true;
  for (int k = 0; k < 3; ++k) {
    axis_finite = axis_finite && std::isfinite(p->axis[k]);
    axis_zero = axis_zero && p->axis[k] == 0.0;
  }
  if (!axis_finite) return refuse("axis must be finite");
  if (axis_zero && p->min_cos != 0.0) return refuse("min_cos must be 0 without an axis");
  if (!axis_zero && !(p->min_cos > 0.0 && p->min_cos <= 1.0)) return refuse("min_cos must be in (0, 1] with an axis");
  if (p->num_hypotheses < 1 || p->num_hypotheses > SICP_PLANE_MAX_HYPOTHESES)
    return refuse("num_hypotheses must be in 1 .. " + std::to_string(SICP_PLANE_MAX_HYPOTHESES));
  if (p->max_planes < 1 || p->max_planes > SICP_PLANE_MAX_PLANES) return refuse("max_planes must be in 1 .. " + std::to_string(SICP_PLANE_MAX_PLANES));
  if (p->min_inliers < 3) return refuse("min_inliers must be >= 3");
  if (p->refine != 0 && p->refine != 1) return refuse("refine must be 0 or 1");
  if (p->n_ignore < 0 || p->n_ignore > SICP_PLANE_MAX_IGNORE) return refuse("n_ignore must be in 0 .. " + std::to_string(SICP_PLANE_MAX_IGNORE));
  if (capacity < 0) return refuse("capacity must be >= 0");
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    h->last_error = "sicp_segment_planes: the slot holds no cloud";
    return SICP_ERR_NOT_READY;
  }
  if (!c.has_label && p->n_ignore != 0) return refuse("the cloud was set without labels: only an empty ignore list can segment it");
  const double t_begin = now_ms();
  SICPCHECK(set_device(h));
  // the cloud's device copy: the finite points in caller order (Cloud::rx ..., valid in every layout), prepared as a merge part is
  if (c.layout < 0) SICPCHECK(prepare_cloud(h, c));
  SICPCHECK(cloud_wait(h, c));
  const int n = c.n, nc = c.n_caller;
  if (n < 3) return too_few(n);
  const bool labels = c.has_label, mapped = !c.keep.empty();
  const bool has_axis = !axis_zero;
  const int H = p->num_hypotheses;
  hipStream_t st = h->stream;
  PlaneScratch X;
  sicp::PlaneArgs A;
  std::memset(&A, 0, sizeof A);
  sicp::PlaneCtl ctl;
  // pinned: finite positions | mask on their way up; the control block | the records | the states on their way back
  const size_t mc = (size_t)nc, m = (size_t)n;
  const size_t o_finv = 0, o_mask = o_finv + up8(mapped ? 4 * mc : 0), o_ctl = o_mask + up8(mask ? mc : 0), o_rec = o_ctl + up8(sizeof ctl),
               o_state = o_rec + sizeof(sicp::PlaneRec) * sicp::kPlaneMaxPlanes, o_end = o_state + up8(4 * mc);
  HIPCHECK(h->pl_stage.resize(o_end));
  unsigned char* o = h->pl_stage.data();
  X.device = h->device;
  X.idle = false;
  const size_t tree = sicp::plane_tree_doubles(nc);
  HIPCHECK(X.state.reserve(mc)); HIPCHECK(X.flag.reserve(mc)); HIPCHECK(X.pos.reserve(mc)); HIPCHECK(X.member.reserve(mc));
  HIPCHECK(X.cx.reserve(m)); HIPCHECK(X.cy.reserve(m)); HIPCHECK(X.cz.reserve(m));
  HIPCHECK(X.hyp.reserve((size_t)H)); HIPCHECK(X.total.reserve((size_t)H));
  HIPCHECK(X.partial.reserve((size_t)sicp::plane_tiles(n) * (size_t)H));
  HIPCHECK(X.sum_f.reserve(tree)); HIPCHECK(X.sum_c.reserve(tree));
  HIPCHECK(X.ctl.reserve(1)); HIPCHECK(X.rec.reserve(sicp::kPlaneMaxPlanes));
  size_t scan_bytes = 0;
  HIPCHECK(sicp::prim_scan_int(nullptr, scan_bytes, X.flag.p, X.pos.p, nc, st));
  HIPCHECK(X.temp.reserve(scan_bytes + 256));

  A.n = n; A.n_caller = nc;
  A.labels = labels ? 1 : 0;
  A.H = H; A.min_inliers = p->min_inliers; A.refine = p->refine;
  A.n_ignore = p->n_ignore;
  for (int k = 0; k < p->n_ignore; ++k) A.ignore[k] = p->ignore[k];
  A.has_axis = has_axis ? 1 : 0;
  A.tt = p->distance_threshold * p->distance_threshold;
  if (has_axis) {
    for (int k = 0; k < 3; ++k) A.axis[k] = p->axis[k];
    A.mc2 = p->min_cos * p->min_cos;
    A.aa = (p->axis[0] * p->axis[0] + p->axis[1] * p->axis[1]) + p->axis[2] * p->axis[2];
  }
  A.seed = p->seed;
  A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
  A.label = labels ? c.rl.p : nullptr;
  A.state = X.state.p; A.flag = X.flag.p; A.pos = X.pos.p; A.member = X.member.p;
  A.cx = X.cx.p; A.cy = X.cy.p; A.cz = X.cz.p;
  A.hyp = X.hyp.p; A.partial = X.partial.p; A.total = X.total.p;
  A.sum_f = X.sum_f.p; A.sum_c = X.sum_c.p;
  A.ctl = X.ctl.p; A.rec = X.rec.p;
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
    std::memcpy(o + o_mask, mask, mc);
    HIPCHECK(hipMemcpyAsync(X.mask.p, o + o_mask, mc, hipMemcpyHostToDevice, st));
    A.mask = X.mask.p;
  }
  HIPCHECK(hipMemsetAsync(X.ctl.p, 0, sizeof ctl, st));
  HIPCHECK(hipMemsetAsync(X.rec.p, 0, sizeof(sicp::PlaneRec) * sicp::kPlaneMaxPlanes, st));
  HIPCHECK(sicp::launch_plane_init(A, st));
  for (int r = 0; r < p->max_planes; ++r) {
    HIPCHECK(sicp::launch_plane_flags(A, st));
    HIPCHECK(sicp::prim_scan_int(X.temp.p, scan_bytes, X.flag.p, X.pos.p, nc, st));
    HIPCHECK(sicp::launch_plane_compact(A, st));
    HIPCHECK(sicp::launch_plane_sample(A, r, st));
    HIPCHECK(sicp::launch_plane_score(A, st));
    HIPCHECK(sicp::launch_plane_winner(A, r, st));
    HIPCHECK(sicp::launch_plane_members(A, st));
    if (p->refine) {
      HIPCHECK(sicp::launch_plane_tree_sums(A, 0, st));
      HIPCHECK(sicp::launch_plane_tree_sums(A, 1, st));
      HIPCHECK(sicp::launch_plane_fit(A, r, st));
      HIPCHECK(sicp::launch_plane_members(A, st));
    }
    HIPCHECK(sicp::launch_plane_tree_sums(A, 0, st));
    HIPCHECK(sicp::launch_plane_record(A, r, st));
    HIPCHECK(sicp::launch_plane_assign(A, r, st));
  }
  HIPCHECK(hipMemcpyAsync(o + o_ctl, X.ctl.p, sizeof ctl, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(o + o_rec, X.rec.p, sizeof(sicp::PlaneRec) * sicp::kPlaneMaxPlanes, hipMemcpyDeviceToHost, st));
  if (plane_id) HIPCHECK(hipMemcpyAsync(o + o_state, X.state.p, 4 * mc, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  X.idle = true;
  std::memcpy(&ctl, o + o_ctl, sizeof ctl);
  if (ctl.n_candidates < 3) return too_few(ctl.n_candidates);
  const int np = ctl.n_planes;
  sicp_plane_info I;
  std::memset(&I, 0, sizeof I);
  I.n_points = nc;
  I.n_finite = n;
  I.n_candidates = ctl.n_candidates;
  I.n_assigned = ctl.n_assigned;
  I.n_planes = np;
  I.rounds = ctl.rounds;
  I.n_invalid_hypotheses = ctl.n_invalid;
  const bool want_table = coeff || count || hyp_index || hyp_count || centroid || rms;
  if (want_table && capacity < np) {
    I.t_total_ms = now_ms() - t_begin;
    if (info) *info = I;
    h->last_error = "sicp_segment_planes: there are " + std::to_string(np) + " planes, the table arrays hold " + std::to_string(capacity);
    return SICP_ERR_INVALID_ARGUMENT;
  }
  if (plane_id) {
    const int32_t* s = reinterpret_cast<const int32_t*>(o + o_state);
    for (int i = 0; i < nc; ++i) plane_id[i] = s[i] < 0 ? -1 : s[i];
  }
  const sicp::PlaneRec* R = reinterpret_cast<const sicp::PlaneRec*>(o + o_rec);
  for (int k = 0; k < np; ++k) {
    if (coeff) std::memcpy(coeff + 4 * k, R[k].coeff, 32);
    if (count) count[k] = R[k].count;
    if (hyp_index) hyp_index[k] = R[k].hyp_index;
    if (hyp_count) hyp_count[k] = R[k].hyp_count;
    if (centroid) std::memcpy(centroid + 3 * k, R[k].centroid, 24);
    if (rms) rms[k] = R[k].rms;
  }
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
