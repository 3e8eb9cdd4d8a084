// deskew.cpp -- sicp_deskew (include/sicp.h, "deskewing a scan"): the argument checks, the relative knots K_k = ref^-1 T_k
// composed once in double with se3.hpp, the times and the table on their way up through the call's scratch, the one launch of
// deskew_kernels.hip on the cloud's device copy, one read-back, and, with dst, the moved cloud staged into dst's slot through the
// path of sicp_set_cloud.  Without dst nothing the handle holds for align() is touched.  sicp_deskew_twist_knots is host only.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

struct DeskewScratch {
  DevBuf<double> times, knot_time, knot_qt;
  DevBuf<int> caller, res;
  DevBuf<float> ox, oy, oz;
  int device = -1;
  bool idle = true;
  ~DeskewScratch() { DevArena::release_scratch(device, idle, times, knot_time, knot_qt, caller, res, ox, oy, oz); }
};

bool slot_ok(int which) { return which == SICP_SOURCE || which == SICP_TARGET; }
size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

// the pose graph's rule: finite, | |q| - 1 | <= 1e-6; "" when the pose is accepted
std::string bad_pose(const double* q) {
  for (int d = 0; d < 7; ++d)
    if (!std::isfinite(q[d])) return "is not finite";
  const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!(std::fabs(norm - 1.0) <= 1e-6)) return "has a quaternion of norm " + std::to_string(norm);
  return "";
}
void normalised(const double* q, double* o) {
  const double inv = 1.0 / std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int d = 0; d < 4; ++d) o[d] = q[d] * inv;
  for (int d = 4; d < 7; ++d) o[d] = q[d];
}

}  // namespace

int deskew(sicp_context* h, int which, const double* times, int32_t n_knots, const double* knot_time, const double* knot_qt,
           const double* ref_qt, sicp_context* dst, int dst_which, float* ox, float* oy, float* oz, double* knots_out,
           sicp_deskew_info* info) {
  if (!h) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    h->last_error = "sicp_deskew: " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!times) return refuse("times is NULL");
  if (!knot_time || !knot_qt) return refuse("the knots are NULL");
  if (!slot_ok(which)) return refuse("which is neither SICP_SOURCE nor SICP_TARGET");
  if (dst && !slot_ok(dst_which)) return refuse("dst_which is neither SICP_SOURCE nor SICP_TARGET");
  if (n_knots < 2 || n_knots > SICP_DESKEW_MAX_KNOTS) return refuse("n_knots must be in 2 .. " + std::to_string(SICP_DESKEW_MAX_KNOTS));
  for (int k = 0; k < n_knots; ++k) {
    if (!std::isfinite(knot_time[k])) return refuse("knot time " + std::to_string(k) + " is not finite");
    if (k > 0 && !(knot_time[k] > knot_time[k - 1])) return refuse("knot time " + std::to_string(k) + " does not ascend");
  }
  for (int k = 0; k < n_knots; ++k) {
    const std::string why = bad_pose(knot_qt + 7 * (size_t)k);
    if (!why.empty()) return refuse("knot pose " + std::to_string(k) + " " + why);
  }
  if (ref_qt) {
    const std::string why = bad_pose(ref_qt);
    if (!why.empty()) return refuse("ref_qt " + why);
  }
  if (dst && dst->device != h->device) return refuse("dst is on device " + std::to_string(dst->device) + ", the handle on " + std::to_string(h->device));
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    h->last_error = "sicp_deskew: the slot holds no cloud";
    return SICP_ERR_NOT_READY;
  }
  if (dst && c.has_label && c.hl.size() < (size_t)c.n) {
    h->last_error = "sicp_deskew: the cloud has no host copy of its labels";
    return SICP_ERR_NOT_READY;
  }
  const double t_begin = now_ms();
  const int n = c.n, nc = c.n_caller, nk = n_knots;
  const bool labels = c.has_label, mapped = !c.keep.empty();

  // rule 2: K_k = ref^-1 T_k, consecutive quaternions in one hemisphere
  std::vector<double> K(7 * (size_t)nk);
  {
    double ref[7], inv[7], T[7];
    normalised(ref_qt ? ref_qt : knot_qt + 7 * (size_t)(nk - 1), ref);
    sicp::se3::inverse(ref, inv);
    for (int k = 0; k < nk; ++k) {
      double* o = &K[7 * (size_t)k];
      normalised(knot_qt + 7 * (size_t)k, T);
      sicp::se3::mul(inv, T, o);
      if (k > 0) {
        const double* p = o - 7;
        if (o[0] * p[0] + o[1] * p[1] + o[2] * p[2] + o[3] * p[3] < 0.0)
          for (int d = 0; d < 4; ++d) o[d] = -o[d];
      }
    }
  }

  SICPCHECK(set_device(h));
  // the cloud's device copy (a cloud not yet indexed is prepared as the handle's next call would)
  if (c.layout < 0) SICPCHECK(prepare_cloud(h, c));
  SICPCHECK(cloud_wait(h, c));
  hipStream_t st = h->stream;
  DeskewScratch X;
  int res[kDkRes] = {0, 0, 0, 0};
  const size_t mc = (size_t)std::max(nc, 1), m = (size_t)std::max(n, 1);
  // pinned, on their way up: times | knot times | knot poses | caller indices; on their way back: the counts
  const size_t o_times = 0, o_kt = o_times + 8 * mc, o_kq = o_kt + 8 * (size_t)nk, o_caller = o_kq + 56 * (size_t)nk,
               o_res = o_caller + up8(mapped ? 4 * m : 0), o_end = o_res + sizeof res;
  HIPCHECK(h->dk_stage.resize(o_end));
  unsigned char* o = h->dk_stage.data();
  // pinned, on their way back, to the caller and into dst: x | y | z | label, the caller's indices
  HIPCHECK(h->dk_out.resize(mc * (dst && labels ? 4 : 3)));
  uint32_t* q = h->dk_out.data();
  if (n > 0) {
    X.device = h->device;
    X.idle = false;
    HIPCHECK(X.times.reserve(mc)); HIPCHECK(X.knot_time.reserve((size_t)nk)); HIPCHECK(X.knot_qt.reserve(7 * (size_t)nk));
    HIPCHECK(X.ox.reserve(mc)); HIPCHECK(X.oy.reserve(mc)); HIPCHECK(X.oz.reserve(mc));
    HIPCHECK(X.res.reserve(kDkRes));
    std::memcpy(o + o_times, times, 8 * (size_t)nc);
    std::memcpy(o + o_kt, knot_time, 8 * (size_t)nk);
    std::memcpy(o + o_kq, K.data(), 56 * (size_t)nk);
    HIPCHECK(hipMemcpyAsync(X.times.p, o + o_times, 8 * (size_t)nc, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(X.knot_time.p, o + o_kt, 8 * (size_t)nk, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(X.knot_qt.p, o + o_kq, 56 * (size_t)nk, hipMemcpyHostToDevice, st));
    sicp::DeskewArgs A;
    std::memset(&A, 0, sizeof A);
    A.n = n; A.n_knots = nk;
    A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
    A.times = X.times.p; A.knot_time = X.knot_time.p; A.knot_qt = X.knot_qt.p;
    A.ox = X.ox.p; A.oy = X.oy.p; A.oz = X.oz.p;
    A.res = X.res.p;
    if (mapped) {  // points were dropped: finite index -> caller index
      HIPCHECK(X.caller.reserve(m));
      std::memcpy(o + o_caller, c.keep.data(), 4 * (size_t)n);
      HIPCHECK(hipMemcpyAsync(X.caller.p, o + o_caller, 4 * (size_t)n, hipMemcpyHostToDevice, st));
      A.caller = X.caller.p;
    }
    HIPCHECK(hipMemsetAsync(X.res.p, 0, sizeof res, st));
    HIPCHECK(sicp::launch_deskew(A, st));
    HIPCHECK(hipMemcpyAsync(o + o_res, X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(q, X.ox.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(q + mc, X.oy.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(q + 2 * mc, X.oz.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    X.idle = true;
    std::memcpy(res, o + o_res, sizeof res);
  }
  // rule 4: a point that is not finite keeps its three floats
  for (size_t k = 0; k < c.drop_i.size(); ++k) {
    const size_t i = (size_t)c.drop_i[k];
    std::memcpy(q + i, &c.drop_xyz[3 * k], 4);
    std::memcpy(q + mc + i, &c.drop_xyz[3 * k + 1], 4);
    std::memcpy(q + 2 * mc + i, &c.drop_xyz[3 * k + 2], 4);
  }
  if (dst && res[kDkMoved] == 0) {
    h->last_error = "sicp_deskew: no finite point remains; dst keeps its cloud";
    return SICP_ERR_TOO_FEW_POINTS;
  }
  sicp_deskew_info I;
  std::memset(&I, 0, sizeof I);
  I.n_points = nc;
  I.n_finite = n;
  I.n_moved = res[kDkMoved];
  I.n_bad_time = res[kDkBadTime];
  I.n_clamped_lo = res[kDkClampedLo];
  I.n_clamped_hi = res[kDkClampedHi];
  int rc = SICP_OK;
  if (dst) {  // (in place: `c` is the new cloud from here on)
    // everything is on the host before dst's slot lets go of its old cloud (filter.cpp); the labels of the finite points at
    // the caller's indices -- a point outside the index has none to keep (sicp_set_cloud drops it with its label)
    if (labels) {
      uint32_t* ql = q + 3 * mc;
      std::memset(ql, 0, 4 * mc);
      for (int f = 0; f < n; ++f) ql[mapped ? c.keep[f] : f] = c.hl[f];
    }
    const StridedCloud in = {(const char*)q, (const char*)(q + mc), (const char*)(q + 2 * mc), labels ? (const char*)(q + 3 * mc) : nullptr, 4, 4};
    rc = set_cloud_common(dst, dst_which, nc, in);
    if (rc != SICP_OK && dst != h) h->last_error = "sicp_deskew: dst: " + dst->last_error;
  }
  if (rc != SICP_OK) return rc;
  if (nc > 0) {
    if (ox) std::memcpy(ox, q, 4 * (size_t)nc);
    if (oy) std::memcpy(oy, q + mc, 4 * (size_t)nc);
    if (oz) std::memcpy(oz, q + 2 * mc, 4 * (size_t)nc);
  }
  if (knots_out) std::memcpy(knots_out, K.data(), 56 * (size_t)nk);
  if (info) {
    I.t_total_ms = now_ms() - t_begin;
    *info = I;
  }
  return SICP_OK;
}

int deskew_twist_knots(const double* delta_qt, double t0, double t1, int32_t n_knots, double* knot_time, double* knot_qt) {
  if (!delta_qt || !knot_time || !knot_qt) return SICP_ERR_INVALID_ARGUMENT;
  if (!bad_pose(delta_qt).empty()) return SICP_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(t0) || !std::isfinite(t1) || !(t1 > t0)) return SICP_ERR_INVALID_ARGUMENT;
  if (n_knots < 2 || n_knots > SICP_DESKEW_MAX_KNOTS) return SICP_ERR_INVALID_ARGUMENT;
  double d[7], xi[6];
  normalised(delta_qt, d);
  sicp::se3::log(d, xi);
  for (int k = 0; k < n_knots; ++k) {
    const double s = (double)k / (double)(n_knots - 1);
    double a[6];
    for (int j = 0; j < 6; ++j) a[j] = s * xi[j];
    sicp::se3::exp(a, knot_qt + 7 * (size_t)k);
    knot_time[k] = t0 + s * (t1 - t0);
  }
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
