// range.cpp -- sicp_range_image / sicp_range_labels / sicp_range_tables (include/sicp.h, "range image and labels from it"): the
// argument checks, the column table and the row edges formed once in double with libm, their way up with the caller map and the
// network's classes through the call's scratch, the launches of range_kernels.hip on the cloud's device copy, one read-back,
// and, with dst, the relabelled cloud staged into dst's slot through the path of sicp_set_cloud.  Without dst nothing the handle
// holds for align() is touched.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

struct RangeScratch {
  DevBuf<double> tables;
  DevBuf<int> caller, pix, res, o_index, o_pixel;
  DevBuf<unsigned long long> key;
  DevBuf<uint32_t> count, pixel_label, o_label, o_out_label;
  DevBuf<float4> rec;
  DevBuf<float> o_r2, o_x, o_y, o_z;
  DevBuf<uint8_t> o_visible, o_votes;
  int device = -1;
  bool idle = true;
  ~RangeScratch() {
    DevArena::release_scratch(device, idle, tables, caller, pix, res, o_index, o_pixel, key, count, pixel_label, o_label, o_out_label, rec,
                              o_r2, o_x, o_y, o_z, o_visible, o_votes);
  }
};

bool slot_ok(int which) { return which == SICP_SOURCE || which == SICP_TARGET; }
size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }
constexpr double kHalfPi = 1.57079632679489661923;

// the parameter checks of rule 14; "" when the parameters are accepted
std::string bad_params(const sicp_range_params& p) {
  if (p.width < 16 || p.width > SICP_RANGE_MAX_WIDTH || p.width % 2 != 0)
    return "width must be even and in 16 .. " + std::to_string(SICP_RANGE_MAX_WIDTH);
  if (p.height < 1 || p.height > SICP_RANGE_MAX_HEIGHT) return "height must be in 1 .. " + std::to_string(SICP_RANGE_MAX_HEIGHT);
  if (!std::isfinite(p.fov_up) || !std::isfinite(p.fov_down)) return "the field of view is not finite";
  if (!(p.fov_up > p.fov_down)) return "fov_up must be above fov_down";
  if (!(p.fov_up < kHalfPi) || !(p.fov_down > -kHalfPi)) return "fov_up and fov_down must lie strictly inside +-pi/2";
  if (!std::isfinite(p.min_range) || p.min_range < 0.0) return "min_range must be finite and >= 0";
  if (!std::isfinite(p.max_range) || !(p.max_range > p.min_range)) return "max_range must be finite and above min_range";
  if (!std::isfinite(p.max_range * p.max_range)) return "max_range squared is not finite";
  if (p.clockwise != 0 && p.clockwise != 1) return "clockwise must be 0 or 1";
  if (p.col_shift < 0 || p.col_shift >= p.width) return "col_shift must be in 0 .. width - 1";
  if (p.window < 1 || p.window > SICP_RANGE_MAX_WINDOW || p.window % 2 == 0)
    return "window must be odd and in 1 .. " + std::to_string(SICP_RANGE_MAX_WINDOW);
  if (p.k < 1 || p.k > SICP_RANGE_MAX_K) return "k must be in 1 .. " + std::to_string(SICP_RANGE_MAX_K);
  if (!(p.max_dist_sq >= 0.0)) return "max_dist_sq must be >= 0";
  return "";
}

// the tables as the kernels read them: row_edge [H + 1] | cos_half [W / 2] | sin_half [W / 2]; "" when they are accepted
std::string make_tables(const sicp_range_params& p, const double* beam, std::vector<double>& t) {
  const int W = p.width, H = p.height, half = W / 2;
  t.assign((size_t)(H + 1 + W), 0.0);
  std::vector<double> a((size_t)H + 1);
  if (beam && H > 1) {
    for (int r = 0; r < H; ++r) {
      if (!std::isfinite(beam[r])) return "beam_elevation[" + std::to_string(r) + "] is not finite";
      if (r > 0 && !(beam[r] < beam[r - 1])) return "beam_elevation[" + std::to_string(r) + "] does not descend";
    }
    a[0] = beam[0] + (beam[0] - beam[1]) / 2.0;
    for (int r = 1; r < H; ++r) a[r] = (beam[r - 1] + beam[r]) / 2.0;
    a[H] = beam[H - 1] - (beam[H - 2] - beam[H - 1]) / 2.0;
  } else {
    if (beam && !std::isfinite(beam[0])) return "beam_elevation[0] is not finite";
    for (int r = 0; r <= H; ++r) a[r] = p.fov_up + (p.fov_down - p.fov_up) * ((double)r / (double)H);
    a[H] = p.fov_down;
  }
  for (int r = 0; r <= H; ++r) {
    if (!(a[r] < kHalfPi) || !(a[r] > -kHalfPi)) return "row edge " + std::to_string(r) + " does not lie strictly inside +-pi/2";
    const double tg = std::tan(a[r]);
    t[r] = tg * std::fabs(tg);
    if (!std::isfinite(t[r])) return "row edge " + std::to_string(r) + " is not finite";
    if (r > 0 && !(t[r] < t[r - 1])) return "row edge " + std::to_string(r) + " does not descend";
  }
  const double two_pi = 2.0 * 3.14159265358979323846;
  for (int j = 0; j < half; ++j) {
    const double ang = two_pi * (double)j / (double)W;
    t[(size_t)(H + 1 + j)] = std::cos(ang);
    t[(size_t)(H + 1 + half + j)] = std::sin(ang);
  }
  return "";
}

struct Copy { void* host; const void* dev; size_t bytes, at; };

// both entry points: vote = the call is sicp_range_labels
int range_call(sicp_context* h, const char* name, bool vote, int which, const sicp_range_params* p, const double* beam, const float* origin,
               const uint32_t* pixel_label, sicp_context* dst, int dst_which, int32_t* index, float* range_sq, float* x, float* y, float* z,
               uint32_t* label, uint32_t* count, int32_t* pixel, uint8_t* visible, uint32_t* out_label, uint8_t* votes,
               sicp_range_info* info) {
  if (!h) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    h->last_error = std::string(name) + ": " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!p) return refuse("params is NULL");
  if (!slot_ok(which)) return refuse("which is neither SICP_SOURCE nor SICP_TARGET");
  if (dst && !slot_ok(dst_which)) return refuse("dst_which is neither SICP_SOURCE nor SICP_TARGET");
  {
    const std::string why = bad_params(*p);
    if (!why.empty()) return refuse(why);
  }
  if (vote && !pixel_label) return refuse("pixel_label is NULL");
  float o3[3] = {0.f, 0.f, 0.f};
  if (origin)
    for (int d = 0; d < 3; ++d) {
      if (!std::isfinite(origin[d])) return refuse("sensor_origin is not finite");
      o3[d] = origin[d];
    }
  std::vector<double> tables;
  {
    const std::string why = make_tables(*p, beam, tables);
    if (!why.empty()) return refuse(why);
  }
  if (dst && dst->device != h->device) return refuse("dst is on device " + std::to_string(dst->device) + ", the handle on " + std::to_string(h->device));
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    h->last_error = std::string(name) + ": the slot holds no cloud";
    return SICP_ERR_NOT_READY;
  }
  if (c.has_label && c.hl.size() < (size_t)c.n) {
    h->last_error = std::string(name) + ": the cloud has no host copy of its labels";
    return SICP_ERR_NOT_READY;
  }
  const double t_begin = now_ms();
  const int n = c.n, nc = c.n_caller, W = p->width, H = p->height;
  const size_t np = (size_t)W * (size_t)H;
  const bool labels = c.has_label, mapped = !c.keep.empty();
  if (dst && n == 0) {
    h->last_error = std::string(name) + ": no finite point remains; dst keeps its cloud";
    return SICP_ERR_TOO_FEW_POINTS;
  }

  SICPCHECK(set_device(h));
  // the cloud's device copy (a cloud not yet indexed is prepared as the handle's next call would)
  if (c.layout < 0) SICPCHECK(prepare_cloud(h, c));
  SICPCHECK(cloud_wait(h, c));
  hipStream_t st = h->stream;
  RangeScratch X;
  X.device = h->device;
  X.idle = false;
  const size_t mc = (size_t)std::max(nc, 1), m = (size_t)std::max(n, 1);
  int res[kRgRes] = {0, 0, 0, 0};

  sicp::RangeArgs A;
  std::memset(&A, 0, sizeof A);
  A.n = n; A.n_caller = nc; A.W = W; A.H = H;
  A.clockwise = p->clockwise; A.col_shift = p->col_shift; A.window = p->window; A.k = p->k;
  A.ox = o3[0]; A.oy = o3[1]; A.oz = o3[2];
  A.min_sq = p->min_range * p->min_range; A.max_sq = p->max_range * p->max_range;
  A.max_dist_sq = p->max_dist_sq;
  A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
  A.label = labels ? c.rl.p : nullptr;

  // what comes back, each part at an 8-byte boundary of the pinned stage, after what goes up: tables | caller map | classes
  std::vector<Copy> back;
  const size_t o_tab = 0, o_caller = o_tab + 8 * tables.size(), o_pl = o_caller + up8(mapped ? 4 * m : 0),
               o_res = o_pl + up8(vote ? 4 * np : 0);
  size_t o_end = o_res + up8(sizeof res);
  auto want = [&](void* host, const void* dev, size_t bytes) {
    back.push_back(Copy{host, dev, bytes, o_end});
    o_end += up8(bytes);
  };
  HIPCHECK(X.tables.reserve(tables.size())); HIPCHECK(X.key.reserve(np)); HIPCHECK(X.count.reserve(np)); HIPCHECK(X.rec.reserve(np));
  HIPCHECK(X.pix.reserve(m)); HIPCHECK(X.res.reserve(kRgRes));
  A.tables = X.tables.p; A.key = X.key.p; A.count = X.count.p; A.rec = X.rec.p; A.pix = X.pix.p; A.res = X.res.p;
  if (mapped) { HIPCHECK(X.caller.reserve(m)); A.caller = X.caller.p; }
  if (vote) {
    HIPCHECK(X.pixel_label.reserve(np)); A.pixel_label = X.pixel_label.p;
    if (out_label || dst) { HIPCHECK(X.o_out_label.reserve(mc)); A.o_out_label = X.o_out_label.p; }
    if (votes) { HIPCHECK(X.o_votes.reserve(mc)); A.o_votes = X.o_votes.p; }
  } else {
    if (index) { HIPCHECK(X.o_index.reserve(np)); A.o_index = X.o_index.p; want(index, A.o_index, 4 * np); }
    if (range_sq) { HIPCHECK(X.o_r2.reserve(np)); A.o_range_sq = X.o_r2.p; want(range_sq, A.o_range_sq, 4 * np); }
    if (x) { HIPCHECK(X.o_x.reserve(np)); A.o_x = X.o_x.p; want(x, A.o_x, 4 * np); }
    if (y) { HIPCHECK(X.o_y.reserve(np)); A.o_y = X.o_y.p; want(y, A.o_y, 4 * np); }
    if (z) { HIPCHECK(X.o_z.reserve(np)); A.o_z = X.o_z.p; want(z, A.o_z, 4 * np); }
    if (label) { HIPCHECK(X.o_label.reserve(np)); A.o_label = X.o_label.p; want(label, A.o_label, 4 * np); }
    if (count) want(count, A.count, 4 * np);
    if (pixel) { HIPCHECK(X.o_pixel.reserve(mc)); A.o_pixel = X.o_pixel.p; }
    if (visible) { HIPCHECK(X.o_visible.reserve(mc)); A.o_visible = X.o_visible.p; }
  }
  if (nc > 0) {
    if (A.o_pixel) want(pixel, A.o_pixel, 4 * (size_t)nc);
    if (A.o_visible) want(visible, A.o_visible, (size_t)nc);
    if (A.o_out_label) want(out_label, A.o_out_label, 4 * (size_t)nc);  // (host NULL with dst alone: it stays in the stage)
    if (A.o_votes) want(votes, A.o_votes, (size_t)nc);
  }
  // with dst: x | y | z of every point the caller handed over, behind everything else (the labels are out_label's part)
  const size_t o_xyz = o_end;
  if (dst) o_end += 3 * 4 * mc;
  HIPCHECK(h->rg_stage.resize(o_end));
  unsigned char* o = h->rg_stage.data();

  std::memcpy(o + o_tab, tables.data(), 8 * tables.size());
  HIPCHECK(hipMemcpyAsync(X.tables.p, o + o_tab, 8 * tables.size(), hipMemcpyHostToDevice, st));
  if (mapped) {  // points were dropped: finite index -> caller index
    std::memcpy(o + o_caller, c.keep.data(), 4 * (size_t)n);
    HIPCHECK(hipMemcpyAsync(X.caller.p, o + o_caller, 4 * (size_t)n, hipMemcpyHostToDevice, st));
  }
  if (vote) {
    std::memcpy(o + o_pl, pixel_label, 4 * np);
    HIPCHECK(hipMemcpyAsync(X.pixel_label.p, o + o_pl, 4 * np, hipMemcpyHostToDevice, st));
  }
  HIPCHECK(hipMemsetAsync(X.key.p, 0xff, 8 * np, st));
  HIPCHECK(hipMemsetAsync(X.count.p, 0, 4 * np, st));
  HIPCHECK(hipMemsetAsync(X.res.p, 0, sizeof res, st));
  // the entries of the points that are not finite
  if (A.o_pixel) HIPCHECK(hipMemsetAsync(A.o_pixel, 0xff, 4 * mc, st));
  if (A.o_visible) HIPCHECK(hipMemsetAsync(A.o_visible, 0, mc, st));
  if (A.o_out_label) HIPCHECK(hipMemsetAsync(A.o_out_label, 0, 4 * mc, st));
  if (A.o_votes) HIPCHECK(hipMemsetAsync(A.o_votes, 0, mc, st));
  HIPCHECK(sicp::launch_range_project(A, st));
  HIPCHECK(sicp::launch_range_resolve(A, st));
  if (vote) HIPCHECK(sicp::launch_range_vote(A, st));
  else if (A.o_visible) HIPCHECK(sicp::launch_range_visible(A, st));
  HIPCHECK(hipMemcpyAsync(o + o_res, X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
  for (const Copy& k : back) HIPCHECK(hipMemcpyAsync(o + k.at, k.dev, k.bytes, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  X.idle = true;
  std::memcpy(res, o + o_res, sizeof res);

  sicp_range_info I;
  std::memset(&I, 0, sizeof I);
  I.n_points = nc;
  I.n_finite = n;
  I.n_kept = res[kRgKept];
  I.n_out_of_range = n - res[kRgKept];
  I.n_outside_fov = res[kRgOutsideFov];
  I.n_pixels_hit = res[kRgPixelsHit];
  if (vote) {
    I.n_voted = res[kRgVoted];
    I.n_unvoted = nc - res[kRgVoted];
  }
  int rc = SICP_OK;
  if (dst) {  // (in place: `c` is the new cloud from here on)
    // everything is on the host before dst's slot lets go of its old cloud (deskew.cpp): the finite points from the cloud's
    // staging copy, the others as they were handed over, the new labels at the caller's indices
    float* q = reinterpret_cast<float*>(o + o_xyz);
    for (int f = 0; f < n; ++f) {
      const size_t i = (size_t)(mapped ? c.keep[f] : f);
      q[i] = c.hx[f]; q[mc + i] = c.hy[f]; q[2 * mc + i] = c.hz[f];
    }
    for (size_t k = 0; k < c.drop_i.size(); ++k) {
      const size_t i = (size_t)c.drop_i[k];
      q[i] = c.drop_xyz[3 * k]; q[mc + i] = c.drop_xyz[3 * k + 1]; q[2 * mc + i] = c.drop_xyz[3 * k + 2];
    }
    const unsigned char* ql = nullptr;
    for (const Copy& k : back)
      if (k.dev == A.o_out_label) ql = o + k.at;
    const StridedCloud in = {(const char*)q, (const char*)(q + mc), (const char*)(q + 2 * mc), (const char*)ql, 4, 4};
    rc = set_cloud_common(dst, dst_which, nc, in);
    if (rc != SICP_OK && dst != h) h->last_error = std::string(name) + ": dst: " + dst->last_error;
  }
  if (rc != SICP_OK) return rc;
  for (const Copy& k : back)
    if (k.host) std::memcpy(k.host, o + k.at, k.bytes);
  if (info) {
    I.t_total_ms = now_ms() - t_begin;
    *info = I;
  }
  return SICP_OK;
}

}  // namespace

void range_default_params(sicp_range_params* p) {
  std::memset(p, 0, sizeof *p);
  p->width = 2048;
  p->height = 64;
  p->fov_up = 3.0 * 3.14159265358979323846 / 180.0;
  p->fov_down = -25.0 * 3.14159265358979323846 / 180.0;
  p->min_range = 0.5;
  p->max_range = 120.0;
  p->clockwise = 1;
  p->col_shift = 1024;
  p->window = 5;
  p->k = 5;
  p->max_dist_sq = 1.0;
}

int range_tables(const sicp_range_params* p, const double* beam, double* cos_half, double* sin_half, double* row_edge) {
  if (!p || !bad_params(*p).empty()) return SICP_ERR_INVALID_ARGUMENT;
  std::vector<double> t;
  if (!make_tables(*p, beam, t).empty()) return SICP_ERR_INVALID_ARGUMENT;
  const size_t H = (size_t)p->height, half = (size_t)p->width / 2;
  if (row_edge) std::memcpy(row_edge, t.data(), 8 * (H + 1));
  if (cos_half) std::memcpy(cos_half, t.data() + H + 1, 8 * half);
  if (sin_half) std::memcpy(sin_half, t.data() + H + 1 + half, 8 * half);
  return SICP_OK;
}

int range_image(sicp_context* h, int which, const sicp_range_params* p, const double* beam, const float* origin, int32_t* index,
                float* range_sq, float* x, float* y, float* z, uint32_t* label, uint32_t* count, int32_t* pixel, uint8_t* visible,
                sicp_range_info* info) {
  return range_call(h, "sicp_range_image", false, which, p, beam, origin, nullptr, nullptr, which, index, range_sq, x, y, z, label, count,
                    pixel, visible, nullptr, nullptr, info);
}

int range_labels(sicp_context* h, int which, const sicp_range_params* p, const double* beam, const float* origin,
                 const uint32_t* pixel_label, sicp_context* dst, int dst_which, uint32_t* out_label, uint8_t* votes, sicp_range_info* info) {
  return range_call(h, "sicp_range_labels", true, which, p, beam, origin, pixel_label, dst, dst_which, nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, nullptr, nullptr, nullptr, out_label, votes, info);
}

}  // namespace host
}  // namespace sicp
