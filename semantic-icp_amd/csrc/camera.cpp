// camera.cpp -- sicp_camera_image / sicp_camera_labels / sicp_camera_unproject / sicp_camera_matrices (include/sicp.h, "camera:
// depth frames and image labels"): the argument checks, the two 3 x 4 matrices formed once in double, the way up of the caller
// map, the network's classes or the depth frame through the call's scratch, the launches of camera_kernels.hip, one read-back,
// and, with dst, the relabelled cloud or the frame's points staged into dst's slot through the path of sicp_set_cloud.  Without
// dst nothing the handle holds for align() is touched.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

struct CameraScratch {
  DevBuf<int> caller, pix, res, o_index, o_pixel;
  DevBuf<unsigned long long> key;
  DevBuf<uint32_t> count, pixel_label, o_label, o_out_label;
  DevBuf<float4> rec;
  DevBuf<float> zf, o_depth, o_x, o_y, o_z, o_u, o_v, depth_f32;
  DevBuf<uint16_t> depth_u16;
  DevBuf<uint8_t> o_visible, o_state;
  int device = -1;
  bool idle = true;
  ~CameraScratch() {
    DevArena::release_scratch(device, idle, caller, pix, res, o_index, o_pixel, key, count, pixel_label, o_label, o_out_label, rec, zf,
                              o_depth, o_x, o_y, o_z, o_u, o_v, depth_f32, depth_u16, o_visible, o_state);
  }
};

bool slot_ok(int which) { return which == SICP_SOURCE || which == SICP_TARGET; }
size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }
constexpr uint32_t kQuietNan = 0x7fc00000u;

// the parameter checks of rule 15; "" when the parameters are accepted
std::string bad_params(const sicp_camera_params& p) {
  if (p.width < 8 || p.width > SICP_CAMERA_MAX_WIDTH) return "width must be in 8 .. " + std::to_string(SICP_CAMERA_MAX_WIDTH);
  if (p.height < 8 || p.height > SICP_CAMERA_MAX_HEIGHT) return "height must be in 8 .. " + std::to_string(SICP_CAMERA_MAX_HEIGHT);
  if (!std::isfinite(p.fx) || !std::isfinite(p.fy) || !std::isfinite(p.cx) || !std::isfinite(p.cy)) return "fx, fy, cx, cy must be finite";
  if (!(p.fx > 0.0) || !(p.fy > 0.0)) return "fx and fy must be above 0";
  if (!std::isfinite(p.k1) || !std::isfinite(p.k2) || !std::isfinite(p.p1) || !std::isfinite(p.p2) || !std::isfinite(p.k3))
    return "a distortion coefficient is not finite";
  if (!(p.min_depth > 0.0)) return "min_depth must be above 0";
  if (!std::isfinite(p.max_depth) || !(p.max_depth > p.min_depth)) return "max_depth must be finite and above min_depth";
  if (!(p.max_tan_sq > 0.0)) return "max_tan_sq must be above 0";
  if (!(p.depth_scale > 0.0)) return "depth_scale must be above 0";
  if (p.undistort_iterations < 0 || p.undistort_iterations > 64) return "undistort_iterations must be in 0 .. 64";
  if (p.window < 1 || p.window > SICP_CAMERA_MAX_WINDOW || p.window % 2 == 0)
    return "window must be odd and in 1 .. " + std::to_string(SICP_CAMERA_MAX_WINDOW);
  if (!(p.occlusion_abs >= 0.0)) return "occlusion_abs must be >= 0";
  if (!(p.occlusion_rel >= 0.0)) return "occlusion_rel must be >= 0";
  return "";
}

// camera -> cloud as the engine forms a pose matrix, cloud -> camera as (R^T | -R^T t); "" when the pose is accepted
std::string make_matrices(const double* qt, double* to_cloud, double* to_cam) {
  const double ident[7] = {0, 0, 0, 1, 0, 0, 0};
  const double* q = qt ? qt : ident;
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(q[k])) return "camera_qt is not finite";
  if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0) return "the quaternion of camera_qt is zero";
  double M[12];
  matrix34(q, M);
  for (int i = 0; i < 3; ++i) {
    const double a = M[i] * M[3], b = M[4 + i] * M[7], c = M[8 + i] * M[11];
    const double s = (a + b) + c;
    to_cam[4 * i + 0] = M[i]; to_cam[4 * i + 1] = M[4 + i]; to_cam[4 * i + 2] = M[8 + i];
    to_cam[4 * i + 3] = -s;
  }
  std::memcpy(to_cloud, M, sizeof M);
  return "";
}

void set_intrinsics(sicp::CameraArgs& A, const sicp_camera_params& p) {
  A.W = p.width; A.H = p.height; A.window = p.window; A.iterations = p.undistort_iterations;
  A.fx = p.fx; A.fy = p.fy; A.cx = p.cx; A.cy = p.cy;
  A.k1 = p.k1; A.k2 = p.k2; A.p1 = p.p1; A.p2 = p.p2; A.k3 = p.k3;
  A.min_depth = p.min_depth; A.max_depth = p.max_depth; A.max_tan_sq = p.max_tan_sq; A.depth_scale = p.depth_scale;
  A.occlusion_abs = p.occlusion_abs; A.occlusion_rel = p.occlusion_rel;
}

struct Copy { void* host; const void* dev; size_t bytes, at; };

// sicp_camera_image and sicp_camera_labels: carry = the call is sicp_camera_labels
int project_call(sicp_context* h, const char* name, bool carry, int which, const sicp_camera_params* p, const double* qt,
                 const uint32_t* pixel_label, sicp_context* dst, int dst_which, int32_t* index, float* depth, float* x, float* y, float* z,
                 uint32_t* label, uint32_t* count, int32_t* pixel, float* u, float* v, uint8_t* visible, uint32_t* out_label,
                 uint8_t* state, sicp_camera_info* info) {
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
  if (carry && !pixel_label) return refuse("pixel_label is NULL");
  double to_cloud[12], to_cam[12];
  {
    const std::string why = make_matrices(qt, to_cloud, to_cam);
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
  CameraScratch X;
  X.device = h->device;
  X.idle = false;
  const size_t mc = (size_t)std::max(nc, 1), m = (size_t)std::max(n, 1);
  int res[kCmRes] = {0, 0, 0, 0, 0, 0, 0, 0};

  sicp::CameraArgs A;
  std::memset(&A, 0, sizeof A);
  A.n = n; A.n_caller = nc;
  set_intrinsics(A, *p);
  std::memcpy(A.m, to_cam, sizeof to_cam);
  A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
  A.label = labels ? c.rl.p : nullptr;

  // what comes back, each part at an 8-byte boundary of the pinned stage, after what goes up: caller map | classes
  std::vector<Copy> back;
  const size_t o_caller = 0, o_pl = o_caller + up8(mapped ? 4 * m : 0), o_res = o_pl + up8(carry ? 4 * np : 0);
  size_t o_end = o_res + up8(sizeof res);
  auto want = [&](void* host, const void* dev, size_t bytes) {
    back.push_back(Copy{host, dev, bytes, o_end});
    o_end += up8(bytes);
  };
  HIPCHECK(X.key.reserve(np)); HIPCHECK(X.count.reserve(np)); HIPCHECK(X.rec.reserve(np));
  HIPCHECK(X.pix.reserve(m)); HIPCHECK(X.zf.reserve(m)); HIPCHECK(X.res.reserve(kCmRes));
  A.key = X.key.p; A.count = X.count.p; A.rec = X.rec.p; A.pix = X.pix.p; A.zf = X.zf.p; A.res = X.res.p;
  if (mapped) { HIPCHECK(X.caller.reserve(m)); A.caller = X.caller.p; }
  if (carry) {
    HIPCHECK(X.pixel_label.reserve(np)); A.pixel_label = X.pixel_label.p;
    if (out_label || dst) { HIPCHECK(X.o_out_label.reserve(mc)); A.o_out_label = X.o_out_label.p; }
    if (state) { HIPCHECK(X.o_state.reserve(mc)); A.o_state = X.o_state.p; }
  } else {
    if (index) { HIPCHECK(X.o_index.reserve(np)); A.o_index = X.o_index.p; want(index, A.o_index, 4 * np); }
    if (depth) { HIPCHECK(X.o_depth.reserve(np)); A.o_depth = X.o_depth.p; want(depth, A.o_depth, 4 * np); }
    if (x) { HIPCHECK(X.o_x.reserve(np)); A.o_x = X.o_x.p; want(x, A.o_x, 4 * np); }
    if (y) { HIPCHECK(X.o_y.reserve(np)); A.o_y = X.o_y.p; want(y, A.o_y, 4 * np); }
    if (z) { HIPCHECK(X.o_z.reserve(np)); A.o_z = X.o_z.p; want(z, A.o_z, 4 * np); }
    if (label) { HIPCHECK(X.o_label.reserve(np)); A.o_label = X.o_label.p; want(label, A.o_label, 4 * np); }
    if (count) want(count, A.count, 4 * np);
    if (pixel) { HIPCHECK(X.o_pixel.reserve(mc)); A.o_pixel = X.o_pixel.p; }
    if (u) { HIPCHECK(X.o_u.reserve(mc)); A.o_u = X.o_u.p; }
    if (v) { HIPCHECK(X.o_v.reserve(mc)); A.o_v = X.o_v.p; }
    if (visible) { HIPCHECK(X.o_visible.reserve(mc)); A.o_visible = X.o_visible.p; }
  }
  if (nc > 0) {
    if (A.o_pixel) want(pixel, A.o_pixel, 4 * (size_t)nc);
    if (A.o_u) want(u, A.o_u, 4 * (size_t)nc);
    if (A.o_v) want(v, A.o_v, 4 * (size_t)nc);
    if (A.o_visible) want(visible, A.o_visible, (size_t)nc);
    if (A.o_out_label) want(out_label, A.o_out_label, 4 * (size_t)nc);  // (host NULL with dst alone: it stays in the stage)
    if (A.o_state) want(state, A.o_state, (size_t)nc);
  }
  // with dst: x | y | z of every point the caller handed over, behind everything else (the labels are out_label's part)
  const size_t o_xyz = o_end;
  if (dst) o_end += 3 * 4 * mc;
  HIPCHECK(h->cm_stage.resize(o_end));
  unsigned char* o = h->cm_stage.data();

  if (mapped) {  // points were dropped: finite index -> caller index
    std::memcpy(o + o_caller, c.keep.data(), 4 * (size_t)n);
    HIPCHECK(hipMemcpyAsync(X.caller.p, o + o_caller, 4 * (size_t)n, hipMemcpyHostToDevice, st));
  }
  if (carry) {
    std::memcpy(o + o_pl, pixel_label, 4 * np);
    HIPCHECK(hipMemcpyAsync(X.pixel_label.p, o + o_pl, 4 * np, hipMemcpyHostToDevice, st));
  }
  HIPCHECK(hipMemsetAsync(X.key.p, 0xff, 8 * np, st));
  HIPCHECK(hipMemsetAsync(X.count.p, 0, 4 * np, st));
  HIPCHECK(hipMemsetAsync(X.res.p, 0, sizeof res, st));
  // the entries of the points that are not finite
  if (A.o_pixel) HIPCHECK(hipMemsetAsync(A.o_pixel, 0xff, 4 * mc, st));
  if (A.o_u) HIPCHECK(hipMemsetD32Async((hipDeviceptr_t)A.o_u, (int)kQuietNan, mc, st));
  if (A.o_v) HIPCHECK(hipMemsetD32Async((hipDeviceptr_t)A.o_v, (int)kQuietNan, mc, st));
  if (A.o_visible) HIPCHECK(hipMemsetAsync(A.o_visible, 0, mc, st));
  if (A.o_out_label) HIPCHECK(hipMemsetAsync(A.o_out_label, 0, 4 * mc, st));
  if (A.o_state) HIPCHECK(hipMemsetAsync(A.o_state, 0, mc, st));
  HIPCHECK(sicp::launch_camera_project(A, st));
  HIPCHECK(sicp::launch_camera_resolve(A, st));
  if (carry) HIPCHECK(sicp::launch_camera_labels(A, st));
  else if (A.o_visible) HIPCHECK(sicp::launch_camera_visible(A, st));
  HIPCHECK(hipMemcpyAsync(o + o_res, X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
  for (const Copy& k : back) HIPCHECK(hipMemcpyAsync(o + k.at, k.dev, k.bytes, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  X.idle = true;
  std::memcpy(res, o + o_res, sizeof res);

  sicp_camera_info I;
  std::memset(&I, 0, sizeof I);
  I.n_points = nc;
  I.n_finite = n;
  I.n_kept = res[kCmKept];
  I.n_outside = res[kCmOutside];
  I.n_pixels_hit = res[kCmPixelsHit];
  I.n_labelled = res[kCmLabelled];
  I.n_occluded = res[kCmOccluded];
  I.n_unclassed = res[kCmUnclassed];
  int rc = SICP_OK;
  if (dst) {  // (in place: `c` is the new cloud from here on)
    // everything is on the host before dst's slot lets go of its old cloud (range.cpp): the finite points from the cloud's
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

void camera_default_params(sicp_camera_params* p) {
  std::memset(p, 0, sizeof *p);
  p->width = 640;
  p->height = 480;
  p->fx = 525.0; p->fy = 525.0; p->cx = 319.5; p->cy = 239.5;
  p->min_depth = 0.3;
  p->max_depth = 100.0;
  p->max_tan_sq = 4.0;
  p->depth_scale = 0.001;
  p->undistort_iterations = 20;
  p->window = 5;
  p->occlusion_abs = 0.3;
  p->occlusion_rel = 0.02;
}

int camera_matrices(const double* qt, double* cam_to_cloud, double* cloud_to_cam) {
  double to_cloud[12], to_cam[12];
  if (!make_matrices(qt, to_cloud, to_cam).empty()) return SICP_ERR_INVALID_ARGUMENT;
  if (cam_to_cloud) std::memcpy(cam_to_cloud, to_cloud, sizeof to_cloud);
  if (cloud_to_cam) std::memcpy(cloud_to_cam, to_cam, sizeof to_cam);
  return SICP_OK;
}

int camera_image(sicp_context* h, int which, const sicp_camera_params* p, const double* qt, int32_t* index, float* depth, float* x,
                 float* y, float* z, uint32_t* label, uint32_t* count, int32_t* pixel, float* u, float* v, uint8_t* visible,
                 sicp_camera_info* info) {
  return project_call(h, "sicp_camera_image", false, which, p, qt, nullptr, nullptr, which, index, depth, x, y, z, label, count, pixel, u, v,
                      visible, nullptr, nullptr, info);
}

int camera_labels(sicp_context* h, int which, const sicp_camera_params* p, const double* qt, const uint32_t* pixel_label,
                  sicp_context* dst, int dst_which, uint32_t* out_label, uint8_t* state, sicp_camera_info* info) {
  return project_call(h, "sicp_camera_labels", true, which, p, qt, pixel_label, dst, dst_which, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out_label, state, info);
}

int camera_unproject(sicp_context* h, const sicp_camera_params* p, const double* qt, const uint16_t* depth_u16, const float* depth_f32,
                     const uint32_t* label, sicp_context* dst, int dst_which, float* x, float* y, float* z, uint8_t* valid,
                     sicp_camera_info* info) {
  const char* name = "sicp_camera_unproject";
  if (!h) return SICP_ERR_INVALID_ARGUMENT;
  auto refuse = [&](const std::string& why) {
    h->last_error = std::string(name) + ": " + why + "; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (!p) return refuse("params is NULL");
  if (dst && !slot_ok(dst_which)) return refuse("dst_which is neither SICP_SOURCE nor SICP_TARGET");
  {
    const std::string why = bad_params(*p);
    if (!why.empty()) return refuse(why);
  }
  if ((depth_u16 != nullptr) == (depth_f32 != nullptr)) return refuse("exactly one of depth_u16 and depth_f32 must be given");
  double to_cloud[12], to_cam[12];
  {
    const std::string why = make_matrices(qt, to_cloud, to_cam);
    if (!why.empty()) return refuse(why);
  }
  if (dst && dst->device != h->device) return refuse("dst is on device " + std::to_string(dst->device) + ", the handle on " + std::to_string(h->device));
  const double t_begin = now_ms();
  const int W = p->width, H = p->height;
  const size_t np = (size_t)W * (size_t)H;

  SICPCHECK(set_device(h));
  hipStream_t st = h->stream;
  CameraScratch X;
  X.device = h->device;
  X.idle = false;
  int res[kCmRes] = {0, 0, 0, 0, 0, 0, 0, 0};

  sicp::CameraArgs A;
  std::memset(&A, 0, sizeof A);
  set_intrinsics(A, *p);
  std::memcpy(A.m, to_cloud, sizeof to_cloud);
  HIPCHECK(X.o_x.reserve(np)); HIPCHECK(X.o_y.reserve(np)); HIPCHECK(X.o_z.reserve(np)); HIPCHECK(X.res.reserve(kCmRes));
  A.p_x = X.o_x.p; A.p_y = X.o_y.p; A.p_z = X.o_z.p; A.res = X.res.p;
  if (valid) { HIPCHECK(X.o_visible.reserve(np)); A.p_valid = X.o_visible.p; }
  const size_t depth_bytes = (depth_u16 ? 2 : 4) * np;
  if (depth_u16) { HIPCHECK(X.depth_u16.reserve(np)); A.depth_u16 = X.depth_u16.p; }
  else { HIPCHECK(X.depth_f32.reserve(np)); A.depth_f32 = X.depth_f32.p; }

  // the pinned stage: depth (up) | counts | x | y | z | valid (back); the labels go from the caller's array into dst
  const size_t o_depth = 0, o_res = o_depth + up8(depth_bytes), o_x = o_res + up8(sizeof res), o_y = o_x + up8(4 * np),
               o_z = o_y + up8(4 * np), o_valid = o_z + up8(4 * np), o_end = o_valid + up8(valid ? np : 0);
  HIPCHECK(h->cm_stage.resize(o_end));
  unsigned char* o = h->cm_stage.data();
  std::memcpy(o + o_depth, depth_u16 ? (const void*)depth_u16 : (const void*)depth_f32, depth_bytes);
  HIPCHECK(hipMemcpyAsync(depth_u16 ? (void*)X.depth_u16.p : (void*)X.depth_f32.p, o + o_depth, depth_bytes, hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemsetAsync(X.res.p, 0, sizeof res, st));
  HIPCHECK(sicp::launch_camera_unproject(A, st));
  HIPCHECK(hipMemcpyAsync(o + o_res, X.res.p, sizeof res, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(o + o_x, A.p_x, 4 * np, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(o + o_y, A.p_y, 4 * np, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(o + o_z, A.p_z, 4 * np, hipMemcpyDeviceToHost, st));
  if (valid) HIPCHECK(hipMemcpyAsync(o + o_valid, A.p_valid, np, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  X.idle = true;
  std::memcpy(res, o + o_res, sizeof res);

  sicp_camera_info I;
  std::memset(&I, 0, sizeof I);
  I.n_points = (int64_t)np;
  I.n_finite = res[kCmValid];
  I.n_valid = res[kCmValid];
  if (dst) {
    if (res[kCmValid] == 0) {
      h->last_error = std::string(name) + ": the frame has no valid pixel; dst keeps its cloud";
      return SICP_ERR_TOO_FEW_POINTS;
    }
    const StridedCloud in = {(const char*)(o + o_x), (const char*)(o + o_y), (const char*)(o + o_z), (const char*)label, 4, 4};
    const int rc = set_cloud_common(dst, dst_which, (int32_t)np, in);
    if (rc != SICP_OK) {
      if (dst != h) h->last_error = std::string(name) + ": dst: " + dst->last_error;
      return rc;
    }
  }
  if (x) std::memcpy(x, o + o_x, 4 * np);
  if (y) std::memcpy(y, o + o_y, 4 * np);
  if (z) std::memcpy(z, o + o_z, 4 * np);
  if (valid) std::memcpy(valid, o + o_valid, np);
  if (info) {
    I.t_total_ms = now_ms() - t_begin;
    *info = I;
  }
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
