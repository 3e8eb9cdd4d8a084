// camera_kernels.hip -- sicp_camera_image / sicp_camera_labels / sicp_camera_unproject: a scan through a calibrated pinhole
// camera and a depth frame back out of one (driver: camera.cpp; the rules: include/sicp.h, "camera: depth frames and image
// labels").  Project: a lane per point moves it into the camera's frame with the twelve matrix entries that arrive as kernel
// arguments, gates its depth, distorts and projects it in double -- two divisions, no root -- and enters the pixel with one
// 64-bit atomicMin on (bits((float)Zc) << 32 | f) and one atomicAdd on the count.  Resolve: a lane per pixel decodes the key and
// gathers the winner into one 16-byte record.  Labels: a lane per point takes the smallest winner depth of its window -- the
// window's edge is a template parameter, so the walk has compile-time bounds and lives in registers -- and decides between
// seen, occluded and unclassed.  Unproject: a lane per pixel, the fixed-count undistortion in registers, loads and stores
// coalesced along the row.  Integer atomics and ballots only: every byte is independent of the launch shape.
#include <hip/hip_runtime.h>

#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

__device__ __forceinline__ void count_ballot(bool b, int& acc) { acc += __popcll(__ballot(b)); }
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }

// rule 4 from normalised coordinates: the distorted pair
__device__ __forceinline__ void distort(const CameraArgs& a, double xn, double yn, double& xd, double& yd) {
  const double aa = xn * xn, bb = yn * yn, cc = xn * yn;
  const double r2 = aa + bb;
  const double rad = 1.0 + r2 * (a.k1 + r2 * (a.k2 + r2 * a.k3));
  const double tx = (2.0 * a.p1) * cc + a.p2 * (r2 + 2.0 * aa);
  const double ty = a.p1 * (r2 + 2.0 * bb) + (2.0 * a.p2) * cc;
  xd = xn * rad + tx;
  yd = yn * rad + ty;
}

// ---- project -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void camera_project_kernel(CameraArgs a) {
  int kept = 0, outside = 0;  // (what lane 0 of a wave keeps)
  const double wmax = (double)(a.W - 1), hmax = (double)(a.H - 1);
  const int stride = 256 * (int)gridDim.x;
  for (int base = 256 * (int)blockIdx.x; base < a.n; base += stride) {  // (uniform over the workgroup: every lane reaches the ballots)
    const int f = base + (int)threadIdx.x;
    bool k = false, o = false;
    if (f < a.n) {
      const double x = (double)a.x[f], y = (double)a.y[f], z = (double)a.z[f];
      const double Xc = ((a.m[0] * x + a.m[1] * y) + a.m[2] * z) + a.m[3];     // rule 1
      const double Yc = ((a.m[4] * x + a.m[5] * y) + a.m[6] * z) + a.m[7];
      const double Zc = ((a.m[8] * x + a.m[9] * y) + a.m[10] * z) + a.m[11];
      int pix = -1;
      float uf = quiet_nan(), vf = quiet_nan(), zf = 0.f;
      k = Zc >= a.min_depth && Zc < a.max_depth;                               // rule 2
      if (k) {
        const double xn = Xc / Zc, yn = Yc / Zc;                               // rule 3
        const double r2 = xn * xn + yn * yn;
        if (r2 <= a.max_tan_sq) {
          double xd, yd;
          distort(a, xn, yn, xd, yd);                                          // rule 4
          const double u = a.fx * xd + a.cx, v = a.fy * yd + a.cy;             // rule 5
          uf = (float)u; vf = (float)v;
          const double cf = floor(u + 0.5), rf = floor(v + 0.5);
          if (cf >= 0.0 && cf <= wmax && rf >= 0.0 && rf <= hmax) {
            pix = (int)rf * a.W + (int)cf;
            zf = (float)Zc;
            atomicMin(&a.key[pix], ((u64)__float_as_uint(zf) << 32) | (u64)(unsigned)f);  // rule 6
            atomicAdd(&a.count[pix], 1u);
          }
        }
        o = pix < 0;
      }
      a.pix[f] = pix;
      a.zf[f] = zf;
      const int ci = a.caller ? a.caller[f] : f;
      if (a.o_pixel) a.o_pixel[ci] = pix;
      if (a.o_u) a.o_u[ci] = uf;
      if (a.o_v) a.o_v[ci] = vf;
    }
    count_ballot(k, kept);
    count_ballot(o, outside);
  }
  if ((threadIdx.x & 63) == 0) {
    if (kept) atomicAdd(a.res + kCmKept, kept);
    if (outside) atomicAdd(a.res + kCmOutside, outside);
  }
}

// ---- resolve -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void camera_resolve_kernel(CameraArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int n_pix = a.W * a.H;
  bool hit = false;
  if (p < n_pix) {
    const u64 key = a.key[p];
    hit = key != kCameraEmptyKey;
    int index = -1;
    float depth = 0.f, x = 0.f, y = 0.f, z = 0.f;
    uint32_t label = 0;
    if (hit) {
      const int f = (int)(unsigned)(key & 0xffffffffull);
      depth = __uint_as_float((unsigned)(key >> 32));
      x = a.x[f]; y = a.y[f]; z = a.z[f];
      label = a.label ? a.label[f] : 0u;
      index = a.caller ? a.caller[f] : f;
    }
    a.rec[p] = make_float4(x, y, z, hit ? depth : __uint_as_float(0x7f800000u));
    if (a.o_index) a.o_index[p] = index;
    if (a.o_depth) a.o_depth[p] = depth;
    if (a.o_x) a.o_x[p] = x;
    if (a.o_y) a.o_y[p] = y;
    if (a.o_z) a.o_z[p] = z;
    if (a.o_label) a.o_label[p] = label;
  }
  const u64 ballot = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(a.res + kCmPixelsHit, (int)__popcll(ballot));
}

// ---- visible -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void camera_visible_kernel(CameraArgs a) {
  const int stride = 256 * (int)gridDim.x;
  for (int f = 256 * (int)blockIdx.x + (int)threadIdx.x; f < a.n; f += stride) {
    const int pix = a.pix[f];
    if (pix >= 0 && (unsigned)(a.key[pix] & 0xffffffffull) == (unsigned)f) a.o_visible[a.caller ? a.caller[f] : f] = 1;
  }
}

// ---- labels --------------------------------------------------------------------------------------------------------------
// S: the window's edge.  An empty pixel's record holds +inf and a pixel beyond the border is skipped, so the minimum runs over
// the occupied pixels of the truncated block; the point's own pixel is among them.
template <int S>
__global__ __launch_bounds__(256) void camera_labels_kernel(CameraArgs a) {
  constexpr int half = S / 2;
  const int W = a.W, H = a.H;
  int labelled = 0, occluded = 0, unclassed = 0;
  const int stride = 256 * (int)gridDim.x;
  for (int base = 256 * (int)blockIdx.x; base < a.n; base += stride) {
    const int f = base + (int)threadIdx.x;
    int state = 0;
    if (f < a.n) {
      const int pix = a.pix[f];
      uint32_t out = a.label ? a.label[f] : 0u;                                // rule 9: the point's own label
      if (pix >= 0) {
        const int r = pix / W, c = pix - r * W;
        float zmin = __uint_as_float(0x7f800000u);
        for (int wr = -half; wr <= half; ++wr) {                               // rule 7
          const int rr = r + wr;
          if (rr < 0 || rr >= H) continue;
          const float4* row = a.rec + (size_t)rr * (size_t)W;
#pragma unroll
          for (int wc = -half; wc <= half; ++wc) {
            const int cc = c + wc;
            if (cc >= 0 && cc < W) zmin = fminf(zmin, row[cc].w);
          }
        }
        const double zd = (double)a.zf[f], zm = (double)zmin;
        const bool occ = (zd - zm) > (a.occlusion_abs + a.occlusion_rel * zm); // rule 8
        const uint32_t cls = a.pixel_label[pix];
        state = occ ? 2 : (cls != 0u ? 1 : 3);
        if (state == 1) out = cls;
      }
      const int ci = a.caller ? a.caller[f] : f;
      if (a.o_out_label) a.o_out_label[ci] = out;
      if (a.o_state) a.o_state[ci] = (uint8_t)state;
    }
    count_ballot(state == 1, labelled);
    count_ballot(state == 2, occluded);
    count_ballot(state == 3, unclassed);
  }
  if ((threadIdx.x & 63) == 0) {
    if (labelled) atomicAdd(a.res + kCmLabelled, labelled);
    if (occluded) atomicAdd(a.res + kCmOccluded, occluded);
    if (unclassed) atomicAdd(a.res + kCmUnclassed, unclassed);
  }
}

// ---- unproject -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void camera_unproject_kernel(CameraArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int n_pix = a.W * a.H;
  bool valid = false;
  if (p < n_pix) {
    const double Z = a.depth_u16 ? (double)a.depth_u16[p] * a.depth_scale : (double)a.depth_f32[p];  // rule 11
    valid = Z >= a.min_depth && Z < a.max_depth;  // (a NaN fails both, an infinity the second: max_depth is finite)
    float ox = quiet_nan(), oy = quiet_nan(), oz = quiet_nan();
    if (valid) {
      const int r = p / a.W, c = p - r * a.W;
      const double xd = ((double)c - a.cx) / a.fx, yd = ((double)r - a.cy) / a.fy;  // rule 12
      double x = xd, y = yd;
      for (int it = 0; it < a.iterations; ++it) {
        const double aa = x * x, bb = y * y, cc = x * y;
        const double r2 = aa + bb;
        const double rad = 1.0 + r2 * (a.k1 + r2 * (a.k2 + r2 * a.k3));
        const double tx = (2.0 * a.p1) * cc + a.p2 * (r2 + 2.0 * aa);
        const double ty = a.p1 * (r2 + 2.0 * bb) + (2.0 * a.p2) * cc;
        x = (xd - tx) / rad;
        y = (yd - ty) / rad;
      }
      const double px = x * Z, py = y * Z;                                     // rule 13
      ox = (float)(((a.m[0] * px + a.m[1] * py) + a.m[2] * Z) + a.m[3]);
      oy = (float)(((a.m[4] * px + a.m[5] * py) + a.m[6] * Z) + a.m[7]);
      oz = (float)(((a.m[8] * px + a.m[9] * py) + a.m[10] * Z) + a.m[11]);
    }
    a.p_x[p] = ox; a.p_y[p] = oy; a.p_z[p] = oz;
    if (a.p_valid) a.p_valid[p] = valid ? 1 : 0;
  }
  const u64 ballot = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(a.res + kCmValid, (int)__popcll(ballot));
}

bool camera_shape_ok(const CameraArgs& a) {
  return a.W >= 8 && a.W <= kCameraMaxWidth && a.H >= 8 && a.H <= kCameraMaxHeight && a.n >= 0;
}
unsigned point_groups(int n) {
  const long long groups = ((long long)n + 255) / 256;
  return (unsigned)(groups < kCameraMaxGroups ? groups : kCameraMaxGroups);
}
unsigned pixel_groups(const CameraArgs& a) { return (unsigned)((a.W * a.H + 255) / 256); }  // at most 2^16

}  // namespace

hipError_t launch_camera_project(const CameraArgs& a, hipStream_t st) {
  if (!camera_shape_ok(a) || !a.key || !a.count || !a.pix || !a.zf) return hipErrorInvalidValue;
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(camera_project_kernel, dim3(point_groups(a.n)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_camera_resolve(const CameraArgs& a, hipStream_t st) {
  if (!camera_shape_ok(a) || !a.key || !a.rec) return hipErrorInvalidValue;
  hipLaunchKernelGGL(camera_resolve_kernel, dim3(pixel_groups(a)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_camera_visible(const CameraArgs& a, hipStream_t st) {
  if (!camera_shape_ok(a) || !a.o_visible) return hipErrorInvalidValue;
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(camera_visible_kernel, dim3(point_groups(a.n)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_camera_labels(const CameraArgs& a, hipStream_t st) {
  if (!camera_shape_ok(a) || a.window < 1 || a.window > kCameraMaxWindow || a.window % 2 == 0 || !a.pixel_label || !a.rec)
    return hipErrorInvalidValue;
  if (a.n <= 0) return hipSuccess;
  const dim3 grid(point_groups(a.n)), block(256);
  switch (a.window) {
    case 1: hipLaunchKernelGGL(camera_labels_kernel<1>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(camera_labels_kernel<3>, grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL(camera_labels_kernel<5>, grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL(camera_labels_kernel<7>, grid, block, 0, st, a); break;
    case 9: hipLaunchKernelGGL(camera_labels_kernel<9>, grid, block, 0, st, a); break;
    case 11: hipLaunchKernelGGL(camera_labels_kernel<11>, grid, block, 0, st, a); break;
    case 13: hipLaunchKernelGGL(camera_labels_kernel<13>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(camera_labels_kernel<15>, grid, block, 0, st, a); break;
  }
  return hipGetLastError();
}

hipError_t launch_camera_unproject(const CameraArgs& a, hipStream_t st) {
  if (!camera_shape_ok(a) || a.iterations < 0 || a.iterations > kCameraMaxIterations || (a.depth_u16 != nullptr) == (a.depth_f32 != nullptr) ||
      !a.p_x || !a.p_y || !a.p_z)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(camera_unproject_kernel, dim3(pixel_groups(a)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sicp
