// deskew_kernels.hip -- sicp_deskew: every point of a scan moved to one instant (driver: deskew.cpp; the rules: include/sicp.h,
// "deskewing a scan").  The host has composed the relative knots K_k = ref^-1 T_k; here the table sits in LDS, a lane finds the
// interval of its point's time by binary search, blends the two knots component by component, takes the rotation from the
// unnormalised quaternion and moves the point -- double operations, each rounded on its own, no sin, cos or sqrt.  A scan
// arrives in firing order, so the lanes of a wave mostly share an interval and their LDS reads are broadcasts; any order is
// correct.  Every lane stores its own outputs; ballots count; integer atomics add the counts.  Every byte is independent of the
// launch shape.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "voxel_key.hpp"

#pragma clang fp contract(off)

namespace sicp {
namespace {

// rule 3, the order of operations (restated in tests/deskew_ref.py)
__device__ __forceinline__ void deskew_point(const double* kt, const double* kq, int nk, double t, double x, double y, double z, float* ox,
                                             float* oy, float* oz, bool* lo, bool* hi) {
  // a: the largest index with kt[a] <= t, limited to 0 .. nk - 2
  int a = 0, b = nk - 1;
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (kt[mid] <= t) a = mid; else b = mid;
  }
  const double ta = kt[a], tb = kt[a + 1];
  *lo = t < kt[0];
  *hi = t > kt[nk - 1];
  double u = __ddiv_rn(__dsub_rn(t, ta), __dsub_rn(tb, ta));
  u = *lo ? 0.0 : (*hi ? 1.0 : u);
  const double w = __dsub_rn(1.0, u);
  const double* A = kq + 7 * a;
  const double* B = A + 7;
  double c[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) c[j] = __dadd_rn(__dmul_rn(w, A[j]), __dmul_rn(u, B[j]));
  const double qx = c[0], qy = c[1], qz = c[2], qw = c[3];
  const double xx = __dmul_rn(qx, qx), yy = __dmul_rn(qy, qy), zz = __dmul_rn(qz, qz), ww = __dmul_rn(qw, qw);
  const double s = __dadd_rn(__dadd_rn(__dadd_rn(xx, yy), zz), ww);
  const double k = __ddiv_rn(2.0, s);
  const double xy = __dmul_rn(qx, qy), xz = __dmul_rn(qx, qz), yz = __dmul_rn(qy, qz);
  const double wx = __dmul_rn(qw, qx), wy = __dmul_rn(qw, qy), wz = __dmul_rn(qw, qz);
  const double r0[4] = {__dsub_rn(1.0, __dmul_rn(k, __dadd_rn(yy, zz))), __dmul_rn(k, __dsub_rn(xy, wz)), __dmul_rn(k, __dadd_rn(xz, wy)), c[4]};
  const double r1[4] = {__dmul_rn(k, __dadd_rn(xy, wz)), __dsub_rn(1.0, __dmul_rn(k, __dadd_rn(xx, zz))), __dmul_rn(k, __dsub_rn(yz, wx)), c[5]};
  const double r2[4] = {__dmul_rn(k, __dsub_rn(xz, wy)), __dmul_rn(k, __dadd_rn(yz, wx)), __dsub_rn(1.0, __dmul_rn(k, __dadd_rn(xx, yy))), c[6]};
  *ox = voxel_xform_row(r0, x, y, z);
  *oy = voxel_xform_row(r1, x, y, z);
  *oz = voxel_xform_row(r2, x, y, z);
}

__global__ __launch_bounds__(256) void deskew_kernel(DeskewArgs a) {
  extern __shared__ __attribute__((aligned(16))) double deskew_lds[];
  double* kt = deskew_lds;
  double* kq = deskew_lds + a.n_knots;
  for (int k = threadIdx.x; k < a.n_knots; k += 256) kt[k] = a.knot_time[k];
  for (int k = threadIdx.x; k < 7 * a.n_knots; k += 256) kq[k] = a.knot_qt[k];
  __syncthreads();
  int moved = 0, bad = 0, c_lo = 0, c_hi = 0;  // (what lane 0 of a wave keeps)
  const int stride = 256 * (int)gridDim.x;
  for (int base = 256 * (int)blockIdx.x; base < a.n; base += stride) {  // (uniform over the workgroup: every lane reaches the ballots)
    const int f = base + (int)threadIdx.x;
    bool m = false, bt = false, lo = false, hi = false;
    if (f < a.n) {
      const int ci = a.caller ? a.caller[f] : f;
      const double t = a.times[ci];
      float px, py, pz;
      if (__dsub_rn(t, t) == 0.0) {  // a finite time
        m = true;
        deskew_point(kt, kq, a.n_knots, t, (double)a.x[f], (double)a.y[f], (double)a.z[f], &px, &py, &pz, &lo, &hi);
      } else {  // rule 4: the point leaves the index
        bt = true;
        px = py = pz = __uint_as_float(0x7fc00000u);
      }
      a.ox[ci] = px; a.oy[ci] = py; a.oz[ci] = pz;
    }
    moved += __popcll(__ballot(m));
    bad += __popcll(__ballot(bt));
    c_lo += __popcll(__ballot(lo));
    c_hi += __popcll(__ballot(hi));
  }
  if ((threadIdx.x & 63) == 0) {
    if (moved) atomicAdd(a.res + kDkMoved, moved);
    if (bad) atomicAdd(a.res + kDkBadTime, bad);
    if (c_lo) atomicAdd(a.res + kDkClampedLo, c_lo);
    if (c_hi) atomicAdd(a.res + kDkClampedHi, c_hi);
  }
}

}  // namespace

hipError_t launch_deskew(const DeskewArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  const long long groups = ((long long)a.n + 255) / 256;
  const unsigned grid = (unsigned)(groups < kDeskewMaxGroups ? groups : kDeskewMaxGroups);
  const size_t lds = sizeof(double) * 8 * (size_t)a.n_knots;  // times | poses: at most 64 KiB
  hipLaunchKernelGGL(deskew_kernel, dim3(grid), dim3(256), lds, st, a);
  return hipGetLastError();
}

}  // namespace sicp
