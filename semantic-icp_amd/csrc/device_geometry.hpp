// device_geometry.hpp -- the closed-form GICP residual shared by the weight and the solve kernels
// (device code; included inside the kernel files).
#ifndef SICP_DEVICE_GEOMETRY_HPP_
#define SICP_DEVICE_GEOMETRY_HPP_
#include "kernels.h"

namespace sicp {

// one rotation of the cyclic Jacobi eigensolver of a symmetric 3x3 matrix (A := J^T A J, V := V J): the normal
// estimation of cov_body and of the bootstrap's normal kernel
__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&V)[3][3], int p, int q) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double tau = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
  const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double akp = A[k][p], akq = A[k][q];
    A[k][p] = c * akp - s * akq;
    A[k][q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double apk = A[p][k], aqk = A[q][k];
    A[p][k] = c * apk - s * aqk;
    A[q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k][p], vkq = V[k][q];
    V[k][p] = c * vkp - s * vkq;
    V[k][q] = s * vkp + c * vkq;
  }
}

// ------------------------------------------------------------------------------------------
// per-correspondence math (closed form of gicp_cost_function.h:31-70
// chained with Sophus' Dx_this_mul_exp_x_at_0, for C = I - (1-eps) n n^T)
// ------------------------------------------------------------------------------------------
struct Corr {
  double r;        // res^T A^-1 res  (the Ceres residual: squared Mahalanobis distance)
  double J[6];     // d r / d delta, T*exp(delta), delta = [upsilon; omega]
  double detA;
};

template <bool WANT_J>
__device__ __forceinline__ void corr_eval(const Pose& P, double one_m_eps, double psx, double psy,
                                          double psz, double nsx, double nsy, double nsz,
                                          double ptx, double pty, double ptz, double ntx,
                                          double nty, double ntz, Corr& o) {
  // pure float64 algebra with tolerance-level parity (1e-9).  NOT contracted: this function is inlined into several
  // kernels (the weight kernels, the label kernel, the search's weight epilogue) and whether a multiply-add pair fuses
  // would be each context's own choice -- the as-double Probability() branch (quirk Q1 off) then differs in the last
  // bit from kernel to kernel.  Separate multiplies and adds are the same everywhere.
#pragma clang fp contract(off)
  const double* R = P.R;
  const double mx = R[0] * nsx + R[1] * nsy + R[2] * nsz;
  const double my = R[3] * nsx + R[4] * nsy + R[5] * nsz;
  const double mz = R[6] * nsx + R[7] * nsy + R[8] * nsz;
  // A = C_t + R C_s R^T = 2I - (1-eps)(n_t n_t^T + m m^T)
  const double a00 = 2.0 - one_m_eps * (ntx * ntx + mx * mx);
  const double a01 = -one_m_eps * (ntx * nty + mx * my);
  const double a02 = -one_m_eps * (ntx * ntz + mx * mz);
  const double a11 = 2.0 - one_m_eps * (nty * nty + my * my);
  const double a12 = -one_m_eps * (nty * ntz + my * mz);
  const double a22 = 2.0 - one_m_eps * (ntz * ntz + mz * mz);
  const double rx = ptx - (R[0] * psx + R[1] * psy + R[2] * psz + P.t[0]);
  const double ry = pty - (R[3] * psx + R[4] * psy + R[5] * psz + P.t[1]);
  const double rz = ptz - (R[6] * psx + R[7] * psy + R[8] * psz + P.t[2]);
  // Eigen Matrix3d::inverse(): cofactors / determinant
  const double k00 = a11 * a22 - a12 * a12;
  const double k01 = a02 * a12 - a01 * a22;
  const double k02 = a01 * a12 - a02 * a11;
  const double k11 = a00 * a22 - a02 * a02;
  const double k12 = a01 * a02 - a00 * a12;
  const double k22 = a00 * a11 - a01 * a01;
  const double det = a00 * k00 + a01 * k01 + a02 * k02;
  const double inv = 1.0 / det;
  const double ax = inv * (k00 * rx + k01 * ry + k02 * rz);
  const double ay = inv * (k01 * rx + k11 * ry + k12 * rz);
  const double az = inv * (k02 * rx + k12 * ry + k22 * rz);
  o.r = rx * ax + ry * ay + rz * az;
  o.detA = det;
  if (WANT_J) {
    const double bx = R[0] * ax + R[3] * ay + R[6] * az;  // b = R^T a
    const double by = R[1] * ax + R[4] * ay + R[7] * az;
    const double bz = R[2] * ax + R[5] * ay + R[8] * az;
    const double nb = one_m_eps * (nsx * bx + nsy * by + nsz * bz);
    const double cx = psx + bx - nb * nsx;  // c = p_s + C_s b
    const double cy = psy + by - nb * nsy;
    const double cz = psz + bz - nb * nsz;
    o.J[0] = -2.0 * bx; o.J[1] = -2.0 * by; o.J[2] = -2.0 * bz;
    o.J[3] = 2.0 * (by * cz - bz * cy);
    o.J[4] = 2.0 * (bz * cx - bx * cz);
    o.J[5] = 2.0 * (bx * cy - by * cx);
  }
}

// r and det A for Probability() AS A DOUBLE (quirk Q1 off), by the reference's own sequence of operations on the full
// matrices (gicp_cost_function.h:75-87: R C_s R^T, + C_t, the cofactor inverse, res^T (M res)) with C = I - (1-eps) n n^T
// formed entry by entry as sicp_covariances reports it.  A has condition 2 / eps: the closed form above and this sequence are
// both right to about (2 / eps) * 2^-52 * r, which exp(-r / 2) turns into a RELATIVE difference of 3e-11 between them at
// r = 774, eps = 1e-3 -- beyond the 1e-11 the double is held to.  The bool only asks whether the product is 0 and keeps
// the closed form; the solve never calls this.
__device__ __forceinline__ void corr_eval_literal(const Pose& P, double one_m_eps, double psx, double psy, double psz,
                                                  double nsx, double nsy, double nsz, double ptx, double pty, double ptz,
                                                  double ntx, double nty, double ntz, Corr& o) {
#pragma clang fp contract(off)
  const double* R = P.R;
  const double ns[3] = {nsx, nsy, nsz}, nt[3] = {ntx, nty, ntz};
  double Cs[3][3], A[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) {
      const double d = a == b ? 1.0 : 0.0;
      Cs[a][b] = Cs[b][a] = d - one_m_eps * ns[a] * ns[b];
      A[a][b] = A[b][a] = d - one_m_eps * nt[a] * nt[b];  // C_t, for now
    }
  double RC[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) RC[i][j] = R[3 * i] * Cs[0][j] + R[3 * i + 1] * Cs[1][j] + R[3 * i + 2] * Cs[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i][j] = A[i][j] + (RC[i][0] * R[3 * j] + RC[i][1] * R[3 * j + 1] + RC[i][2] * R[3 * j + 2]);
  // Eigen Matrix3d::inverse(): cofactors / determinant, all nine entries (A is symmetric only up to rounding)
  const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1];
  const double c10 = A[1][2] * A[2][0] - A[1][0] * A[2][2];
  const double c20 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
  const double inv = 1.0 / (A[0][0] * c00 + A[0][1] * c10 + A[0][2] * c20);
  const double m00 = c00 * inv;
  const double m01 = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * inv;
  const double m02 = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * inv;
  const double m10 = c10 * inv;
  const double m11 = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * inv;
  const double m12 = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * inv;
  const double m20 = c20 * inv;
  const double m21 = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * inv;
  const double m22 = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * inv;
  double tx = R[0] * psx + R[1] * psy + R[2] * psz;
  double ty = R[3] * psx + R[4] * psy + R[5] * psz;
  double tz = R[6] * psx + R[7] * psy + R[8] * psz;
  tx += P.t[0]; ty += P.t[1]; tz += P.t[2];
  const double rx = ptx - tx, ry = pty - ty, rz = ptz - tz;
  const double dx = m00 * rx + m01 * ry + m02 * rz;
  const double dy = m10 * rx + m11 * ry + m12 * rz;
  const double dz = m20 * rx + m21 * ry + m22 * rz;
  o.r = rx * dx + ry * dy + rz * dz;
  o.detA = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
           A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

// GICPCostFunction::Probability as the reference uses it (gicp_cost_function.h:75-87 through em_icp.hpp:108):
// the density det(2 pi A)^-1/2 exp(-r/2), converted to bool (quirk Q1: 1 unless the product underflows to
// exactly 0; NaN -> 1).  pow() and exp() cost ~300 instructions to answer a question that is decided long
// before the last digit: with 1e-60 < det A < 1e30 (det of A = C_t + R C_s R^T is at most 8 for real inputs) the
// power lies in (6e-17, 6e28), so the product cannot be 0 for r < 1300 (exp(-650) = 5e-283: the product is above
// 3e-299, a normal number) and is exactly 0 for r > 1600 (exp(-800) is 0, below the smallest denormal, times a
// finite power).  The band between them -- and every determinant outside that range, NaN, Inf, det <= 0 -- takes
// the literal formula, so the decision is the reference's for every input.
__device__ __forceinline__ double geometric_gate(const Corr& c, int bool_probability) {
  const double two_pi = 6.283185307179586;
  if (bool_probability) {
    const bool sane = c.detA > 1e-60 && c.detA < 1e30;
    if (sane && c.r < 1300.0) return 1.0;
    if (sane && c.r > 1600.0) return 0.0;
    const double probability = pow(two_pi * two_pi * two_pi * c.detA, -0.5) * exp(-0.5 * c.r);
    return (probability != 0.0) ? 1.0 : 0.0;  // quirk Q1: double -> bool (NaN -> true)
  }
  return pow(two_pi * two_pi * two_pi * c.detA, -0.5) * exp(-0.5 * c.r);
}

// the geometric factor of one slot: the closed form decides the bool, the literal sequence gives the double.  LITERAL is a
// template parameter, not only a run-time flag: with both forms compiled in, the K = 4 packet search needs 66 VGPRs instead of
// 54 (8 -> 7 waves per SIMD) and em_weight_rows4_jobs_kernel 156 instead of 126 (4 -> 3), whichever form runs.  The launchers
// pick the LITERAL kernels only for handles with quirk_bool_probability = 0; every other launch runs the code it always ran.
// (A job launch takes them when any of its jobs is such a handle; em_weight_hist4_body, a developer switch, keeps the closed form.)
template <bool LITERAL>
__device__ __forceinline__ double slot_gate(const Pose& P, double one_m_eps, const PointRec& s, const PointRec& t, int bool_probability) {
  Corr c;
  if (LITERAL && !bool_probability) corr_eval_literal(P, one_m_eps, s.x, s.y, s.z, s.nx, s.ny, s.nz, t.x, t.y, t.z, t.nx, t.ny, t.nz, c);
  else corr_eval<false>(P, one_m_eps, s.x, s.y, s.z, s.nx, s.ny, s.nz, t.x, t.y, t.z, t.nx, t.ny, t.nz, c);
  return geometric_gate(c, bool_probability);
}

}  // namespace sicp
#endif
