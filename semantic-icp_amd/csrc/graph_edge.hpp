// graph_edge.hpp -- one edge of the pose graph (sicp_graph_*; include/sicp.h), host + device: the residual, the inverse right
// Jacobian of SE(3), the adjoint, the loss and the edge's blocks of the normal equations.  One source for the kernels of
// graph_kernels.hip and for a host build that the CPU tests compile on its own.
//
// An edge (i, j, z, Omega) measures z ~ T_i^-1 T_j.  r = log(z^-1 T_i^-1 T_j), s = r^T Omega r, cost = 1/2 sum rho(s).  Under
// T <- T exp(delta), delta = [upsilon; omega] (se3.hpp's tangent), at both ends:
//     dr / d delta_j = Jr^-1(r),     dr / d delta_i = -Jr^-1(r) Ad(T_j^-1 T_i),     Ad_T = [[R, [t]x R], [0, R]].
// Jr^-1(xi) = Jl^-1(-xi), Jl = [[J, Q], [0, J]] (Barfoot, State Estimation for Robotics, 7.85-7.86), so
// Jl^-1 = [[J^-1, -J^-1 Q J^-1], [0, J^-1]] with J^-1 = I - Phi / 2 + c Phi^2.  Below theta = 0.25 every coefficient is its
// series in theta^2 to theta^10: the truncation is below 1e-18 relative there, and the closed forms' cancellation
// (eps / theta^4 relative on the last coefficient, which multiplies a theta^3 term) is at rounding level of the block above it.
#ifndef SICP_GRAPH_EDGE_HPP_
#define SICP_GRAPH_EDGE_HPP_

#include "lm.hpp"
#include "se3.hpp"

namespace sicp {
namespace graph {

enum { kLossNone = 0, kLossCauchy = 1 };
constexpr double kSeriesThetaSq = 0.0625;  // theta = 0.25

SICP_HD inline void hat(const double* v, double* M) {
  M[0] = 0;     M[1] = -v[2]; M[2] = v[1];
  M[3] = v[2];  M[4] = 0;     M[5] = -v[0];
  M[6] = -v[1]; M[7] = v[0];  M[8] = 0;
}

SICP_HD inline void mul3(const double* A, const double* B, double* C) {
  SICP_UNROLL
  for (int i = 0; i < 3; ++i)
    SICP_UNROLL
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// the four coefficients of Jl^-1: c of J^-1 = I - Phi / 2 + c Phi^2, and a1, a2, a3 of Q
SICP_HD inline void coefficients(double t2, double* c, double* a1, double* a2, double* a3) {
  if (t2 < kSeriesThetaSq) {
    *c = 1.0 / 12 + t2 * (1.0 / 720 + t2 * (1.0 / 30240 + t2 * (1.0 / 1209600 + t2 * (1.0 / 47900160 + t2 * (691.0 / 1307674368000.0)))));
    *a1 = 1.0 / 6 - t2 * (1.0 / 120 - t2 * (1.0 / 5040 - t2 * (1.0 / 362880 - t2 * (1.0 / 39916800 - t2 * (1.0 / 6227020800.0)))));
    *a2 = 1.0 / 24 - t2 * (1.0 / 720 - t2 * (1.0 / 40320 - t2 * (1.0 / 3628800 - t2 * (1.0 / 479001600 - t2 * (1.0 / 87178291200.0)))));
    *a3 = 1.0 / 120 - t2 * (2.0 / 5040 - t2 * (3.0 / 362880 - t2 * (4.0 / 39916800 - t2 * (5.0 / 6227020800.0 - t2 * (6.0 / 1307674368000.0)))));
  } else {
    const double t = sqrt(t2);
    double st, ct, sh, ch;
    se3::sincos_pair(t, &st, &ct);
    se3::sincos_pair(0.5 * t, &sh, &ch);
    *c = (1.0 - t * ch / (2.0 * sh)) / t2;
    *a1 = (t - st) / (t2 * t);
    *a2 = (t2 + 2.0 * ct - 2.0) / (2.0 * t2 * t2);
    *a3 = (2.0 * t - 3.0 * st + t * ct) / (2.0 * t2 * t2 * t);
  }
}

// Jl^-1(xi), row-major 6x6
SICP_HD inline void jl_inv(const double* xi, double* J) {
  const double* rho = xi;
  const double* phi = xi + 3;
  const double t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  double c, a1, a2, a3;
  coefficients(t2, &c, &a1, &a2, &a3);
  double F[9], P[9], FF[9], A[9];
  hat(phi, F);
  hat(rho, P);
  mul3(F, F, FF);
  SICP_UNROLL
  for (int k = 0; k < 9; ++k) A[k] = -0.5 * F[k] + c * FF[k];
  A[0] += 1; A[4] += 1; A[8] += 1;
  double FP[9], PF[9], FPF[9], FFP[9], PFF[9], FPFF[9], FFPF[9], Q[9];
  mul3(F, P, FP);
  mul3(P, F, PF);
  mul3(FP, F, FPF);
  mul3(F, FP, FFP);
  mul3(PF, F, PFF);
  mul3(FPF, F, FPFF);
  mul3(F, FPF, FFPF);
  SICP_UNROLL
  for (int k = 0; k < 9; ++k)
    Q[k] = 0.5 * P[k] + a1 * (FP[k] + PF[k] + FPF[k]) + a2 * (FFP[k] + PFF[k] - 3.0 * FPF[k]) + a3 * (FPFF[k] + FFPF[k]);
  double AQ[9], AQA[9];
  mul3(A, Q, AQ);
  mul3(AQ, A, AQA);
  SICP_UNROLL
  for (int i = 0; i < 3; ++i)
    SICP_UNROLL
    for (int j = 0; j < 3; ++j) {
      J[6 * i + j] = A[3 * i + j];
      J[6 * i + 3 + j] = -AQA[3 * i + j];
      J[6 * (i + 3) + j] = 0;
      J[6 * (i + 3) + 3 + j] = A[3 * i + j];
    }
}

// Jr^-1(xi) = Jl^-1(-xi)
SICP_HD inline void jr_inv(const double* xi, double* J) {
  double m[6];
  SICP_UNROLL
  for (int k = 0; k < 6; ++k) m[k] = -xi[k];
  jl_inv(m, J);
}

// Ad_T of qt = [q; t], row-major 6x6
SICP_HD inline void adjoint(const double* qt, double* A) {
  double R[9], T[9], TR[9];
  se3::rotation(qt, R);
  hat(qt + 4, T);
  mul3(T, R, TR);
  SICP_UNROLL
  for (int i = 0; i < 3; ++i)
    SICP_UNROLL
    for (int j = 0; j < 3; ++j) {
      A[6 * i + j] = R[3 * i + j];
      A[6 * i + 3 + j] = TR[3 * i + j];
      A[6 * (i + 3) + j] = 0;
      A[6 * (i + 3) + 3 + j] = R[3 * i + j];
    }
}

// r = log(z^-1 T_i^-1 T_j); Tji = T_j^-1 T_i (what the adjoint of node i's Jacobian takes)
SICP_HD inline void residual(const double* Ti, const double* Tj, const double* z, double* r, double* Tji) {
  double inv[7], Tij[7], E[7];
  se3::inverse(Ti, inv);
  se3::mul(inv, Tj, Tij);
  se3::inverse(z, inv);
  se3::mul(inv, Tij, E);
  se3::log(E, r);
  se3::inverse(Tij, Tji);
}

SICP_HD inline double chi2(const double* r, const double* Omega, double* Or) {
  double s = 0;
  SICP_UNROLL
  for (int a = 0; a < 6; ++a) {
    double t = 0;
    SICP_UNROLL
    for (int b = 0; b < 6; ++b) t += Omega[6 * a + b] * r[b];
    Or[a] = t;
    s += r[a] * t;
  }
  return s;
}

// rho(s) and the IRLS weight w = rho'(s) (no second-order corrector)
SICP_HD inline void loss(int kind, double a, double s, double* rho, double* w) {
  if (kind == kLossCauchy) {
    const double a2 = a * a, q = 1.0 + s / a2;
    *rho = a2 * log(q);
    *w = 1.0 / q;
  } else {
    *rho = s;
    *w = 1.0;
  }
}

// C = w A^T B, row-major 6x6
SICP_HD inline void atb6(const double* A, const double* B, double w, double* C) {
  SICP_UNROLL
  for (int a = 0; a < 6; ++a)
    SICP_UNROLL
    for (int b = 0; b < 6; ++b) {
      double t = 0;
      SICP_UNROLL
      for (int k = 0; k < 6; ++k) t += A[6 * k + a] * B[6 * k + b];
      C[6 * a + b] = w * t;
    }
}
// the same for a product that is symmetric: the upper triangle is computed and mirrored
SICP_HD inline void atb6_sym(const double* A, const double* B, double w, double* C) {
  SICP_UNROLL
  for (int a = 0; a < 6; ++a)
    SICP_UNROLL
    for (int b = a; b < 6; ++b) {
      double t = 0;
      SICP_UNROLL
      for (int k = 0; k < 6; ++k) t += A[6 * k + a] * B[6 * k + b];
      C[6 * a + b] = w * t;
      C[6 * b + a] = w * t;
    }
}
SICP_HD inline void atv6(const double* A, const double* v, double w, double* o) {
  SICP_UNROLL
  for (int a = 0; a < 6; ++a) {
    double t = 0;
    SICP_UNROLL
    for (int k = 0; k < 6; ++k) t += A[6 * k + a] * v[k];
    o[a] = w * t;
  }
}
SICP_HD inline void mul6(const double* A, const double* B, double sign, double* C) {
  SICP_UNROLL
  for (int a = 0; a < 6; ++a)
    SICP_UNROLL
    for (int b = 0; b < 6; ++b) {
      double t = 0;
      SICP_UNROLL
      for (int k = 0; k < 6; ++k) t += A[6 * a + k] * B[6 * k + b];
      C[6 * a + b] = sign * t;
    }
}

// residual, chi2 and loss of an edge at the poses of its ends; Tji as residual()
SICP_HD inline void edge_error(const double* Ti, const double* Tj, const double* z, const double* Omega, int loss_kind, double cauchy_a,
                               double* r, double* Or, double* s, double* w, double* rho, double* Tji) {
  residual(Ti, Tj, z, r, Tji);
  *s = chi2(r, Omega, Or);
  loss(loss_kind, cauchy_a, *s, rho, w);
}

// The blocks of an edge: Hi = Ji^T w Omega Ji and gi = Ji^T w Omega r go to Ci[0 .. 36) and Ci[36 .. 42), node j's to Cj, the
// one off-diagonal block Ji^T w Omega Jj to B.  Or = Omega r.  Ordered so that few 6x6 arrays are alive at a time: one lane of
// the linearise kernel holds them in registers.
SICP_HD inline void edge_blocks(const double* r, const double* Or, const double* Omega, double w, const double* Tji, double* Ci, double* Cj,
                                double* B) {
  double Jj[36], M[36];
  jr_inv(r, Jj);
  mul6(Omega, Jj, 1.0, M);  // Omega Jj
  atb6_sym(Jj, M, w, Cj);
  atv6(Jj, Or, w, Cj + 36);
  double Ad[36], Ji[36];
  adjoint(Tji, Ad);
  mul6(Jj, Ad, -1.0, Ji);
  atb6(Ji, M, w, B);
  atv6(Ji, Or, w, Ci + 36);
  double N[36];
  mul6(Omega, Ji, 1.0, N);  // Omega Ji
  atb6_sym(Ji, N, w, Ci);
}

}  // namespace graph
}  // namespace sicp
#endif
