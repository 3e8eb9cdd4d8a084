// graph_prior.hpp -- one prior of the pose graph (sicp_graph_add_priors; include/sicp.h), host + device, beside graph_edge.hpp:
// the residual, the loss and the prior's block of the normal equations.  One source for the prior kernel of graph_kernels.hip
// and for a host build that the CPU tests compile on its own.
//
// A pose prior (k, z, Omega) measures z ~ T_k: r = log(z^-1 T_k) in the tangent of z exp(delta), s = r^T Omega r.  Under
// T_k <- T_k exp(delta): dr / d delta_k = Jr^-1(r).  It is node j's half of an edge (i, k, z, Omega) whose node i stands at
// the identity, so its record is that edge's Cj.
// A position prior (k, p, Omega3) measures p ~ t_k in the world frame: r = t_k - p, s = r^T Omega3 r.  t' = t + R V(omega)
// upsilon under T exp(delta), so dr / d delta_k = [R_k | 0] exactly: the block is w [[R^T Omega3 R, 0], [0, 0]], the gradient
// w [R^T Omega3 r; 0].
#ifndef SICP_GRAPH_PRIOR_HPP_
#define SICP_GRAPH_PRIOR_HPP_

#include "graph_edge.hpp"

namespace sicp {
namespace graph {

enum { kPriorPose = 0, kPriorPosition = 1 };

// residual, chi2 and loss of a pose prior at the node's pose; Or = Omega r
SICP_HD inline void prior_pose_error(const double* Tk, const double* z, const double* Omega, int loss_kind, double cauchy_a, double* r,
                                     double* Or, double* s, double* w, double* rho) {
  double inv[7], E[7];
  se3::inverse(z, inv);
  se3::mul(inv, Tk, E);
  se3::log(E, r);
  *s = chi2(r, Omega, Or);
  loss(loss_kind, cauchy_a, *s, rho, w);
}

// C[0 .. 36) = w J^T Omega J, C[36 .. 42) = w J^T Omega r with J = Jr^-1(r): edge_blocks' Cj
SICP_HD inline void prior_pose_blocks(const double* r, const double* Or, const double* Omega, double w, double* C) {
  double J[36], M[36];
  jr_inv(r, J);
  mul6(Omega, J, 1.0, M);  // Omega J
  atb6_sym(J, M, w, C);
  atv6(J, Or, w, C + 36);
}

// r[0 .. 3) = t_k - p, r[3 .. 6) = 0; Or = Omega3 r (3 entries)
SICP_HD inline void prior_position_error(const double* Tk, const double* p, const double* Omega3, int loss_kind, double cauchy_a, double* r,
                                         double* Or, double* s, double* w, double* rho) {
  SICP_UNROLL
  for (int k = 0; k < 3; ++k) { r[k] = Tk[4 + k] - p[k]; r[3 + k] = 0.0; }
  double c = 0;
  SICP_UNROLL
  for (int a = 0; a < 3; ++a) {
    double t = 0;
    SICP_UNROLL
    for (int b = 0; b < 3; ++b) t += Omega3[3 * a + b] * r[b];
    Or[a] = t;
    c += r[a] * t;
  }
  *s = c;
  loss(loss_kind, cauchy_a, *s, rho, w);
}

// C[0 .. 36) = w [[R^T Omega3 R, 0], [0, 0]] (the upper triangle computed and mirrored), C[36 .. 42) = w [R^T Omega3 r; 0]
SICP_HD inline void prior_position_blocks(const double* Tk, const double* Or, const double* Omega3, double w, double* C) {
  double R[9], M[9];
  se3::rotation(Tk, R);
  mul3(Omega3, R, M);  // Omega3 R
  SICP_UNROLL
  for (int k = 0; k < 42; ++k) C[k] = 0.0;
  SICP_UNROLL
  for (int a = 0; a < 3; ++a) {
    SICP_UNROLL
    for (int b = a; b < 3; ++b) {
      double t = 0;
      SICP_UNROLL
      for (int k = 0; k < 3; ++k) t += R[3 * k + a] * M[3 * k + b];
      C[6 * a + b] = w * t;
      C[6 * b + a] = w * t;
    }
    double t = 0;
    SICP_UNROLL
    for (int k = 0; k < 3; ++k) t += R[3 * k + a] * Or[k];
    C[36 + a] = w * t;
  }
}

}  // namespace graph
}  // namespace sicp
#endif
