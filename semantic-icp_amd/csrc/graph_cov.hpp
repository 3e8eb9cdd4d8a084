// graph_cov.hpp -- the Jacobian of a relative pose (sicp_graph_relative_covariances; include/sicp.h), host + device.  One source
// for graph_cov_kernels.hip and for a host build that the CPU tests compile on its own, as graph_edge.hpp.
//
// z = T_a^-1 T_b under z exp(delta_z), the nodes under T <- T exp(delta).  To first order
//     delta_z = delta_b - Ad(T_b^-1 T_a) delta_a,
// so J has the block J_a = -Ad(T_b^-1 T_a) at node a and the identity at node b.
#ifndef SICP_GRAPH_COV_HPP_
#define SICP_GRAPH_COV_HPP_

#include "graph_edge.hpp"

namespace sicp {
namespace graph {

// J_a = -Ad(T_b^-1 T_a), row-major 6x6
SICP_HD inline void relative_jacobian_a(const double* Ta, const double* Tb, double* Ja) {
  double inv[7], Tba[7];
  se3::inverse(Tb, inv);
  se3::mul(inv, Ta, Tba);
  adjoint(Tba, Ja);
  SICP_UNROLL
  for (int k = 0; k < 36; ++k) Ja[k] = -Ja[k];
}

}  // namespace graph
}  // namespace sicp
#endif
