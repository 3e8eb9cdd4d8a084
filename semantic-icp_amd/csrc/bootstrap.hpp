// bootstrap.hpp -- internal interface of the initial alignment without a pose prior (bootstrap.cpp; entry points in
// sicp_api.cpp).
#ifndef SICP_BOOTSTRAP_HPP_
#define SICP_BOOTSTRAP_HPP_

#include "engine.hpp"

namespace sicp {
namespace host {

constexpr int kBootMaxSamples = 8;  // nr_samples

// splitmix64 from `state`; index(n) = floor(n * u), u = (next() >> 11) * 2^-53: the hypothesis sequence is a pure function
// of the seed (tests/bootstrap_ref.py restates it)
struct BootRng {
  uint64_t state;
  uint64_t next();
  int index(int n);
};

void bootstrap_default_params(sicp_bootstrap_params* p);
int bootstrap_run(sicp_context* h, const sicp_bootstrap_params* p, double* out_qt, sicp_bootstrap_info* info);
// sicp_bootstrap_batch: checks its arguments, then runs every pair (status[i] per pair)
int bootstrap_batch(sicp_handle* hs, int32_t n, const sicp_bootstrap_params* p, double* out_qt, int32_t* status,
                    sicp_bootstrap_info* infos);
int bootstrap_keypoints(sicp_context* h, int which, const sicp_bootstrap_params* p, int32_t capacity, int64_t nbr_capacity,
                        int32_t* n_keypoints, int64_t* n_nbrs, float* xyz3, double* normal3, float* fpfh33,
                        int64_t* nbr_offsets, int32_t* nbr_idx);
int bootstrap_score(sicp_context* h, const sicp_bootstrap_params* p, int32_t n, const int32_t* src_idx, const int32_t* tgt_idx,
                    double* M12, double* err, int32_t knn_capacity, int32_t* feat_knn);

// the label forms (sicp_bootstrap_semantic*): the same stages with the label rules of lp ("Bootstrap")
void bootstrap_default_label_params(sicp_bootstrap_label_params* lp);
int bootstrap_semantic_run(sicp_context* h, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp, double* out_qt,
                           sicp_bootstrap_info* info);
int bootstrap_semantic_batch(sicp_handle* hs, int32_t n, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp,
                             double* out_qt, int32_t* status, sicp_bootstrap_info* infos);
int bootstrap_semantic_keypoints(sicp_context* h, int which, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp,
                                 int32_t capacity, int32_t* n_keypoints, float* xyz3, uint32_t* label);
int bootstrap_semantic_score(sicp_context* h, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp, int32_t n,
                             const int32_t* src_idx, const int32_t* tgt_idx, double* M12, double* err, int32_t knn_capacity,
                             int32_t* feat_knn);

}  // namespace host
}  // namespace sicp
#endif
