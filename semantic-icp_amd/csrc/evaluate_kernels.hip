// evaluate_kernels.hip -- the reductions of sicp_evaluate (gfx950, wave64).
//
// The K = 1 searches have run: one per target segment, every one over ALL source points, into idx / d2 [n_seg][n_s] (a flat
// target has one segment, a SEMANTIC-mode target one per label).  Per source point:
//   merge     the segments' winners by (d^2, caller index) -- the order of the search itself, so the result is the nearest
//             neighbour in the whole target whatever the layout; a winner the search gated out carries index -1, and winners
//             of equal d^2 pass or fail the gate together
//   gate      the winner is an inlier when the search kept it (float d^2 < gate, strict)
//   counts    inliers, inliers of equal labels, inliers with a label outside 1..C; the confusion table
//   sum       the inliers' d^2 in double
//   scatter   the winner's caller index (-1: no inlier) and d^2 to the source point's caller index (optional)
//
//   evaluate_jobs           one lane per source point, kEvalChunksPerBlock chunks of kEvalChunk points per workgroup.  A chunk's
//                           counts (ballot + popcount per wave) and its sum (the fixed butterfly per wave, the four waves in
//                           order) become ONE row of partials: the chunk is the unit, not the workgroup, so the sums do not
//                           depend on how many chunks a workgroup walks.  Table counts go to a 32-bit copy in LDS (C <= 64;
//                           integer atomics: any order gives the same table) that the workgroup adds to the 64-bit table in
//                           HBM once, non-zero entries only; larger tables are counted in HBM directly.
//   evaluate_finalize_jobs  one wave per job: lane l adds the partials l, l + 64, ... in order, then the butterfly.
// No float atomics: a pair has the same bits alone, in any group of a batch and run after run.  Every result is written with
// plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SICP_HD __host__ __device__
#include "job_table.hpp"
#include "kernels.h"

namespace sicp {
namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#define SICP_GLOBAL __attribute__((address_space(1)))
#else
#define SICP_GLOBAL  // (the host pass only parses the kernels)
#endif
// a pointer read from a job record only ever holds device memory: global loads and stores instead of flat ones
template <class T>
__device__ __forceinline__ SICP_GLOBAL T* dev(T* p) {
  return (SICP_GLOBAL T*)p;
}

__global__ __launch_bounds__(256) void evaluate_jobs_kernel(const EvalJob* __restrict__ jobs, const int* __restrict__ blk_end, int nj) {
  __shared__ unsigned s_tab[kEvalLdsClasses * kEvalLdsClasses];
  __shared__ double s_sum[4];
  __shared__ int s_cnt[4][3];
  int lb;
  const EvalJob& J = jobs[job_of(blk_end, nj, blockIdx.x, &lb)];
  const int n_s = J.n_s, n_seg = J.n_seg, C = J.C;
  const float gate = J.gate_sq;
  const auto idx = dev(J.idx);
  const auto d2 = dev(J.d2);
  const auto slabel = dev(J.slabel);
  const auto tlabel = dev(J.tlabel);
  const auto sperm = dev(J.sperm);
  const auto tperm = dev(J.tperm);
  const auto nn_idx = dev(J.nn_idx);
  const auto nn_d2 = dev(J.nn_d2);
  const bool labels = J.slabel != nullptr && J.tlabel != nullptr;
  const bool table = J.conf != nullptr && labels && C > 0;
  const bool in_lds = table && C <= kEvalLdsClasses;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (in_lds) {
    for (int e = threadIdx.x; e < C * C; e += 256) s_tab[e] = 0u;
    __syncthreads();
  }
  const int chunks = eval_chunks(n_s);
  const int c_begin = lb * kEvalChunksPerBlock, c_end = min(c_begin + kEvalChunksPerBlock, chunks);
  for (int c = c_begin; c < c_end; ++c) {
    const int q = c * kEvalChunk + threadIdx.x;
    bool inlier = false, agree = false, outside = false;
    double v = 0.0;
    if (q < n_s) {
      float bd = d2[q];
      int bj = idx[q];
      int bc = bj >= 0 ? tperm[bj] : 0x7fffffff;
      for (int s = 1; s < n_seg; ++s) {
        const size_t o = (size_t)s * n_s + q;
        const float d = d2[o];
        const int j = idx[o];
        if (d < bd) {
          bd = d; bj = j;
          bc = j >= 0 ? tperm[j] : 0x7fffffff;
        } else if (d == bd && j >= 0) {
          const int cc = tperm[j];
          if (cc < bc) { bj = j; bc = cc; }
        }
      }
      inlier = bj >= 0 && bd < gate;
      if (inlier) {
        v = (double)bd;
        if (labels) {
          const uint32_t ls = slabel[q], lt = tlabel[bj];
          agree = ls == lt;
          if (table) {
            if (ls - 1u < (uint32_t)C && lt - 1u < (uint32_t)C) {
              const int e = (int)(ls - 1u) * C + (int)(lt - 1u);
              if (in_lds) atomicAdd(&s_tab[e], 1u);
              else atomicAdd((unsigned long long*)(J.conf + e), 1ull);
            } else {
              outside = true;
            }
          }
        }
      }
      if (J.nn_idx != nullptr || J.nn_d2 != nullptr) {
        const int o = sperm[q];
        if (J.nn_idx != nullptr) nn_idx[o] = inlier ? bc : -1;
        if (J.nn_d2 != nullptr) nn_d2[o] = bd;
      }
    }
    const int n_in = __popcll(__ballot(inlier)), n_ag = __popcll(__ballot(agree)), n_out = __popcll(__ballot(outside));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) {
      s_sum[wave] = v;
      s_cnt[wave][0] = n_in; s_cnt[wave][1] = n_ag; s_cnt[wave][2] = n_out;
    }
    __syncthreads();
    if (threadIdx.x == 0) dev(J.part_sum)[c] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    if (threadIdx.x < 4) {
      const int k = threadIdx.x;
      dev(J.part_cnt)[(size_t)c * 4 + k] = k < 3 ? (s_cnt[0][k] + s_cnt[1][k]) + (s_cnt[2][k] + s_cnt[3][k]) : 0;
    }
    __syncthreads();  // (the next chunk writes s_sum / s_cnt again; it also orders the table's LDS atomics before the flush)
  }
  if (in_lds) {
    for (int e = threadIdx.x; e < C * C; e += 256) {
      const unsigned cnt = s_tab[e];
      if (cnt) atomicAdd((unsigned long long*)(J.conf + e), (unsigned long long)cnt);
    }
  }
}

__global__ __launch_bounds__(64) void evaluate_finalize_jobs_kernel(const EvalJob* __restrict__ jobs) {
  const EvalJob& J = jobs[blockIdx.x];
  const int chunks = eval_chunks(J.n_s), lane = threadIdx.x;
  const auto part_sum = dev(J.part_sum);
  const auto part_cnt = dev(J.part_cnt);
  double v = 0.0;
  long long n_in = 0, n_ag = 0, n_out = 0;
  for (int c = lane; c < chunks; c += 64) {
    v += part_sum[c];
    n_in += part_cnt[(size_t)c * 4];
    n_ag += part_cnt[(size_t)c * 4 + 1];
    n_out += part_cnt[(size_t)c * 4 + 2];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    v += __shfl_xor(v, off, 64);
    n_in += __shfl_xor(n_in, off, 64);
    n_ag += __shfl_xor(n_ag, off, 64);
    n_out += __shfl_xor(n_out, off, 64);
  }
  if (lane == 0) {
    const auto out = dev(J.out);
    out->inliers = n_in; out->label_agree = n_ag; out->label_outside = n_out; out->sum_d2 = v;
  }
}

}  // namespace

hipError_t launch_evaluate_jobs(const EvalJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st) {
  if (nj <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(evaluate_jobs_kernel, dim3(blocks), dim3(256), 0, st, jobs, blk_end, nj);
  return hipGetLastError();
}

hipError_t launch_evaluate_finalize_jobs(const EvalJob* jobs, int nj, hipStream_t st) {
  if (nj <= 0) return hipSuccess;
  hipLaunchKernelGGL(evaluate_finalize_jobs_kernel, dim3(nj), dim3(64), 0, st, jobs);
  return hipGetLastError();
}

}  // namespace sicp
