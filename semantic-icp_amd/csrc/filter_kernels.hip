// filter_kernels.hip -- sicp_filter: statistical / radius outlier removal and masked selection of one cloud (driver: filter.cpp;
// the rules: include/sicp.h, "filtering a cloud").  The cloud's own exact k-NN search (run_nn) has written every query's
// ascending list of float32 squared distances; here a lane per query turns it into the mean distance m, a binary tree of fixed
// shape over the caller's indices sums m and m m, the cluster's sorted cell grid counts the neighbours inside the radius, and a
// flag per point, its scan and a gather write the kept cloud.  Integer atomics count; no floating-point atomics; every byte is
// independent of the launch shapes.
#include <hip/hip_runtime.h>

#include "cell_grid.hpp"
#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

__device__ __forceinline__ int caller_of(const FilterArgs& a, int f) { return a.caller ? a.caller[f] : f; }

// rule 1.  Every caller index gets its defaults -- not kept, no mean distance, no count -- and every finite point its class.
__global__ __launch_bounds__(256) void filter_class_kernel(FilterArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_caller) {
    a.okeep[i] = 0;
    a.omd[i] = __longlong_as_double(0x7ff8000000000000ll);
    a.onb[i] = -1;
  }
  int cls = kFlRemoved;
  if (i < a.n) {
    bool dropped = a.mask != nullptr && a.mask[caller_of(a, i)] == 0, prot = false;
    if (a.labels) {
      const uint32_t l = a.label[i];
      for (int k = 0; k < a.n_drop; ++k) dropped = dropped || a.drop[k] == l;
      for (int k = 0; k < a.n_protect; ++k) prot = prot || a.protect[k] == l;
    }
    cls = dropped ? kFlRemoved : prot ? kFlProtect : kFlTest;
    a.cls[i] = (uint8_t)cls;
  }
  const int tested = __popcll(__ballot(cls == kFlTest)), prots = __popcll(__ballot(cls == kFlProtect));
  if ((threadIdx.x & 63) == 0) {
    if (tested) atomicAdd(a.res + kFlTested, tested);
    if (prots) atomicAdd(a.res + kFlProtected, prots);
  }
}

// rule 10: the list_k smallest values of two ascending lists, into the first, by a lane per query.  A forward pass over both
// counts how many the first list gives; the backward merge then writes position k from a position <= k of the first list, so
// nothing is overwritten before it is read.  Only values are merged: equal values need no order.
__global__ __launch_bounds__(256) void filter_merge_lists_kernel(FilterArgs a) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= a.n) return;
  const int K = a.list_k;
  float* A = a.list + (size_t)q * K;
  const float* B = a.list2 + (size_t)q * K;
  int ia = 0, ib = 0;
  for (int k = 0; k < K; ++k) {
    if (B[ib] < A[ia]) ++ib; else ++ia;  // (ia + ib = k < K: both in range)
  }
  --ia; --ib;
  for (int k = K - 1; k >= 0; --k) {
    const bool from_b = ib >= 0 && (ia < 0 || B[ib] > A[ia]);
    A[k] = from_b ? B[ib] : A[ia];
    if (from_b) --ib; else --ia;
  }
}

// rule 3: m = (sum of (double)sqrtf(d2_j), ascending, the first entry -- the point itself -- left out) / (double)mean_k, written
// at the caller's index.  (float)sqrt((double)d2) is the correctly rounded float root: a double root of a float rounds once
// more without changing the result.
__global__ __launch_bounds__(256) void filter_mean_dist_kernel(FilterArgs a) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= a.n) return;
  const int f = a.perm[q];
  if (a.cls[f] != kFlTest) return;
  const float* L = a.list + (size_t)q * a.list_k;
  double s = 0.0;
  for (int k = 1; k < a.list_k; ++k) s = __dadd_rn(s, (double)(float)__dsqrt_rn((double)L[k]));
  a.omd[caller_of(a, f)] = __ddiv_rn(s, (double)a.mean_k);
}

// rule 3, the sums: one workgroup reduces an aligned run of kFilterTreeRun entries as the perfect binary tree over them,
// s[j] = s[2 j] + s[2 j + 1] level by level; entries past `count` are +0.0.  The same kernel over the partial sums continues the
// tree, so the result is the sum over the perfect tree on 2^ceil(log2 n) leaves (a subtree of zeros adds +0.0 to a non-negative
// sum: nothing) whatever the launch.
__global__ __launch_bounds__(256) void filter_tree_sum_kernel(const double* in1, const double* in2, int count, int first, double* out1,
                                                              double* out2) {
  static_assert(kFilterTreeRun == 512, "two entries per lane of a 256-lane workgroup");
  __shared__ double s1[256], s2[256];
  const int t = threadIdx.x;
  const long long base = (long long)blockIdx.x * kFilterTreeRun + 2 * t;
  double v1[2], v2[2];
  for (int k = 0; k < 2; ++k) {
    v1[k] = 0.0; v2[k] = 0.0;
    if (base + k < count) {
      const double m = in1[base + k];
      if (first) {
        if (m == m) { v1[k] = m; v2[k] = __dmul_rn(m, m); }
      } else {
        v1[k] = m; v2[k] = in2[base + k];
      }
    }
  }
  s1[t] = __dadd_rn(v1[0], v1[1]);
  s2[t] = __dadd_rn(v2[0], v2[1]);
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    double p1 = 0.0, p2 = 0.0;
    if (t < w) { p1 = __dadd_rn(s1[2 * t], s1[2 * t + 1]); p2 = __dadd_rn(s2[2 * t], s2[2 * t + 1]); }
    __syncthreads();
    if (t < w) { s1[t] = p1; s2[t] = p2; }
    __syncthreads();
  }
  if (t == 0) { out1[blockIdx.x] = s1[0]; out2[blockIdx.x] = s2[0]; }
}

// rule 3, the threshold: double operations, each rounded on its own
__global__ void filter_threshold_kernel(FilterArgs a, const double* s1, const double* s2) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double S1 = s1[0], S2 = s2[0], nt = (double)a.res[kFlTested];
  const double mean = __ddiv_rn(S1, nt);
  const double v = __ddiv_rn(__dsub_rn(S2, __ddiv_rn(__dmul_rn(S1, S1), nt)), __dsub_rn(nt, 1.0));
  const double var = v > 0.0 ? v : 0.0;
  const double sd = __dsqrt_rn(var);
  FilterStats r;
  r.s1 = S1; r.s2 = S2; r.mean = mean; r.stddev = sd;
  r.threshold = __dadd_rn(mean, __dmul_rn(a.std_mul, sd));
  *a.stats = r;
}

// rule 4.  One workgroup per cell and 256 x gridDim.y of its points, as in the cluster's pair pass; here every point looks both
// ways, so the 27 cells are nine runs of consecutive sorted positions -- the cells x - 1 .. x + 1 of the rows (y + dy, z + dz) --
// whose eighteen ends eighteen lanes find by binary search in the cell keys.  The runs stream through LDS in tiles of 256; a lane
// counts the tile entries other than itself with d2 < r2 and leaves when it has min_neighbors; a wave's loop over a tile ends
// when its last lane has left, and the workgroup leaves the chunk when no lane is counting any more.  Only integers are produced.
__global__ __launch_bounds__(256) void filter_radius_kernel(FilterArgs a) {
  __shared__ float4 tile[256];
  __shared__ int run_b[9], run_e[9];
  const int n_cells = a.grid_res[kClCells];
  const int c = blockIdx.x;
  if (c >= n_cells) return;
  const int b = a.heads[c], e = a.heads[c + 1];
  const int first = b + 256 * (int)blockIdx.y, stride = 256 * (int)gridDim.y;
  if (first >= e) return;
  if (threadIdx.x < 18) {  // lanes 0..8: where run r begins; lanes 9..17: where it ends
    const int r = (int)threadIdx.x % 9;
    const bool end = threadIdx.x >= 9;
    // (unsigned arithmetic: a step to the row or plane below is the two's complement of the step up; a biased coordinate
    // lies in 2 .. 2^21 - 2, so x - 1, y - 1, z - 1 borrow nothing and x + 2 compares above every cell of its row)
    const u64 mid = a.ckey[c] + (u64)(long long)(r / 3 - 1) * kCellPlane + (u64)(long long)(r % 3 - 1) * kCellRow;
    const int at = a.heads[lower_bound_key(a.ckey, 0, n_cells, end ? mid + 2 : mid - 1)];
    if (end) run_e[r] = at; else run_b[r] = at;
  }
  __syncthreads();
  for (int p0 = first; p0 < e; p0 += stride) {
    const int my = p0 + (int)threadIdx.x;
    float4 P = make_float4(0.f, 0.f, 0.f, 0.f);
    int pi = 0, cnt = 0;
    bool tested = false;
    if (my < e) {
      pi = a.sval[my];
      tested = a.cls[pi] == kFlTest;
      P = a.spt[my];
    }
    bool counting = tested;
    bool live = true;  // (uniform over the workgroup)
    for (int r = 0; r < 9 && live; ++r) {
      const int rb = run_b[r], re = run_e[r];
      for (int t0 = rb; t0 < re; t0 += 256) {
        // (the barrier also ends the reads of the previous tile)
        if (!__syncthreads_or(counting ? 1 : 0)) { live = false; break; }
        const int len = min(256, re - t0);
        if ((int)threadIdx.x < len) tile[threadIdx.x] = a.spt[t0 + (int)threadIdx.x];
        __syncthreads();
        if (counting) {
          for (int k = 0; k < len; ++k) {
            if (t0 + k == my) continue;
            const float4 Q = tile[k];
            const float dx = __fsub_rn(P.x, Q.x), dy = __fsub_rn(P.y, Q.y), dz = __fsub_rn(P.z, Q.z);
            float d2 = __fmul_rn(dx, dx);
            d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
            d2 = __fadd_rn(d2, __fmul_rn(dz, dz));
            if (d2 < a.r2 && ++cnt >= a.min_neighbors) { counting = false; break; }
          }
        }
      }
    }
    if (tested) a.nb[pi] = cnt;
  }
}

// rules 5 and 6: the kept flag of every finite point, the per-point outputs at the caller's index, the failures counted
__global__ __launch_bounds__(256) void filter_flag_kernel(FilterArgs a) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  bool fail_stat = false, fail_radius = false;
  if (f < a.n) {
    const int cls = a.cls[f], ci = caller_of(a, f);
    bool keep = cls != kFlRemoved;
    if (cls == kFlTest) {
      if (a.mean_k > 0) fail_stat = !(a.omd[ci] <= a.stats->threshold);
      if (a.min_neighbors > 0) {
        const int c = a.nb[f];
        fail_radius = c < a.min_neighbors;
        a.onb[ci] = c;
      }
      keep = !fail_stat && !fail_radius;
    }
    a.flag[f] = keep ? 1 : 0;
    a.okeep[ci] = keep ? 1 : 0;
  }
  const int fs = __popcll(__ballot(fail_stat)), fr = __popcll(__ballot(fail_radius));
  if ((threadIdx.x & 63) == 0) {
    if (fs) atomicAdd(a.res + kFlFailStat, fs);
    if (fr) atomicAdd(a.res + kFlFailRadius, fr);
  }
}

// rule 8: the kept points in ascending caller index (f ascends with it)
__global__ __launch_bounds__(256) void filter_gather_kernel(FilterArgs a) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.n) return;
  const int keep = a.flag[f], p = a.pos[f];
  if (keep) {
    a.ox[p] = a.x[f]; a.oy[p] = a.y[f]; a.oz[p] = a.z[f];
    if (a.labels) a.ol[p] = a.label[f];
  }
  if (f == a.n - 1) a.res[kFlKept] = p + keep;
}

inline dim3 grid256(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_filter_classes(const FilterArgs& a, hipStream_t st) {
  const int m = a.n > a.n_caller ? a.n : a.n_caller;
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(filter_class_kernel, grid256(m), dim3(256), 0, st, a);
  return hipGetLastError();
}

#define SICP_FILTER_LAUNCH(fn, kernel)                                         \
  hipError_t fn(const FilterArgs& a, hipStream_t st) {                         \
    if (a.n <= 0) return hipSuccess;                                           \
    hipLaunchKernelGGL(kernel, grid256(a.n), dim3(256), 0, st, a);             \
    return hipGetLastError();                                                  \
  }
SICP_FILTER_LAUNCH(launch_filter_merge_lists, filter_merge_lists_kernel)
SICP_FILTER_LAUNCH(launch_filter_mean_dist, filter_mean_dist_kernel)
SICP_FILTER_LAUNCH(launch_filter_flags, filter_flag_kernel)
SICP_FILTER_LAUNCH(launch_filter_gather, filter_gather_kernel)
#undef SICP_FILTER_LAUNCH

hipError_t launch_filter_tree_sum(const double* in1, const double* in2, int count, int first, double* out1, double* out2, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)(((long long)count + kFilterTreeRun - 1) / kFilterTreeRun);
  hipLaunchKernelGGL(filter_tree_sum_kernel, dim3(blocks), dim3(256), 0, st, in1, in2, count, first, out1, out2);
  return hipGetLastError();
}

hipError_t launch_filter_threshold(const FilterArgs& a, const double* s1, const double* s2, hipStream_t st) {
  hipLaunchKernelGGL(filter_threshold_kernel, dim3(1), dim3(64), 0, st, a, s1, s2);
  return hipGetLastError();
}

// the cell count stays on the device, as in the cluster's pair pass: one row of workgroups per point bounds it
constexpr int kCountChunkGroups = 8;
hipError_t launch_filter_radius_count(const FilterArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(filter_radius_kernel, dim3((unsigned)a.n, kCountChunkGroups), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sicp
