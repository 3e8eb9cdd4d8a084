// cluster_kernels.hip -- sicp_cluster: label-aware Euclidean clustering of one cloud (driver: cluster.cpp; the rules:
// include/sicp.h, "objects of a labelled cloud").  A cell grid finds the close pairs; a union-find over the point indices in HBM
// -- path halving, the larger root hooked under the smaller by an integer compare-and-swap -- joins them, so that a component's
// final root is its smallest index whatever order the pairs arrive in; integer atomics size the components; a scan over the
// roots in index order numbers the clusters; a sort by (cluster, index) feeds one wave per cluster with the members in the
// order the centroid's float64 sums are specified in.  No floating-point atomics, no grid-wide barrier.
#include <hip/hip_runtime.h>

#include "cell_grid.hpp"  // the cells, their keys and the proof that neighbouring cells hold every joined pair
#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

__device__ __forceinline__ bool cluster_ignored(const ClusterArgs& a, uint32_t l) {
  bool ig = false;
  for (int k = 0; k < a.n_ignore; ++k) ig = ig || a.ignore[k] == l;
  return ig;
}

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// parent[x] <= x always (a root is only ever hooked under a smaller root; halving stores an ancestor), so every walk descends
// and ends; a store to parent[x] never meets a hook of x, which needs parent[x] == x
__device__ __forceinline__ int uf_find(int* parent, int x) {
  for (;;) {
    const int p = ld(parent + x);
    if (p == x) return x;
    const int g = ld(parent + p);
    if (g == p) return p;
    st(parent + x, g);
    x = g;
  }
}

// joins the sets of a and b; returns their root as far as this lane has seen it
__device__ __forceinline__ int uf_union(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return a;
    const int lo = min(a, b), hi = max(a, b);
    const int old = atomicCAS(parent + hi, hi, lo);  // agent scope
    if (old == hi) return lo;
    a = lo; b = old;  // hi was hooked elsewhere meanwhile: go on from where it hangs now
  }
}

__global__ __launch_bounds__(256) void cluster_key_kernel(ClusterArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  u64 k = kNone;
  const bool vertex = !(a.labels && cluster_ignored(a, a.label[i]));
  if (vertex) {
    int cx, cy, cz;
    if (cluster_cell(a.x[i], a.inv, &cx) && cluster_cell(a.y[i], a.inv, &cy) && cluster_cell(a.z[i], a.inv, &cz))
      k = cell_key(cx, cy, cz);
    else
      a.res[kClRange] = 1;  // (a plain store: every writer stores the same 1)
  }
  a.key[i] = k;
  a.val[i] = i;
  a.parent[i] = vertex ? i : -1;
  a.size[i] = 0;
}

__global__ __launch_bounds__(256) void cluster_cell_flag_kernel(ClusterArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const u64 k = a.skey[j];
  a.flag[j] = (k != kNone && (j == 0 || k != a.skey[j - 1])) ? 1 : 0;
}

// the vertices once into sorted order (x, y, z, label bits: one 16-byte load per point in the pair pass), the first position and
// the key of every cell, the counts
__global__ __launch_bounds__(256) void cluster_cells_kernel(ClusterArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const u64 k = a.skey[j];
  const int f = a.flag[j], p = a.pos[j];
  if (k != kNone) {
    const int i = a.sval[j];
    a.spt[j] = make_float4(a.x[i], a.y[i], a.z[i], __uint_as_float(a.labels ? a.label[i] : 0u));
    if (f) { a.heads[p] = j; a.ckey[p] = k; }
    if (j == a.n - 1 || a.skey[j + 1] == kNone) {
      a.res[kClKept] = j + 1;
      a.res[kClCells] = p + f;
      a.heads[p + f] = j + 1;
    }
  }
}

// One workgroup per cell and 256 x gridDim.y of its points (blockIdx.y takes every gridDim.y-th chunk of 256, so that a dense
// cell is not one workgroup's work; most cells have one chunk and the other workgroups leave at once).  With keys ascending in (z, y, x), the cell and its 13 forward neighbours are five runs of consecutive
// sorted positions: {self, x + 1}, the three cells of row y + 1, and the three rows of plane z + 1 -- their ten ends found by
// ten lanes' binary searches in the cell keys, from the own cell on.  The workgroup takes its own points 256 at a time, one per lane, and
// streams the runs through LDS in tiles of 256; a lane tests its point against every tile entry at a later sorted position (all
// forward cells lie behind the own cell, so this is every pair once) by the arithmetic of rule 2.  A tile entry carries the
// root its point had when the tile was loaded (the finds of a tile run side by side, one per lane); a hit whose two ancestors
// are equal costs no memory access -- in a dense cell nearly every pair is already joined -- and only the others go to HBM.
__global__ __launch_bounds__(256) void cluster_pair_kernel(ClusterArgs a) {
  __shared__ float4 tile[256];
  __shared__ int tidx[256], troot[256];
  __shared__ int run_b[5], run_e[5];
  const int n_cells = a.res[kClCells];
  const int c = blockIdx.x;
  if (c >= n_cells) return;
  const int b = a.heads[c], e = a.heads[c + 1];
  const int first = b + 256 * (int)blockIdx.y, stride = 256 * (int)gridDim.y;  // a dense cell's chunks go round gridDim.y workgroups
  if (first >= e) return;
  if (threadIdx.x < 10) {  // lanes 0..4: where run r begins; lanes 5..9: where it ends
    const u64 key = a.ckey[c];
    const u64 row = 1ull << 21, plane = 1ull << 42;
    const u64 lo[5] = {key, key + row - 1, key + plane - row - 1, key + plane - 1, key + plane + row - 1};
    const u64 hi[5] = {key + 1, key + row + 1, key + plane - row + 1, key + plane + 1, key + plane + row + 1};
    const int r = (int)threadIdx.x % 5;
    const bool end = threadIdx.x >= 5;
    const int at = a.heads[lower_bound_key(a.ckey, c, n_cells, end ? hi[r] + 1 : lo[r])];
    if (end) run_e[r] = at; else run_b[r] = at;
  }
  __syncthreads();
  for (int p0 = first; p0 < e; p0 += stride) {
    const int my = p0 + (int)threadIdx.x;
    const bool have = my < e;
    float4 P = make_float4(0.f, 0.f, 0.f, 0.f);
    int pi = 0, root = 0;
    if (have) {
      P = a.spt[my];
      pi = a.sval[my];
      root = uf_find(a.parent, pi);
    }
    const unsigned pl = __float_as_uint(P.w);
    for (int r = 0; r < 5; ++r) {
      const int rb = r == 0 ? p0 : run_b[r], re = run_e[r];  // (run 0 begins at the own cell: what lies before p0 is done)
      for (int t0 = rb; t0 < re; t0 += 256) {
        const int cnt = min(256, re - t0);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
          const int qi = a.sval[t0 + (int)threadIdx.x];
          tile[threadIdx.x] = a.spt[t0 + (int)threadIdx.x];
          tidx[threadIdx.x] = qi;
          troot[threadIdx.x] = uf_find(a.parent, qi);
        }
        __syncthreads();
        if (!have) continue;
        for (int k = max(0, my + 1 - t0); k < cnt; ++k) {
          const float4 Q = tile[k];
          if (a.same_label && __float_as_uint(Q.w) != pl) continue;
          const float dx = __fsub_rn(P.x, Q.x), dy = __fsub_rn(P.y, Q.y), dz = __fsub_rn(P.z, Q.z);
          float d2 = __fmul_rn(dx, dx);
          d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
          d2 = __fadd_rn(d2, __fmul_rn(dz, dz));
          if (!(d2 < a.t2)) continue;
          if (troot[k] == root) continue;  // a common ancestor, whether or not it is still a root: one component already
          root = uf_union(a.parent, pi, tidx[k]);
          troot[k] = root;  // (an ancestor of q whichever lane's store lands)
        }
      }
    }
  }
}

// the flatten pass and the component sizes: every vertex learns its root (the walk only reads, the store is the vertex's own
// slot, and whoever still walks through it finds the old ancestor or the root) and counts itself there
__global__ __launch_bounds__(256) void cluster_size_kernel(ClusterArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  int r = ld(a.parent + i);
  if (r < 0) return;
  for (int p = ld(a.parent + r); p != r; p = ld(a.parent + r)) r = p;
  st(a.parent + i, r);
  atomicAdd(a.size + r, 1);
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int w = 32; w > 0; w >>= 1) v = max(v, __shfl_xor(v, w, 64));
  return v;
}

// a root whose size lies in the bounds opens a cluster; the integer totals
__global__ __launch_bounds__(256) void cluster_root_flag_kernel(ClusterArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int root = 0, s = 0, f = 0;
  if (i < a.n) {
    root = a.parent[i] == i ? 1 : 0;
    s = root ? a.size[i] : 0;
    f = (root && s >= a.min_points && s <= a.max_points) ? 1 : 0;
    a.flag[i] = f;
  }
  const int comps = wave_sum(root), pts = wave_sum(f ? s : 0), big = wave_max(f ? s : 0);
  if ((threadIdx.x & 63) == 0) {
    if (comps) atomicAdd(a.res + kClComponents, comps);
    if (pts) atomicAdd(a.res + kClClustered, pts);
    if (big) atomicMax(a.res + kClMaxCount, big);
  }
}

__global__ __launch_bounds__(256) void cluster_id_kernel(ClusterArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int r = a.parent[i];
  const int c = (r >= 0 && a.flag[r]) ? a.pos[r] : -1;
  a.cid[i] = c;
  a.mkey[i] = c >= 0 ? (((u64)(unsigned)c << 32) | (u64)(unsigned)i) : kNone;
  if (a.lkey) a.lkey[i] = c >= 0 ? (((u64)(unsigned)c << 32) | (u64)a.label[i]) : kNone;
  if (i == a.n - 1) a.res[kClClusters] = a.pos[i] + a.flag[i];
}

__global__ __launch_bounds__(256) void cluster_member_head_kernel(ClusterArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const u64 k = a.msorted[j];
  if (k == kNone) return;
  const int c = (int)(k >> 32);
  if (j == 0 || (int)(a.msorted[j - 1] >> 32) != c) a.mheads[c] = j;
  if (j == a.n - 1 || a.msorted[j + 1] == kNone) a.mheads[c + 1] = j + 1;
}

// One wave per cluster.  The members arrive 64 at a time in ascending index (coalesced index loads, gathered coordinates) and go
// through LDS to lanes 0, 1, 2, which add their axis in that order in float64 -- the order is the specification, so the sum of a
// long cluster is serial; every lane keeps the extremes of what it loaded for the box.  The label: the members' own with
// same_label, else the longest run of equal labels in the cluster's range of the (cluster, label) sort -- ascending labels, so
// the first of equal runs is the smallest.
__global__ __launch_bounds__(64) void cluster_table_kernel(ClusterArgs a, int n_clusters) {
  __shared__ float t[3][64];
  const int c = blockIdx.x, lane = threadIdx.x;
  if (c >= n_clusters) return;
  const int b = a.mheads[c], e = a.mheads[c + 1];
  const float inf = __builtin_huge_valf();
  float lo0 = inf, lo1 = inf, lo2 = inf, hi0 = -inf, hi1 = -inf, hi2 = -inf;
  double s = 0.0;
  for (int j0 = b; j0 < e; j0 += 64) {
    const int cnt = min(64, e - j0);
    __syncthreads();
    if (lane < cnt) {
      const int i = (int)(a.msorted[j0 + lane] & 0xffffffffull);
      const float x = a.x[i], y = a.y[i], z = a.z[i];
      t[0][lane] = x; t[1][lane] = y; t[2][lane] = z;
      lo0 = fminf(lo0, x); lo1 = fminf(lo1, y); lo2 = fminf(lo2, z);
      hi0 = fmaxf(hi0, x); hi1 = fmaxf(hi1, y); hi2 = fmaxf(hi2, z);
    }
    __syncthreads();
    if (lane < 3)
      for (int k = 0; k < cnt; ++k) s = __dadd_rn(s, (double)t[lane][k]);
  }
  for (int w = 32; w > 0; w >>= 1) {
    lo0 = fminf(lo0, __shfl_xor(lo0, w, 64)); lo1 = fminf(lo1, __shfl_xor(lo1, w, 64)); lo2 = fminf(lo2, __shfl_xor(lo2, w, 64));
    hi0 = fmaxf(hi0, __shfl_xor(hi0, w, 64)); hi1 = fmaxf(hi1, __shfl_xor(hi1, w, 64)); hi2 = fmaxf(hi2, __shfl_xor(hi2, w, 64));
  }
  if (lane < 3) a.ocentroid[3 * (size_t)c + lane] = __ddiv_rn(s, (double)(e - b));
  if (lane == 0) {
    const int first = (int)(a.msorted[b] & 0xffffffffull);
    a.ocount[c] = e - b;
    a.ofirst[c] = first;
    a.obmin[3 * (size_t)c + 0] = lo0; a.obmin[3 * (size_t)c + 1] = lo1; a.obmin[3 * (size_t)c + 2] = lo2;
    a.obmax[3 * (size_t)c + 0] = hi0; a.obmax[3 * (size_t)c + 1] = hi1; a.obmax[3 * (size_t)c + 2] = hi2;
    uint32_t best = 0;
    if (a.labels && a.same_label) {
      best = a.label[first];
    } else if (a.labels) {
      uint32_t cur = 0;
      int best_len = 0, len = 0;
      for (int j = b; j < e; ++j) {
        const uint32_t l = (uint32_t)(a.lsorted[j] & 0xffffffffull);
        if (len > 0 && l == cur) ++len; else { cur = l; len = 1; }
        if (len > best_len) { best_len = len; best = cur; }
      }
    }
    a.olabel[c] = best;
  }
}

inline dim3 grid256(int n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

#define SICP_CLUSTER_LAUNCH(fn, kernel)                                        \
  hipError_t fn(const ClusterArgs& a, hipStream_t st) {                        \
    if (a.n <= 0) return hipSuccess;                                           \
    hipLaunchKernelGGL(kernel, grid256(a.n), dim3(256), 0, st, a);             \
    return hipGetLastError();                                                  \
  }
SICP_CLUSTER_LAUNCH(launch_cluster_keys, cluster_key_kernel)
SICP_CLUSTER_LAUNCH(launch_cluster_cell_flags, cluster_cell_flag_kernel)
SICP_CLUSTER_LAUNCH(launch_cluster_cells, cluster_cells_kernel)
SICP_CLUSTER_LAUNCH(launch_cluster_sizes, cluster_size_kernel)
SICP_CLUSTER_LAUNCH(launch_cluster_root_flags, cluster_root_flag_kernel)
SICP_CLUSTER_LAUNCH(launch_cluster_ids, cluster_id_kernel)
SICP_CLUSTER_LAUNCH(launch_cluster_member_heads, cluster_member_head_kernel)
#undef SICP_CLUSTER_LAUNCH

// the cell count stays on the device: one row of workgroups per point bounds it, and a workgroup without a cell, or without a
// chunk of its cell, leaves at once
constexpr int kPairChunkGroups = 8;
hipError_t launch_cluster_pairs(const ClusterArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(cluster_pair_kernel, dim3((unsigned)a.n, kPairChunkGroups), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_cluster_table(const ClusterArgs& a, int n_clusters, hipStream_t st) {
  if (n_clusters <= 0) return hipSuccess;
  hipLaunchKernelGGL(cluster_table_kernel, dim3((unsigned)n_clusters), dim3(64), 0, st, a, n_clusters);
  return hipGetLastError();
}

}  // namespace sicp
