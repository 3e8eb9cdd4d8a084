// range_kernels.hip -- sicp_range_image / sicp_range_labels: the spherical projection of a scan and the vote that carries a
// network's per-pixel classes back onto the points (driver: range.cpp; the rules: include/sicp.h, "range image and labels from
// it").  Project: the row edges and the column table sit in LDS, a lane per point forms its offset and squared range in float,
// finds its sector and its row by two fixed bisections on doubles -- no atan2, no sqrt, no division -- and enters the pixel with
// one 64-bit atomicMin on (bits(r2) << 32 | f) and one atomicAdd on the count.  Resolve: a lane per pixel decodes the key and
// gathers the winner into one 16-byte record.  Vote: a lane per point gathers the records of its window (at 64 x 2048 they are
// 2 MB and stay in L2), keeps the k nearest in a sorted list that lives in registers -- the list length is a template
// parameter and every index into it a compile-time constant, so nothing goes to scratch -- and counts the classes pair by pair.
// Integer atomics and ballots only: every byte is independent of the launch shape.
#include <hip/hip_runtime.h>

#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

__device__ __forceinline__ void count_ballot(bool b, int& acc) { acc += __popcll(__ballot(b)); }

// ---- project -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void range_project_kernel(RangeArgs a) {
  extern __shared__ __attribute__((aligned(16))) double range_lds[];
  const int W = a.W, H = a.H, half = W / 2;
  for (int t = threadIdx.x; t < H + 1 + W; t += 256) range_lds[t] = a.tables[t];
  __syncthreads();
  const double* row_edge = range_lds;
  const double* cos_half = range_lds + H + 1;
  const double* sin_half = cos_half + half;
  int kept = 0, outside = 0;  // (what lane 0 of a wave keeps)
  const int stride = 256 * (int)gridDim.x;
  for (int base = 256 * (int)blockIdx.x; base < a.n; base += stride) {  // (uniform over the workgroup: every lane reaches the ballots)
    const int f = base + (int)threadIdx.x;
    bool k = false, o = false;
    if (f < a.n) {
      const float px = a.x[f], py = a.y[f], pz = a.z[f];
      const float dx = px - a.ox, dy = py - a.oy, dz = pz - a.oz;                // rule 1
      const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
      const float s = xx + yy;
      const float r2 = s + zz;                                                    // rule 2
      const double R = (double)r2;
      int pix = -1;
      k = R >= a.min_sq && R < a.max_sq;
      if (k) {
        const double X = (double)dx, Y = (double)dy, Z = (double)dz;              // rule 3
        const double XX = X * X, YY = Y * Y;
        const double D = XX + YY;
        const double Zs = Z * fabs(Z);
        const double top = row_edge[0] * D, bottom = row_edge[H] * D;
        o = (Zs > top) || !(Zs >= bottom);                                        // rule 5
        if (!o) {
          int lo = 0, hi = H;
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            const double e = row_edge[mid] * D;
            if (Zs < e) lo = mid; else hi = mid;
          }
          const int row = lo;
          const bool lower = !(dy > 0.f || (dy == 0.f && dx > 0.f));              // rule 4
          const double xp = lower ? -X : X;
          const double yp = lower ? -Y : Y;
          lo = 0; hi = half;
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            const double u = cos_half[mid] * yp;
            const double v = sin_half[mid] * xp;
            if ((u - v) >= 0.0) lo = mid; else hi = mid;
          }
          const int sec = lo + (lower ? half : 0);
          int col = (a.clockwise ? W - 1 - sec : sec) + a.col_shift;
          col -= col >= W ? W : 0;
          pix = row * W + col;
          atomicMin(&a.key[pix], ((u64)__float_as_uint(r2) << 32) | (u64)(unsigned)f);  // rule 6
          atomicAdd(&a.count[pix], 1u);
        }
      }
      a.pix[f] = pix;
      if (a.o_pixel) a.o_pixel[a.caller ? a.caller[f] : f] = pix;
    }
    count_ballot(k, kept);
    count_ballot(o, outside);
  }
  if ((threadIdx.x & 63) == 0) {
    if (kept) atomicAdd(a.res + kRgKept, kept);
    if (outside) atomicAdd(a.res + kRgOutsideFov, outside);
  }
}

// ---- resolve -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void range_resolve_kernel(RangeArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int n_pix = a.W * a.H;
  bool hit = false;
  if (p < n_pix) {
    const u64 key = a.key[p];
    hit = key != kRangeEmptyKey;
    int index = -1;
    float r2 = 0.f, x = 0.f, y = 0.f, z = 0.f;
    uint32_t label = 0, word = 0;
    if (hit) {
      const int f = (int)(unsigned)(key & 0xffffffffull);
      r2 = __uint_as_float((unsigned)(key >> 32));
      x = a.x[f]; y = a.y[f]; z = a.z[f];
      label = a.label ? a.label[f] : 0u;
      word = a.pixel_label ? a.pixel_label[p] : label;
      index = a.caller ? a.caller[f] : f;
    }
    a.rec[p] = make_float4(hit ? x : __uint_as_float(0x7fc00000u), y, z, __uint_as_float(word));
    if (a.o_index) a.o_index[p] = index;
    if (a.o_range_sq) a.o_range_sq[p] = r2;
    if (a.o_x) a.o_x[p] = x;
    if (a.o_y) a.o_y[p] = y;
    if (a.o_z) a.o_z[p] = z;
    if (a.o_label) a.o_label[p] = label;
  }
  const u64 ballot = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(a.res + kRgPixelsHit, (int)__popcll(ballot));
}

// ---- visible -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void range_visible_kernel(RangeArgs a) {
  const int stride = 256 * (int)gridDim.x;
  for (int f = 256 * (int)blockIdx.x + (int)threadIdx.x; f < a.n; f += stride) {
    const int pix = a.pix[f];
    if (pix >= 0 && (unsigned)(a.key[pix] & 0xffffffffull) == (unsigned)f) a.o_visible[a.caller ? a.caller[f] : f] = 1;
  }
}

// ---- vote ----------------------------------------------------------------------------------------------------------------
// KB: the list's length, the smallest of 1, 2, 4, 8, 16 that holds k.  key[] ascends; an entry is (bits(d2) << 32 | visiting
// order), kRangeEmptyKey where the list is not full.
template <int KB>
__global__ __launch_bounds__(256) void range_vote_kernel(RangeArgs a) {
  const int W = a.W, H = a.H, half = a.window >> 1, k = a.k;
  int voted = 0;
  const int stride = 256 * (int)gridDim.x;
  for (int base = 256 * (int)blockIdx.x; base < a.n; base += stride) {
    const int f = base + (int)threadIdx.x;
    bool v = false;
    if (f < a.n) {
      const int pix = a.pix[f];
      uint32_t out = a.label ? a.label[f] : 0u;  // rule 12
      int nv = 0;
      if (pix >= 0) {
        const int r = pix / W, c = pix - r * W;
        const float px = a.x[f], py = a.y[f], pz = a.z[f];
        u64 key[KB];
        uint32_t lab[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) { key[j] = kRangeEmptyKey; lab[j] = 0; }
        unsigned order = 0;
        for (int wr = -half; wr <= half; ++wr) {
          const int rr = r + wr;
          for (int wc = -half; wc <= half; ++wc, ++order) {
            if (rr < 0 || rr >= H) continue;                                       // rule 8
            int cc = c + wc;
            cc += cc < 0 ? W : 0;
            cc -= cc >= W ? W : 0;
            const float4 q = a.rec[rr * W + cc];
            const float ex = px - q.x, ey = py - q.y, ez = pz - q.z;               // rule 9 (an empty pixel: NaN, no part)
            const float exx = ex * ex, eyy = ey * ey, ezz = ez * ez;
            const float s = exx + eyy;
            const float d2 = s + ezz;
            if ((double)d2 < a.max_dist_sq) {
              u64 e = ((u64)__float_as_uint(d2) << 32) | (u64)order;               // rule 10
              uint32_t el = __float_as_uint(q.w);
#pragma unroll
              for (int j = 0; j < KB; ++j) {  // the carried entry is the larger of the two from here on
                const bool less = e < key[j];
                const u64 tk = key[j];
                const uint32_t tl = lab[j];
                key[j] = less ? e : tk;
                lab[j] = less ? el : tl;
                e = less ? tk : e;
                el = less ? tl : el;
              }
            }
          }
        }
        int best = 0;
        uint32_t best_lab = 0;
#pragma unroll
        for (int i = 0; i < KB; ++i) {                                             // rule 11
          const bool in_i = i < k && key[i] != kRangeEmptyKey && lab[i] != 0u;
          int cnt = 0;
#pragma unroll
          for (int j = 0; j < KB; ++j) cnt += (j < k && key[j] != kRangeEmptyKey && lab[j] == lab[i]) ? 1 : 0;
          if (in_i && (cnt > best || (cnt == best && lab[i] < best_lab))) { best = cnt; best_lab = lab[i]; }
        }
        if (best > 0) { out = best_lab; nv = best; v = true; }
      }
      const int ci = a.caller ? a.caller[f] : f;
      if (a.o_out_label) a.o_out_label[ci] = out;
      if (a.o_votes) a.o_votes[ci] = (uint8_t)nv;
    }
    count_ballot(v, voted);
  }
  if ((threadIdx.x & 63) == 0 && voted) atomicAdd(a.res + kRgVoted, voted);
}

bool range_shape_ok(const RangeArgs& a) {
  return a.W >= 16 && a.W <= kRangeMaxWidth && a.W % 2 == 0 && a.H >= 1 && a.H <= kRangeMaxHeight && a.col_shift >= 0 &&
         a.col_shift < a.W && a.n >= 0;
}
unsigned point_groups(int n) {
  const long long groups = ((long long)n + 255) / 256;
  return (unsigned)(groups < kRangeMaxGroups ? groups : kRangeMaxGroups);
}

}  // namespace

hipError_t launch_range_project(const RangeArgs& a, hipStream_t st) {
  if (!range_shape_ok(a)) return hipErrorInvalidValue;
  if (a.n <= 0) return hipSuccess;
  const size_t lds = sizeof(double) * (size_t)(a.H + 1 + a.W);  // at most 34 824 bytes
  hipLaunchKernelGGL(range_project_kernel, dim3(point_groups(a.n)), dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_range_resolve(const RangeArgs& a, hipStream_t st) {
  if (!range_shape_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(range_resolve_kernel, dim3((unsigned)((a.W * a.H + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_range_visible(const RangeArgs& a, hipStream_t st) {
  if (!range_shape_ok(a) || !a.o_visible) return hipErrorInvalidValue;
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(range_visible_kernel, dim3(point_groups(a.n)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_range_vote(const RangeArgs& a, hipStream_t st) {
  if (!range_shape_ok(a) || a.window < 1 || a.window > kRangeMaxWindow || a.window % 2 == 0 || a.k < 1 || a.k > kRangeMaxK)
    return hipErrorInvalidValue;
  if (a.n <= 0) return hipSuccess;
  const dim3 grid(point_groups(a.n)), block(256);
  if (a.k <= 1) hipLaunchKernelGGL(range_vote_kernel<1>, grid, block, 0, st, a);
  else if (a.k <= 2) hipLaunchKernelGGL(range_vote_kernel<2>, grid, block, 0, st, a);
  else if (a.k <= 4) hipLaunchKernelGGL(range_vote_kernel<4>, grid, block, 0, st, a);
  else if (a.k <= 8) hipLaunchKernelGGL(range_vote_kernel<8>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(range_vote_kernel<16>, grid, block, 0, st, a);
  return hipGetLastError();
}

}  // namespace sicp
