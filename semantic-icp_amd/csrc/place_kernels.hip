// place_kernels.hip -- sicp_place_*: scan descriptors and the loop-candidate search (driver: place.cpp; the rules:
// include/sicp.h and INTEGRATION.md, "Place recognition").  A descriptor is R rings x S sectors of uint8 cell codes.  Describe:
// one pass over the points with integer atomics into a zeroed table (counts per (cell, label), or count and largest level per
// cell), then one lane per cell.  Search: one wave per (query, entry), one lane per sector shift; the query lies in LDS with
// every ring stored twice end to end, so a shift is a byte offset (two LDS words and a byte-align), and the entry's words come
// from memory once per wave as coalesced loads, a word per lane, handed round by lane reads.  Four cells are compared per
// 32-bit word with zero-byte masks and population counts.  Everything the search computes is an integer: every launch shape
// gives the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>

#define SICP_HD __host__ __device__
#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

// ---- describe ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void place_cells_kernel(PlaceDescribeArgs a) {
  __shared__ double tab[kPlaceMaxRings + 1 + kPlaceMaxSectors];
  __shared__ unsigned int kept_in_block;
  const int R = a.R, S = a.S, half = S / 2;
  for (int t = threadIdx.x; t < R + 1 + S; t += 256) tab[t] = a.tables[t];
  if (threadIdx.x == 0) kept_in_block = 0;
  __syncthreads();
  const double* edge2 = tab;
  const double* cos_half = tab + R + 1;
  const double* sin_half = cos_half + half;
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  if (i < a.n) {
    const float dx = a.x[i] - a.ox, dy = a.y[i] - a.oy, dz = a.z[i] - a.oz;
    const float xx = dx * dx, yy = dy * dy;
    const float d2 = xx + yy;
    const double D = (double)d2;
    keep = D < edge2[R] && D >= a.min_range_sq;
    if (keep) {
      int ring = 0;
      for (int r = 1; r < R; ++r) ring += D >= edge2[r] ? 1 : 0;
      const bool lower = !(dy > 0.f || (dy == 0.f && dx > 0.f));
      const double xp = lower ? -(double)dx : (double)dx;
      const double yp = lower ? -(double)dy : (double)dy;
      int sector = lower ? half : 0;
      for (int j = 1; j < half; ++j) {
        const double u = cos_half[j] * yp;
        const double v = sin_half[j] * xp;
        sector += (u - v) >= 0.0 ? 1 : 0;
      }
      const size_t cell = (size_t)ring * (size_t)S + (size_t)sector;
      if (a.label) {
        const uint32_t l = a.label[i];
        if (l > (uint32_t)a.C) {
          a.res[kPlaceBadLabel] = 1;  // (plain store: every writer stores the same 1)
        } else if (l != 0 && !((a.ignore[l >> 5] >> (l & 31)) & 1u)) {
          atomicAdd(&a.table[cell * (size_t)a.C + (l - 1)], 1u);
        }
      } else {
        const double t = ((double)dz - a.z_min) * a.inv_z_step;
        const uint32_t level = t < 0.0 ? 0u : t >= 254.0 ? 254u : (uint32_t)(int)t;  // (t in [0, 254): the cast is the floor)
        atomicAdd(&a.table[2 * cell], 1u);
        atomicMax(&a.table[2 * cell + 1], level);
      }
    }
  }
  const u64 ballot = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(&kept_in_block, (unsigned int)__popcll(ballot));
  __syncthreads();
  if (threadIdx.x == 0 && kept_in_block) atomicAdd(&a.res[kPlaceKept], (u64)kept_in_block);
}

__global__ __launch_bounds__(256) void place_finalise_kernel(PlaceDescribeArgs a) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  uint8_t code = 0;
  if (cell < a.R * a.S) {
    if (a.label) {
      const uint32_t* h = a.table + (size_t)cell * (size_t)a.C;
      uint32_t best = 0, total = 0;
      int arg = 0;
      for (int l = 0; l < a.C; ++l) {
        const uint32_t c = h[l];
        total += c;
        if (c > best) { best = c; arg = l + 1; }  // (strictly more: ties stay with the smallest label)
      }
      if (total >= (uint32_t)a.min_cell_points) code = (uint8_t)arg;
    } else {
      if (a.table[2 * (size_t)cell] >= (uint32_t)a.min_cell_points) code = (uint8_t)(1u + a.table[2 * (size_t)cell + 1]);
    }
    a.desc[cell] = code;
  }
  const u64 ballot = __ballot(code != 0);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(&a.res[kPlaceCells], (u64)__popcll(ballot));
}

// ---- search ------------------------------------------------------------------------------------------------------------
// bit 7 of every byte of v that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v) {
  return (((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;
}

// is (m, e, s) a better (match, either, shift) than (bm, be, bs): a larger fraction, or the same with the smaller shift.  The
// products stay below 2^29 (match <= either <= 16384).  Within one (query, entry) pair either = 0 at one shift means either = 0
// at all of them, so a 0 / 0 only ever meets its like or the 0 / 1 of a lane without a shift.
__device__ __forceinline__ bool place_better(int m, int e, int s, int bm, int be, int bs) {
  const int l = m * be, r = bm * e;
  return l > r || (l == r && s < bs);
}

constexpr int kSearchWaves = 4;

__global__ __launch_bounds__(64 * kSearchWaves) void place_search_kernel(const uint32_t* __restrict__ query, const uint32_t* __restrict__ entries,
                                                                         int n_q, int count, int R, int S, u64* __restrict__ key,
                                                                         u64* __restrict__ hit) {
  extern __shared__ uint32_t q2[];  // [R][S / 2] words: ring r's S bytes twice, then one word that is read and never used
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int row_words = S / 4, words = R * row_words;
  for (int q = blockIdx.y; q < n_q; q += gridDim.y) {
    __syncthreads();  // (the previous query's readers are done)
    const uint32_t* qsrc = query + (size_t)q * (size_t)words;
    for (int t = threadIdx.x; t < 2 * words; t += blockDim.x) {
      const int r = t / (2 * row_words), w = t - r * 2 * row_words;
      q2[t] = qsrc[r * row_words + (w >= row_words ? w - row_words : w)];
    }
    if (threadIdx.x == 0) q2[2 * words] = 0;
    __syncthreads();
    for (int e = blockIdx.x * kSearchWaves + wave; e < count; e += gridDim.x * kSearchWaves) {
      const uint32_t* ew = entries + (size_t)e * (size_t)words;
      int bm = 0, be = 1, bs = 0x7fffffff;
      for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool live = s < S;
        const int a0 = S - (live ? s : 0);  // first byte of this lane's window into a doubled ring: 1..S
        const int k = a0 & 3, i0 = a0 >> 2;
        int m = 0, ei = 0;
        // the entry, 64 words at a time: lane l holds word f0 + l (one coalesced load, the next one in flight meanwhile), and
        // word f0 + i reaches every lane through a read of lane i.  Entry word f = r * row_words + w meets the query's bytes
        // a0 + 4w .. a0 + 4w + 3 of doubled ring r: words f + off and f + off + 1 of q2 with off = r * row_words + i0.
        uint32_t next = lane < words ? ew[lane] : 0u;
        int w = 0, off = i0;
        for (int f0 = 0; f0 < words; f0 += 64) {
          const uint32_t mine = next;
          next = f0 + 64 + lane < words ? ew[f0 + 64 + lane] : 0u;
          const int lim = min(64, words - f0);
#pragma unroll 4
          for (int i = 0; i < lim; ++i) {
            const uint32_t ev = (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
            const uint32_t lo = q2[f0 + i + off], hi = q2[f0 + i + off + 1];
            const uint32_t qv = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)k);
            const uint32_t differ = nonzero_bytes(qv ^ ev);
            m += __popc(nonzero_bytes(qv) & ~differ);
            ei += __popc(nonzero_bytes(qv | ev));
            if (++w == row_words) { w = 0; off += row_words; }
          }
        }
        if (live && place_better(m, ei, s, bm, be, bs)) { bm = m; be = ei; bs = s; }
      }
      for (int off = 32; off >= 1; off >>= 1) {
        const int om = __shfl_xor(bm, off), oe = __shfl_xor(be, off), os = __shfl_xor(bs, off);
        if (place_better(om, oe, os, bm, be, bs)) { bm = om; be = oe; bs = os; }
      }
      if (lane == 0) {
        const u64 sk = be > 0 ? ((u64)bm << 30) / (u64)be : 0ull;
        const size_t at = (size_t)q * (size_t)count + (size_t)e;
        key[at] = (((1ull << 30) - sk) << 31) | (u64)e;
        hit[at] = (u64)bs | ((u64)bm << 16) | ((u64)be << 32);
      }
    }
  }
}

__global__ __launch_bounds__(256) void place_gather_kernel(const u64* __restrict__ sorted_key, const u64* __restrict__ hit, int n_q, int count,
                                                           int top, int4* __restrict__ rows) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n_q * top) return;
  const int q = (int)(t / top), k = (int)(t - (long long)q * top);
  const u64 key = sorted_key[(size_t)q * (size_t)count + (size_t)k];
  const int e = (int)(key & 0x7fffffffull);
  const u64 h = hit[(size_t)q * (size_t)count + (size_t)e];
  rows[t] = make_int4(e, (int)(h & 0xffffull), (int)((h >> 16) & 0xffffull), (int)((h >> 32) & 0xffffull));
}

bool place_shape_ok(int R, int S) { return R >= 1 && R <= kPlaceMaxRings && S >= 4 && S <= kPlaceMaxSectors && S % 4 == 0; }

}  // namespace

hipError_t launch_place_cells(const PlaceDescribeArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (!place_shape_ok(a.R, a.S) || (a.label && (a.C < 1 || a.C > 255))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(place_cells_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_place_finalise(const PlaceDescribeArgs& a, hipStream_t st) {
  if (!place_shape_ok(a.R, a.S) || (a.label && (a.C < 1 || a.C > 255))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(place_finalise_kernel, dim3((unsigned)((a.R * a.S + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_place_search(const PlaceSearchArgs& a, hipStream_t st) {
  if (a.n_q <= 0 || a.count <= 0) return hipSuccess;
  if (!place_shape_ok(a.R, a.S)) return hipErrorInvalidValue;
  // waves enough to fill the device a few times over; a wave walks its entries with the grid's stride
  const long long want = ((long long)a.count + kSearchWaves - 1) / kSearchWaves;
  const unsigned gx = (unsigned)std::min<long long>(want, 2048);
  const unsigned gy = (unsigned)std::min(a.n_q, 1024);
  const size_t lds = sizeof(uint32_t) * ((size_t)a.R * (size_t)a.S / 2 + 1);
  hipLaunchKernelGGL(place_search_kernel, dim3(gx, gy), dim3(64 * kSearchWaves), lds, st, reinterpret_cast<const uint32_t*>(a.query),
                     reinterpret_cast<const uint32_t*>(a.entries), a.n_q, a.count, a.R, a.S, a.key, a.hit);
  return hipGetLastError();
}

hipError_t launch_place_gather(const unsigned long long* sorted_key, const unsigned long long* hit, int n_q, int count, int top, int4* rows,
                               hipStream_t st) {
  if (n_q <= 0 || top <= 0) return hipSuccess;
  if (top > count) return hipErrorInvalidValue;
  const long long n = (long long)n_q * top;
  hipLaunchKernelGGL(place_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, sorted_key, hit, n_q, count, top, rows);
  return hipGetLastError();
}

}  // namespace sicp
