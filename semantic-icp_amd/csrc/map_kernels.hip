// map_kernels.hip -- sicp_map_*: the persistent voxel map (driver: map.cpp; the rules: INTEGRATION.md, "A persistent voxel
// map").  The map's rows lie sorted by voxel key.  An integrate keys the scan's points with merge's arithmetic
// (voxel_key.hpp), sorts THEM (a stable radix sort: point indices ascend inside a voxel), and merges by rank: a lower-bound
// search of every scan voxel among the map's keys, a search of every map row among the few absent keys, one pass that moves
// the rows to their new places in the spare buffers, and one lane per scan voxel that continues its row's f64 sums in point
// order.  A lane owns its row: plain stores, no float atomics, so every byte is run-to-run reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>

#define SICP_HD __host__ __device__
#include "kernels.h"
#include "voxel_key.hpp"

#pragma clang fp contract(off)

namespace sicp {
namespace {

typedef unsigned long long u64;

// the number of keys below k in the ascending keys[n]
__device__ __forceinline__ int map_lower_bound(const u64* keys, int n, u64 k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// per point of the scan: transform, crop, voxel key (~0 for a dropped point); a coordinate beyond the key's fields and a label
// beyond the histogram raise their flags (plain stores: every writer stores the same 1)
__global__ __launch_bounds__(256) void map_key_kernel(MapKeyArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const double x = a.x[i], y = a.y[i], z = a.z[i];
  const float px = voxel_xform_row(a.M + 0, x, y, z);
  const float py = voxel_xform_row(a.M + 4, x, y, z);
  const float pz = voxel_xform_row(a.M + 8, x, y, z);
  a.tx[i] = px; a.ty[i] = py; a.tz[i] = pz;
  u64 k = kVoxelDropped;
  if (!a.crop || voxel_crop_keeps(px, py, pz, a.cx, a.cy, a.cz, a.range_sq)) {
    if (!voxel_key(px, py, pz, a.inv_leaf, &k)) {
      k = kVoxelDropped;
      a.res[kMapRange] = 1;
    }
    if (a.label && a.label[i] > (uint32_t)a.num_classes) a.res[kMapBadLabel] = 1;
  }
  a.key[i] = k;
  a.val[i] = i;
}

// one lane per scan voxel: where its key stands among the map's, and whether it is there
__global__ __launch_bounds__(256) void map_lookup_kernel(MapFoldArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.n) return;
  int miss = 0;
  if (k < a.res[kMapScanVoxels]) {
    const u64 key = a.skey[a.heads[k]];
    const int r = map_lower_bound(a.from.key, a.n_map, key);
    a.rank[k] = r;
    miss = (r < a.n_map && a.from.key[r] == key) ? 0 : 1;
  }
  a.miss[k] = miss;
}

// the absent keys, compacted (ascending, as the scan's voxels are), and their number
__global__ __launch_bounds__(256) void map_miss_kernel(MapFoldArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.n) return;
  const int f = a.miss[k], p = a.mpos[k];
  if (f) {
    a.miss_key[p] = a.skey[a.heads[k]];
    a.miss_rank[p] = a.rank[k];
  }
  if (k == a.n - 1) a.res[kMapNew] = p + f;
}

// one lane per row of the grown map: an old row i moves up by the absent keys below it, absent key j opens the row
// j + (old keys below it), empty
__global__ __launch_bounds__(256) void map_scatter_kernel(MapFoldArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < a.n_map) {
    const u64 key = a.from.key[t];
    const int r = t + map_lower_bound(a.miss_key, a.n_new, key);
    a.to.key[r] = key;
    a.to.sx[r] = a.from.sx[t]; a.to.sy[r] = a.from.sy[t]; a.to.sz[r] = a.from.sz[t];
    a.to.cnt[r] = a.from.cnt[t];
    a.src_of[r] = t;
  } else if (t - a.n_map < a.n_new) {
    const int j = t - a.n_map;
    const int r = j + a.miss_rank[j];
    a.to.key[r] = a.miss_key[j];
    a.to.sx[r] = 0.0; a.to.sy[r] = 0.0; a.to.sz[r] = 0.0;
    a.to.cnt[r] = 0u;
    a.src_of[r] = -1;
  }
}

// histogram rows to their new places (consecutive lanes write consecutive words)
__global__ __launch_bounds__(256) void map_move_hist_kernel(const uint32_t* from, uint32_t* to, const int* src_of, long long total, int stride) {
  const long long step = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
    const long long r = e / stride;
    const int s = src_of[r];
    to[e] = s >= 0 ? from[(long long)s * stride + (e - r * stride)] : 0u;
  }
}

// one lane per scan voxel: its row's sums continued with the voxel's points in ascending point index -- s += (double)p, one
// add per point, from the stored value (the order is the specification: a voxel's run is not split across lanes) -- and its
// count and histogram bins.  Scan voxel k's row: its rank among the old keys plus the absent keys below it.
__global__ __launch_bounds__(256) void map_fold_kernel(MapFoldArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n_vox = a.res[kMapScanVoxels], n_kept = a.res[kMapKept];
  if (k >= a.n || k >= n_vox) return;
  const int r = a.rank[k] + a.mpos[k];
  if (r >= a.n_map + a.n_new) return;  // (cannot happen; a row beyond the buffers is never written)
  const int b = a.heads[k], e = k + 1 < n_vox ? a.heads[k + 1] : n_kept;
  double sx = a.to.sx[r], sy = a.to.sy[r], sz = a.to.sz[r];
  uint32_t* const h = a.stride > 0 ? a.to.hist + (size_t)r * (size_t)a.stride : nullptr;
  for (int j = b; j < e; ++j) {
    sx += (double)a.gx[j]; sy += (double)a.gy[j]; sz += (double)a.gz[j];
    if (h) {
      const uint32_t l = (uint32_t)(a.lkey[j] & 0xffffffffull);
      if (l < (uint32_t)a.stride) h[l] += 1u;  // (labels beyond the bins were refused before this launch)
    }
  }
  a.to.sx[r] = sx; a.to.sy[r] = sy; a.to.sz[r] = sz;
  a.to.cnt[r] += (uint32_t)(e - b);
}

// a row's centroid as the caller sees it: (float)(s / count) per axis
__device__ __forceinline__ void map_centroid(const MapRows& R, int i, float* cx, float* cy, float* cz) {
  const double c = (double)R.cnt[i];
  *cx = (float)(R.sx[i] / c); *cy = (float)(R.sy[i] / c); *cz = (float)(R.sz[i] / c);
}

// flag[i]: row i has at least min_count points and its centroid passes the crop
__global__ __launch_bounds__(256) void map_select_kernel(MapSelectArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_map) return;
  bool keep = (long long)a.rows.cnt[i] >= a.min_count;
  if (keep && a.crop) {
    float px, py, pz;
    map_centroid(a.rows, i, &px, &py, &pz);
    keep = voxel_crop_keeps(px, py, pz, a.cx, a.cy, a.cz, a.range_sq);
  }
  a.flag[i] = keep ? 1 : 0;
}

// the surviving rows, bit for bit, to the spare buffers; their number and the sum of their counts (one integer atomic a wave)
__global__ __launch_bounds__(256) void map_prune_kernel(MapSelectArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  u64 c = 0;
  if (i < a.n_map) {
    const int f = a.flag[i], p = a.pos[i];
    if (f) {
      a.to.key[p] = a.rows.key[i];
      a.to.sx[p] = a.rows.sx[i]; a.to.sy[p] = a.rows.sy[i]; a.to.sz[p] = a.rows.sz[i];
      a.to.cnt[p] = a.rows.cnt[i];
      a.src_of[p] = i;
      c = a.rows.cnt[i];
    }
    if (i == a.n_map - 1) a.res[kMapOut] = p + f;
  }
  unsigned lo = (unsigned)c, carry = 0;  // (64 counts below 2^32: the wave's sum in two words)
  for (int w = 32; w > 0; w >>= 1) {
    const unsigned olo = (unsigned)__shfl_xor((int)lo, w, 64), oc = (unsigned)__shfl_xor((int)carry, w, 64);
    const unsigned s = lo + olo;
    carry += oc + (s < lo ? 1u : 0u);
    lo = s;
  }
  const u64 sum = ((u64)carry << 32) | lo;
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(a.kept_points, sum);
}

// the selected rows as points, ascending key: centroid, count, the arg-max bin (ties to the smallest label); their number and
// the largest count
__global__ __launch_bounds__(256) void map_extract_kernel(MapSelectArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int cnt = 0;
  if (i < a.n_map) {
    const int f = a.flag[i], p = a.pos[i];
    if (f) {
      float px, py, pz;
      map_centroid(a.rows, i, &px, &py, &pz);
      a.ox[p] = px; a.oy[p] = py; a.oz[p] = pz;
      const uint32_t c = a.rows.cnt[i];
      a.ocount[p] = c;
      cnt = (int)(c > 0x7fffffffu ? 0x7fffffffu : c);
      a.src_of[p] = i;
      if (a.olabel) a.olabel[p] = map_fullest_bin(a.rows.hist + (size_t)i * (size_t)a.stride, a.stride);
    }
    if (i == a.n_map - 1) a.res[kMapOut] = p + f;
  }
  int m = cnt;
  for (int w = 32; w > 0; w >>= 1) m = max(m, __shfl_xor(m, w, 64));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&a.res[kMapMaxCount], m);
}

// ---- free-space carving (kernels.h: MapCarveArgs) ------------------------------------------------------------------------------
// the lower bound of k in keys[lo, hi): every key below lo is known to be < k, every key from hi on >= k
__device__ __forceinline__ int map_lower_bound_in(const u64* keys, int lo, int hi, u64 k) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the lower bound of k, known to be >= from: probes at from, from + 2, from + 6, from + 14 ... (each 1, 2, 4, 8 ... past the
// last key found below k) bracket it
__device__ __forceinline__ int map_gallop_up(const u64* keys, int n, int from, u64 k) {
  int lo = from, hi = n;
  for (long long s = 1;; s <<= 1) {
    const long long p = (long long)lo + (s - 1);
    if (p >= n) break;
    if (keys[p] >= k) { hi = (int)p; break; }
    lo = (int)p + 1;
  }
  return map_lower_bound_in(keys, lo, hi, k);
}

// the lower bound of k, known to be <= from (<= n): probes at from - 1, from - 3, from - 7 ... (each 1, 2, 4 ... below the last
// key found >= k) bracket it
__device__ __forceinline__ int map_gallop_down(const u64* keys, int from, u64 k) {
  int lo = 0, hi = from;
  for (long long s = 1;; s <<= 1) {
    const long long p = (long long)hi - s;
    if (p < 0) break;
    if (keys[p] < k) { lo = (int)p + 1; break; }
    hi = (int)p;
  }
  return map_lower_bound_in(keys, lo, hi, k);
}

// the sensor origin as a point of the scan: transformed, keyed; false when it lies beyond the key's range
template <class Args>  // (MapCarveArgs, MapRaycastArgs)
__device__ __forceinline__ bool carve_origin(const Args& a, float* ox, float* oy, float* oz, u64* ko) {
  const double x = a.sx, y = a.sy, z = a.sz;
  *ox = voxel_xform_row(a.M + 0, x, y, z);
  *oy = voxel_xform_row(a.M + 4, x, y, z);
  *oz = voxel_xform_row(a.M + 8, x, y, z);
  return voxel_key(*ox, *oy, *oz, a.inv_leaf, ko);
}

// per point of the scan: the row of its voxel, when the map holds it, is hit (plain stores: every writer stores the same 1)
__global__ __launch_bounds__(256) void map_carve_hit_kernel(MapCarveArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    float ox, oy, oz;
    u64 ko;
    if (!carve_origin(a, &ox, &oy, &oz, &ko)) a.res[kMapRange] = 1;
  }
  if (i >= a.n) return;
  const double x = a.x[i], y = a.y[i], z = a.z[i];
  const float px = voxel_xform_row(a.M + 0, x, y, z);
  const float py = voxel_xform_row(a.M + 4, x, y, z);
  const float pz = voxel_xform_row(a.M + 8, x, y, z);
  u64 k;
  if (!voxel_key(px, py, pz, a.inv_leaf, &k)) return;
  const int r = map_lower_bound(a.key, a.n_map, k);
  if (r < a.n_map && a.key[r] == k) a.hit[r] = 1;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int w = 32; w > 0; w >>= 1) v += (u64)__shfl_xor((long long)v, w, 64);
  return v;
}

// The lookup of a walk's step (the carve walk and the ray cast share it): the ray has just stepped along `axis` into the voxel
// r.key; lb and found, which described the voxel it left, become the new key's lower bound among the map's keys and whether
// the map holds it.  A step along x derives both from the row beside the old one, a step along y gallops from lb, a step
// along z searches the side it went to.
__device__ __forceinline__ void map_walk_lookup(const u64* keys, int n_map, const VoxelRay& r, int axis, int* lb_io, bool* found_io) {
  int lb = *lb_io;
  bool found = *found_io;
  const u64 k = r.key;
  if (axis == 0 && r.sx < 0) {  // the key went down by 1: it is the row below or it is absent
    found = lb > 0 && keys[lb - 1] == k;
    lb -= found ? 1 : 0;
  } else {
    if (axis == 0) lb += found ? 1 : 0;  // up by 1: the keys below it are those below the old key, and the old key
    else if (axis == 1) lb = r.sy > 0 ? map_gallop_up(keys, n_map, lb + (found ? 1 : 0), k) : map_gallop_down(keys, lb, k);
    else lb = r.sz > 0 ? map_lower_bound_in(keys, lb + (found ? 1 : 0), n_map, k) : map_lower_bound_in(keys, 0, lb, k);
    found = lb < n_map && keys[lb] == k;
  }
  *lb_io = lb;
  *found_io = found;
}

// The walk.  A wave owns the rays [wave * kCarveRaysPerWave, ...) and deals them to its lanes as they fall idle: every turn
// of the loop the idle lanes take the next rays in lane order, then every lane with a ray visits the voxel it stands in and
// steps on.  `lb` is the lower bound of the lane's key among the map's and `found` says whether the map holds it
// (map_walk_lookup carries them from step to step).
// The counts are integer atomics, so neither the dealing nor the launch shape shows in the result.
__global__ __launch_bounds__(256) void map_carve_walk_kernel(MapCarveArgs a) {
  float ox, oy, oz;
  u64 ko;
  if (!carve_origin(a, &ox, &oy, &oz, &ko)) return;  // (the same in every lane; the host refuses the call)
  const int lane = threadIdx.x & 63;
  const long long first = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * kCarveRaysPerWave;
  const int end = (int)std::min<long long>(first + kCarveRaysPerWave, a.n);
  int next = (int)std::min<long long>(first, a.n);
  const u64* const keys = a.key;
  const int n_map = a.n_map;
  const int lb0 = map_lower_bound(keys, n_map, ko);  // every ray starts in the origin's voxel
  const bool found0 = lb0 < n_map && keys[lb0] == ko;
  VoxelRay r;
  int left = 0, lb = 0;
  bool found = false;
  u64 rays = 0, steps = 0;
  for (;;) {
    const bool idle = left == 0;
    const u64 idle_mask = __ballot(idle);
    if (idle_mask == ~0ull && next >= end) break;
    if (idle) {
      const int i = next + __popcll(idle_mask & ((1ull << lane) - 1ull));
      if (i < end) {
        const double x = a.x[i], y = a.y[i], z = a.z[i];
        const float px = voxel_xform_row(a.M + 0, x, y, z);
        const float py = voxel_xform_row(a.M + 4, x, y, z);
        const float pz = voxel_xform_row(a.M + 8, x, y, z);
        u64 kp;
        if (voxel_key(px, py, pz, a.inv_leaf, &kp) && (!a.ranged || voxel_crop_keeps(px, py, pz, ox, oy, oz, a.range_sq))) {
          rays += 1;
          voxel_ray_begin(ox, oy, oz, ko, px, py, pz, kp, a.inv_leaf, &r);
          left = r.n > a.end_margin ? r.n - a.end_margin : 0;
          steps += (u64)left;
          if (n_map == 0) left = 0;  // (an empty map: the candidates are counted, there is nothing to look up)
          lb = lb0;
          found = found0;
        }
      }
    }
    next = (int)std::min<long long>((long long)next + __popcll(idle_mask), end);
    if (left > 0) {
      if (found) atomicAdd(&a.miss[lb], 1u);
      left -= 1;
      if (left > 0) {
        const int axis = voxel_ray_step(&r);
        map_walk_lookup(keys, n_map, r, axis, &lb, &found);
      }
    }
  }
  rays = wave_sum(rays);
  steps = wave_sum(steps);
  if (lane == 0) {
    if (rays) atomicAdd(&a.stat[kCarveRays], rays);
    if (steps) atomicAdd(&a.stat[kCarveSteps], steps);
  }
}

// flag[i]: row i stays -- fewer than min_rays rays passed through it, or a return landed in it, or its fullest bin is
// protected (asked in that order); the counts of sicp_map_carve_info, one integer atomic a wave each
__global__ __launch_bounds__(256) void map_carve_select_kernel(MapCarveSelectArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool touched = false, hit = false, removed = false, spared_hit = false, spared_label = false;
  if (i < a.n_map) {
    const uint32_t m = a.miss[i];
    touched = m > 0u;
    hit = a.hit[i] != 0;
    if (m >= (uint32_t)a.min_rays) {
      if (hit) {
        spared_hit = true;
      } else {
        if (a.n_protect > 0) {
          const uint32_t l = map_fullest_bin(a.hist + (size_t)i * (size_t)a.stride, a.stride);
          for (int j = 0; j < a.n_protect; ++j) spared_label = spared_label || a.protect[j] == l;
        }
        removed = !spared_label;
      }
    }
    a.flag[i] = removed ? 0 : 1;
  }
  const u64 b0 = __ballot(touched), b1 = __ballot(hit), b2 = __ballot(removed), b3 = __ballot(spared_hit), b4 = __ballot(spared_label);
  if ((threadIdx.x & 63) == 0) {
    if (b0) atomicAdd(&a.stat[kCarveTouched], (u64)__popcll(b0));
    if (b1) atomicAdd(&a.stat[kCarveHit], (u64)__popcll(b1));
    if (b2) atomicAdd(&a.stat[kCarveRemoved], (u64)__popcll(b2));
    if (b3) atomicAdd(&a.stat[kCarveSparedHit], (u64)__popcll(b3));
    if (b4) atomicAdd(&a.stat[kCarveSparedLabel], (u64)__popcll(b4));
  }
}

// ---- ray casting (kernels.h: MapRaycastArgs) -----------------------------------------------------------------------------------
// opaque[i]: row i stops a ray -- it has min_count points and its fullest bin is not ignored (the histogram is read only when
// labels are ignored); lane 0 checks the origin as carve's hit kernel does
__global__ __launch_bounds__(256) void map_raycast_opaque_kernel(MapRaycastArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    float ox, oy, oz;
    u64 ko;
    if (!carve_origin(a, &ox, &oy, &oz, &ko)) a.res[kMapRange] = 1;
  }
  if (i >= a.n_map) return;
  bool opaque = (long long)a.rows.cnt[i] >= a.min_count;
  if (opaque && a.n_ignore > 0) {
    const uint32_t l = map_fullest_bin(a.rows.hist + (size_t)i * (size_t)a.stride, a.stride);
    for (int j = 0; j < a.n_ignore; ++j) opaque = opaque && a.ignore[j] != l;
  }
  a.opaque[i] = opaque ? 1 : 0;
}

// ray i's outputs (plain stores by the lane that owns it): the hit row `row` at walk index `step`, or row < 0 for none
__device__ __forceinline__ void raycast_store(const MapRaycastArgs& a, int i, int row, int step, int length, float ox, float oy,
                                              float oz) {
  float cx = 0.f, cy = 0.f, cz = 0.f;
  uint32_t label = 0u, count = 0u;
  double d2 = -1.0;
  if (row >= 0) {
    map_centroid(a.rows, row, &cx, &cy, &cz);
    count = a.rows.cnt[row];
    if (a.rows.hist) label = map_fullest_bin(a.rows.hist + (size_t)row * (size_t)a.stride, a.stride);
    const double dx = __dsub_rn((double)cx, (double)ox), dy = __dsub_rn((double)cy, (double)oy), dz = __dsub_rn((double)cz, (double)oz);
    d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
    a.visible[row] = 1;
  }
  a.orow[i] = row; a.ostep[i] = step; a.olength[i] = length;
  a.ox[i] = cx; a.oy[i] = cy; a.oz[i] = cz;
  a.olabel[i] = label; a.ocount[i] = count;
  a.orange_sq[i] = d2;
}

// The walk, dealt as carve's: a wave owns the rays [wave * kRaycastRaysPerWave, ...) and its idle lanes take the next ones in
// lane order.  A lane with a ray stands in voxel v_i with `left` = n + 1 - i voxels still to visit (this one included) and
// `skip` of them not to be tested; it tests the voxel (the map holds it and its row is opaque: the hit, and the lane falls
// idle), or steps on.  An end that casts no ray is answered by the lane that drew it.
__global__ __launch_bounds__(256) void map_raycast_walk_kernel(MapRaycastArgs a) {
  float ox, oy, oz;
  u64 ko;
  if (!carve_origin(a, &ox, &oy, &oz, &ko)) return;  // (the same in every lane; the host refuses the call)
  const int lane = threadIdx.x & 63;
  const long long first = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * kRaycastRaysPerWave;
  const int end = (int)std::min<long long>(first + kRaycastRaysPerWave, a.n);
  int next = (int)std::min<long long>(first, a.n);
  const u64* const keys = a.rows.key;
  const unsigned char* const opaque = a.opaque;
  const int n_map = a.n_map;
  const int lb0 = map_lower_bound(keys, n_map, ko);  // every ray starts in the origin's voxel
  const bool found0 = lb0 < n_map && keys[lb0] == ko;
  VoxelRay r;
  int left = 0, skip = 0, lb = 0, mine = -1;
  bool found = false;
  u64 rays = 0, steps = 0, hits = 0;
  for (;;) {
    const bool idle = left == 0;
    const u64 idle_mask = __ballot(idle);
    if (idle_mask == ~0ull && next >= end) break;
    int done = -1, done_row = -1, done_step = -1, done_length = -1;  // the ray this lane answers in this turn (at most one)
    if (idle) {
      const int i = next + __popcll(idle_mask & ((1ull << lane) - 1ull));
      if (i < end) {
        const double x = a.x[i], y = a.y[i], z = a.z[i];
        const float px = voxel_xform_row(a.M + 0, x, y, z);
        const float py = voxel_xform_row(a.M + 4, x, y, z);
        const float pz = voxel_xform_row(a.M + 8, x, y, z);
        u64 kp;
        done = i;  // (an end that casts no ray: length -1)
        if (voxel_key(px, py, pz, a.inv_leaf, &kp) && (!a.ranged || voxel_crop_keeps(px, py, pz, ox, oy, oz, a.range_sq))) {
          rays += 1;
          voxel_ray_begin(ox, oy, oz, ko, px, py, pz, kp, a.inv_leaf, &r);
          const int tests = r.n + 1 > a.start_margin ? r.n + 1 - a.start_margin : 0;  // the voxels a walk without a hit tests
          if (n_map == 0 || tests == 0) {  // nothing can stop it
            steps += (u64)tests;
            done_length = r.n;
          } else {
            done = -1;
            mine = i;
            left = r.n + 1;
            skip = a.start_margin;
            lb = lb0;
            found = found0;
          }
        }
      }
    }
    next = (int)std::min<long long>((long long)next + __popcll(idle_mask), end);
    if (left > 0) {
      const bool tested = skip == 0;
      steps += tested ? 1 : 0;
      if (tested && found && opaque[lb] != 0) {
        hits += 1;
        done = mine; done_row = lb; done_step = r.n + 1 - left; done_length = r.n;
        left = 0;
      } else {
        skip -= tested ? 0 : 1;
        left -= 1;
        if (left > 0) {
          const int axis = voxel_ray_step(&r);
          map_walk_lookup(keys, n_map, r, axis, &lb, &found);
        } else {
          done = mine; done_length = r.n;
        }
      }
    }
    if (done >= 0) raycast_store(a, done, done_row, done_step, done_length, ox, oy, oz);
  }
  rays = wave_sum(rays);
  steps = wave_sum(steps);
  hits = wave_sum(hits);
  if (lane == 0) {
    if (rays) atomicAdd(&a.stat[kRaycastRays], rays);
    if (steps) atomicAdd(&a.stat[kRaycastSteps], steps);
    if (hits) atomicAdd(&a.stat[kRaycastHits], hits);
  }
}

// the distinct rows hit: a ballot and one integer atomic a wave
__global__ __launch_bounds__(256) void map_raycast_visible_kernel(MapRaycastArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const u64 b = __ballot(i < a.n_map && a.visible[i] != 0);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&a.stat[kRaycastVisible], (u64)__popcll(b));
}

// ---- label fusion through the confusion matrix (kernels.h: MapFuseArgs) -------------------------------------------------------
constexpr int kFuseSlots = 4;  // classes a lane owns at most: ceil(255 / 64)

// One item -- a histogram row h (nullptr: none) and, added last, the single observation `own` (0: none) -- scored by the
// `width` neighbouring lanes it belongs to; lane j of them owns the classes j + 1, j + 1 + width, ...  EVERY lane of the wave
// calls this, from wave-uniform control flow (a ballot and shuffles inside); items differ between the groups of a wave.
// The groups' lanes read the row's bins `width` at a time, and the non-zero ones are walked in ascending r: every lane
// continues its classes' scores with (double)h[r] * L[r - 1][s - 1], product and sum rounded once each -- the per-class
// order of kernels.h whatever the lane mapping.  The arg-max (the smallest class among equals) goes through a butterfly;
// the denominator of the confidence is each lane's terms in ascending class, then a butterfly over lane distance 1, 2, 4 ...
// Returns whether there was evidence: a term was added and the best score is not -inf.
template <int SLOTS>
__device__ __forceinline__ bool map_fuse(const uint32_t* h, uint32_t own, const double* L, int C, int width, uint32_t* label,
                                         double* conf) {
  const int lane = threadIdx.x & 63, sub = lane & (width - 1), base = lane - sub;
  const u64 group = width == 64 ? ~0ull : ((1ull << width) - 1ull);
  double sc[SLOTS];
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) sc[k] = 0.0;
  bool added = false;
#pragma unroll
  for (int c = 0; c < SLOTS; ++c) {
    const int r0 = c * width;  // this round: the bins r0 + 1 ... r0 + width
    if (r0 >= C) break;
    const int r = r0 + sub + 1;
    const uint32_t v = (h && r <= C) ? h[r] : 0u;
    u64 live = (__ballot(v > 0u) >> base) & group;
    while (__any(live != 0ull)) {
      const int b = live ? __ffsll((unsigned long long)live) - 1 : 0;
      const uint32_t n = (uint32_t)__shfl((int)v, base + b, 64);
      if (live) {
        const double* row = L + (size_t)(r0 + b) * (size_t)C;
        const double w = (double)n;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
          const int s = sub + 1 + k * width;
          if (s <= C) sc[k] = __dadd_rn(sc[k], __dmul_rn(w, row[s - 1]));
        }
        added = true;
        live &= live - 1ull;
      }
    }
  }
  if (own >= 1u && own <= (uint32_t)C) {
    const double* row = L + (size_t)(own - 1u) * (size_t)C;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      const int s = sub + 1 + k * width;
      if (s <= C) sc[k] = __dadd_rn(sc[k], row[s - 1]);
    }
    added = true;
  }
  const double ninf = -__builtin_inf();
  double best = ninf;
  int best_s = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) {
    const int s = sub + 1 + k * width;
    if (s <= C && sc[k] > best) { best = sc[k]; best_s = s; }
  }
  for (int w = width >> 1; w > 0; w >>= 1) {
    const double os = __shfl_xor(best, w, 64);
    const int ol = __shfl_xor(best_s, w, 64);
    if (os > best || (os == best && ol < best_s)) { best = os; best_s = ol; }
  }
  const bool evidence = added && best > ninf;
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) {
    const int s = sub + 1 + k * width;
    if (s <= C) t = __dadd_rn(t, exp(sc[k] - best));
  }
  for (int w = 1; w < width; w <<= 1) t = __dadd_rn(t, __shfl_xor(t, w, 64));
  *label = evidence ? (uint32_t)best_s : 0u;
  *conf = evidence ? 1.0 / t : 0.0;
  return evidence;
}

// log cm where the lanes read it: a copy in LDS (SLOTS == 1: C <= kMapFuseLdsClasses) or the global array
template <int SLOTS>
__device__ __forceinline__ const double* map_fuse_stage(const MapFuseArgs& a, double* lds) {
  if (SLOTS != 1) return a.logcm;
  for (int e = threadIdx.x; e < a.C * a.C; e += 256) lds[e] = a.logcm[e];
  __syncthreads();
  return lds;
}

// the selected rows' posteriors: `width` lanes per row, 256 / width rows per workgroup and turn (no lane leaves early)
template <int SLOTS>
__global__ __launch_bounds__(256) void map_posterior_kernel(MapFuseArgs a, int width) {
  __shared__ double lds[SLOTS == 1 ? kMapFuseLdsClasses * kMapFuseLdsClasses : 1];
  const double* L = map_fuse_stage<SLOTS>(a, lds);
  const int n = a.res_in[kMapOut];
  const int per_block = 256 / width, mine = threadIdx.x / width;
  for (long long j0 = (long long)blockIdx.x * per_block; j0 < n; j0 += (long long)gridDim.x * per_block) {
    const long long j = j0 + mine;
    const bool valid = j < n;
    const uint32_t* h = valid ? a.rows.hist + (size_t)a.src_of[j] * (size_t)a.stride : nullptr;
    uint32_t lab;
    double cf;
    map_fuse<SLOTS>(h, 0u, L, a.C, width, &lab, &cf);
    if (valid && (threadIdx.x & (width - 1)) == 0) { a.olabel[j] = lab; a.oconf[j] = cf; }
  }
}

// per point of a scan: transform and key as map_key_kernel does (no crop), its voxel among the map's keys, the posterior of
// that row (when it has min_count points) with the point's own label added last; a label beyond the classes raises its flag
template <int SLOTS>
__global__ __launch_bounds__(256) void map_relabel_kernel(MapFuseArgs a, int width) {
  __shared__ double lds[SLOTS == 1 ? kMapFuseLdsClasses * kMapFuseLdsClasses : 1];
  const double* L = map_fuse_stage<SLOTS>(a, lds);
  const int per_block = 256 / width, mine = threadIdx.x / width;
  for (long long i0 = (long long)blockIdx.x * per_block; i0 < a.n; i0 += (long long)gridDim.x * per_block) {
    const long long i = i0 + mine;
    const bool valid = i < a.n;
    const uint32_t* h = nullptr;
    uint32_t own_label = 0u, own = 0u;
    if (valid) {
      const double x = a.x[i], y = a.y[i], z = a.z[i];
      const float px = voxel_xform_row(a.M + 0, x, y, z);
      const float py = voxel_xform_row(a.M + 4, x, y, z);
      const float pz = voxel_xform_row(a.M + 8, x, y, z);
      u64 k;
      if (voxel_key(px, py, pz, a.inv_leaf, &k)) {  // (beyond the key's range: not in the map)
        const int r = map_lower_bound(a.rows.key, a.n_map, k);
        if (r < a.n_map && a.rows.key[r] == k && (long long)a.rows.cnt[r] >= a.min_count) h = a.rows.hist + (size_t)r * (size_t)a.stride;
      }
      if (a.label) {
        own_label = a.label[i];
        if (a.include_own) {
          if (own_label > (uint32_t)a.C) a.res[kMapBadLabel] = 1; else own = own_label;
        }
      }
    }
    uint32_t lab;
    double cf;
    const bool evidence = map_fuse<SLOTS>(h, own, L, a.C, width, &lab, &cf);
    if (valid && (threadIdx.x & (width - 1)) == 0) { a.olabel[i] = evidence ? lab : own_label; a.oconf[i] = cf; }
  }
}

// workgroups for `items` scored `width` lanes each: eight turns a workgroup where there is that much (the LDS copy of log cm
// is paid once a workgroup), 2048 at the most
inline dim3 fuse_grid(long long items, int width) {
  const long long per_turn = 256 / width;
  return dim3((unsigned)std::max<long long>(1, std::min<long long>((items + per_turn * 8 - 1) / (per_turn * 8), 2048)));
}

inline dim3 map_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_map_keys(const MapKeyArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_key_kernel, map_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_lookup(const MapFoldArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_lookup_kernel, map_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_misses(const MapFoldArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_miss_kernel, map_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_scatter(const MapFoldArgs& a, hipStream_t st) {
  const long long rows = (long long)a.n_map + a.n_new;
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_scatter_kernel, map_grid(rows), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_move_hist(const uint32_t* from, uint32_t* to, const int* src_of, long long rows, int stride, hipStream_t st) {
  const long long total = rows * stride;
  if (total <= 0) return hipSuccess;
  const long long blocks = std::min<long long>((total + 255) / 256, 1 << 16);  // (the rest by the kernel's stride loop)
  hipLaunchKernelGGL(map_move_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, st, from, to, src_of, total, stride);
  return hipGetLastError();
}

hipError_t launch_map_fold(const MapFoldArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_fold_kernel, map_grid(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_select(const MapSelectArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_select_kernel, map_grid(a.n_map), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_prune(const MapSelectArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_prune_kernel, map_grid(a.n_map), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_extract(const MapSelectArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_extract_kernel, map_grid(a.n_map), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_carve_hits(const MapCarveArgs& a, hipStream_t st) {
  if (a.n < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(map_carve_hit_kernel, map_grid(std::max(a.n, 1)), dim3(256), 0, st, a);  // (n = 0: the origin's check alone)
  return hipGetLastError();
}

hipError_t launch_map_carve_walk(const MapCarveArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  const long long per_block = 4 * kCarveRaysPerWave;  // four waves a workgroup
  hipLaunchKernelGGL(map_carve_walk_kernel, dim3((unsigned)((a.n + per_block - 1) / per_block)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_carve_select(const MapCarveSelectArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  if (a.n_protect < 0 || a.n_protect > kMapMaxProtect || (a.n_protect > 0 && !a.hist)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(map_carve_select_kernel, map_grid(a.n_map), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_raycast_opaque(const MapRaycastArgs& a, hipStream_t st) {
  if (a.n_map < 0 || a.n_ignore < 0 || a.n_ignore > kMapMaxIgnore || (a.n_ignore > 0 && !a.rows.hist)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(map_raycast_opaque_kernel, map_grid(std::max(a.n_map, 1)), dim3(256), 0, st, a);  // (n_map = 0: the origin's check alone)
  return hipGetLastError();
}

hipError_t launch_map_raycast_walk(const MapRaycastArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  const long long per_block = 4 * kRaycastRaysPerWave;  // four waves a workgroup
  hipLaunchKernelGGL(map_raycast_walk_kernel, dim3((unsigned)((a.n + per_block - 1) / per_block)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_raycast_visible(const MapRaycastArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_raycast_visible_kernel, map_grid(a.n_map), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_posterior(const MapFuseArgs& a, hipStream_t st) {
  if (a.n_map <= 0) return hipSuccess;
  if (a.C < 1 || a.C > 255 || a.stride != a.C + 1) return hipErrorInvalidValue;
  const int width = map_fuse_width(a.C);
  if (a.C <= kMapFuseLdsClasses) hipLaunchKernelGGL(map_posterior_kernel<1>, fuse_grid(a.n_map, width), dim3(256), 0, st, a, width);
  else hipLaunchKernelGGL(map_posterior_kernel<kFuseSlots>, fuse_grid(a.n_map, width), dim3(256), 0, st, a, width);
  return hipGetLastError();
}

hipError_t launch_map_relabel(const MapFuseArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (a.C < 1 || a.C > 255 || a.stride != a.C + 1) return hipErrorInvalidValue;
  const int width = map_fuse_width(a.C);
  if (a.C <= kMapFuseLdsClasses) hipLaunchKernelGGL(map_relabel_kernel<1>, fuse_grid(a.n, width), dim3(256), 0, st, a, width);
  else hipLaunchKernelGGL(map_relabel_kernel<kFuseSlots>, fuse_grid(a.n, width), dim3(256), 0, st, a, width);
  return hipGetLastError();
}

}  // namespace sicp
