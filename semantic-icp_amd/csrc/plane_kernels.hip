// plane_kernels.hip -- sicp_segment_planes: RANSAC plane extraction of one cloud (driver: plane.cpp; the rules: include/sicp.h,
// "planes of a cloud").  Per round: the candidates not yet assigned are compacted in ascending caller index, a lane per
// hypothesis draws its three samples from its own SplitMix64 states and forms the plane, the score kernel -- candidates x
// hypotheses, the hot one -- writes every hypothesis' inlier count per tile of candidates with plain stores, a sum over the tiles
// and an argmax pick the winner, and the membership pass, the tree sums, the one-lane Jacobi fit and the re-selection make the
// plane.  Counts are integers, every float sum runs over a binary tree of fixed shape, no float atomics: every byte is
// independent of the launch shapes.  A kernel returns at once when the call has ended (ctl->done).
#include <hip/hip_runtime.h>

#include "device_geometry.hpp"
#include "kernels.h"

#pragma clang fp contract(off)

namespace sicp {
namespace {

__device__ __forceinline__ int finite_of(const PlaneArgs& a, int i) { return a.finv ? a.finv[i] : i; }

// rule 3: e e <= (t t) nn with d = p - a in double, e = (nx dx + ny dy) + nz dz; ten operations, each rounded on its own
__device__ __forceinline__ bool plane_inlier(double px, double py, double pz, double ax, double ay, double az, double nx, double ny,
                                             double nz, double thr) {
  const double dx = __dsub_rn(px, ax), dy = __dsub_rn(py, ay), dz = __dsub_rn(pz, az);
  const double e = __dadd_rn(__dadd_rn(__dmul_rn(nx, dx), __dmul_rn(ny, dy)), __dmul_rn(nz, dz));
  return __dmul_rn(e, e) <= thr;
}

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
}

// rule 1: the candidates
__global__ __launch_bounds__(256) void plane_init_kernel(PlaneArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool cand = false;
  if (i < a.n_caller) {
    const int f = finite_of(a, i);
    cand = f >= 0 && (a.mask == nullptr || a.mask[i] != 0);
    if (cand && a.labels) {
      const uint32_t l = a.label[f];
      for (int k = 0; k < a.n_ignore; ++k) cand = cand && a.ignore[k] != l;
    }
    a.state[i] = cand ? -1 : -2;
  }
  const int c = __syncthreads_count(cand ? 1 : 0);
  if (threadIdx.x == 0 && c) atomicAdd(&a.ctl->n_candidates, c);
}

__global__ __launch_bounds__(256) void plane_flag_kernel(PlaneArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_caller || a.ctl->done) return;
  a.flag[i] = a.state[i] == -1 ? 1 : 0;
}

__global__ __launch_bounds__(256) void plane_compact_kernel(PlaneArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_caller || a.ctl->done) return;
  const int fl = a.flag[i], p = a.pos[i];
  if (fl) {
    const int f = finite_of(a, i);
    a.cx[p] = a.x[f]; a.cy[p] = a.y[f]; a.cz[p] = a.z[f];
  }
  if (i == a.n_caller - 1) a.ctl->m = p + fl;
}

// rule 2.  Draw number k of the stream is the output of the state seed + (k + 1) * 0x9E3779B97F4A7C15.
__device__ __forceinline__ unsigned long long splitmix_draw(unsigned long long seed, unsigned long long k) {
  unsigned long long z = seed + (k + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void plane_sample_kernel(PlaneArgs a, int round) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= a.H || a.ctl->done) return;
  const int m = a.ctl->m;
  if (m < 3) return;
  int s[3];
  for (int k = 0; k < 3; ++k) {
    const unsigned long long z = splitmix_draw(a.seed, 3ull * ((unsigned long long)round * (unsigned long long)a.H + (unsigned long long)h) + (unsigned long long)k);
    const double u = __dmul_rn((double)(z >> 11), 0x1.0p-53);
    const long long j = (long long)floor(__dmul_rn((double)m, u));
    s[k] = (int)(j < m ? j : m - 1);
  }
  PlaneHyp r;
  r.ax = (double)a.cx[s[0]]; r.ay = (double)a.cy[s[0]]; r.az = (double)a.cz[s[0]];
  const double e1x = __dsub_rn((double)a.cx[s[1]], r.ax), e1y = __dsub_rn((double)a.cy[s[1]], r.ay), e1z = __dsub_rn((double)a.cz[s[1]], r.az);
  const double e2x = __dsub_rn((double)a.cx[s[2]], r.ax), e2y = __dsub_rn((double)a.cy[s[2]], r.ay), e2z = __dsub_rn((double)a.cz[s[2]], r.az);
  r.nx = __dsub_rn(__dmul_rn(e1y, e2z), __dmul_rn(e1z, e2y));
  r.ny = __dsub_rn(__dmul_rn(e1z, e2x), __dmul_rn(e1x, e2z));
  r.nz = __dsub_rn(__dmul_rn(e1x, e2y), __dmul_rn(e1y, e2x));
  r.nn = dot3(r.nx, r.ny, r.nz, r.nx, r.ny, r.nz);
  bool valid = s[0] != s[1] && s[0] != s[2] && s[1] != s[2] && r.nn > 0.0;
  if (valid && a.has_axis) {
    const double na = dot3(r.nx, r.ny, r.nz, a.axis[0], a.axis[1], a.axis[2]);
    valid = __dmul_rn(na, na) >= __dmul_rn(__dmul_rn(a.mc2, r.nn), a.aa);
  }
  r.thr = valid ? __dmul_rn(a.tt, r.nn) : -1.0;
  a.hyp[h] = r;
}

// rule 3, the hot kernel: workgroup (x, y) tests the candidates of tile x against the hypotheses of group y.  A lane keeps
// kPlaneLanePoints candidates in registers as doubles; the hypothesis index is uniform over the workgroup, so its seven doubles
// are LDS broadcasts; a wave's count is the population of its ballots, lane 0 stores it, and after the loop a lane per
// hypothesis adds the four waves' counts and stores the tile's count: no atomics, and nothing is read back.
__global__ __launch_bounds__(256) void plane_score_kernel(PlaneArgs a) {
  __shared__ PlaneHyp sh[kPlaneHypGroup];
  __shared__ int wc[4][kPlaneHypGroup];
  if (a.ctl->done) return;
  const int m = a.ctl->m;
  const int first = (int)blockIdx.x * kPlaneTile;
  if (m < 3 || first >= m) return;
  const int t = threadIdx.x, h0 = (int)blockIdx.y * kPlaneHypGroup;
  const int G = min(kPlaneHypGroup, a.H - h0);
  if (t < G) sh[t] = a.hyp[h0 + t];
  // (a slot past the round's candidates holds NaN: e e <= thr is false for it, and the loop needs no mask)
  double px[kPlaneLanePoints], py[kPlaneLanePoints], pz[kPlaneLanePoints];
#pragma unroll
  for (int k = 0; k < kPlaneLanePoints; ++k) {
    const int j = first + k * 256 + t;
    const int jj = j < m ? j : first;
    px[k] = j < m ? (double)a.cx[jj] : __longlong_as_double(0x7ff8000000000000ll);
    py[k] = (double)a.cy[jj]; pz[k] = (double)a.cz[jj];
  }
  __syncthreads();
  const int w = t >> 6;
  for (int hl = 0; hl < G; ++hl) {
    const double ax = sh[hl].ax, ay = sh[hl].ay, az = sh[hl].az, nx = sh[hl].nx, ny = sh[hl].ny, nz = sh[hl].nz, thr = sh[hl].thr;
    int c = 0;
#pragma unroll
    for (int k = 0; k < kPlaneLanePoints; ++k)
      c += __popcll(__ballot(plane_inlier(px[k], py[k], pz[k], ax, ay, az, nx, ny, nz, thr)));
    if ((t & 63) == 0) wc[w][hl] = c;
  }
  __syncthreads();
  if (t < G) a.partial[(size_t)blockIdx.x * (size_t)a.H + (size_t)(h0 + t)] = (wc[0][t] + wc[1][t]) + (wc[2][t] + wc[3][t]);
}

// a hypothesis' count: sixteen lanes share its tiles, sixteen hypotheses a workgroup (integers: the order decides nothing)
__global__ __launch_bounds__(256) void plane_total_kernel(PlaneArgs a) {
  __shared__ int part[16][17];
  const int hl = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int h = blockIdx.x * 16 + hl;
  if (a.ctl->done) return;
  const int m = a.ctl->m;
  if (m < 3) return;
  const int tiles = (m + kPlaneTile - 1) / kPlaneTile;
  int s = 0;
  if (h < a.H)
    for (int k = slice; k < tiles; k += 16) s += a.partial[(size_t)k * (size_t)a.H + (size_t)h];
  part[slice][hl] = s;
  __syncthreads();
  if (slice == 0 && h < a.H) {
    int sum = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) sum += part[k][hl];
    a.total[h] = sum;
  }
}

// rule 3, the winner: the largest count among the valid hypotheses, ties to the smallest h -- the largest key count << 32 |
// ~h -- by one workgroup; its lane 0 ends the call or makes the winner the model of the membership pass.
__global__ __launch_bounds__(256) void plane_winner_kernel(PlaneArgs a, int round) {
  __shared__ unsigned long long key[256];
  __shared__ int inv[256];
  const int t = threadIdx.x;
  const int ended = a.ctl->done, m = a.ctl->m;
  __syncthreads();  // (every lane has read them before lane 0 writes)
  if (ended) return;
  if (m < 3) {
    if (t == 0) a.ctl->done = 1;
    return;
  }
  unsigned long long best = 0ull;
  int bad = 0;
  for (int h = t; h < a.H; h += 256) {
    if (a.hyp[h].thr >= 0.0) {
      const unsigned long long k = ((unsigned long long)(unsigned)a.total[h] << 32) | (unsigned long long)(0xffffffffu - (unsigned)h);
      best = k > best ? k : best;
    } else {
      ++bad;
    }
  }
  key[t] = best; inv[t] = bad;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      key[t] = key[t + w] > key[t] ? key[t + w] : key[t];
      inv[t] += inv[t + w];
    }
    __syncthreads();
  }
  if (t != 0) return;
  PlaneCtl* c = a.ctl;
  c->rounds += 1;
  c->n_invalid += inv[0];
  const int count = (int)(key[0] >> 32), h = (int)(0xffffffffu - (unsigned)(key[0] & 0xffffffffull));
  if (key[0] == 0ull || count < a.min_inliers) {
    c->done = 1;
    return;
  }
  c->model = a.hyp[h];
  c->cnt = 0;
  a.rec[round].hyp_index = h;
  a.rec[round].hyp_count = count;
}

// the model's inliers among the candidates not yet assigned: the winner's (rule 4; rule 5, first pass) or the fit's (rule 5,
// the re-selection)
__global__ __launch_bounds__(256) void plane_member_kernel(PlaneArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (a.ctl->done) return;
  bool in = false;
  if (i < a.n_caller) {
    if (a.state[i] == -1) {
      const PlaneHyp& M = a.ctl->model;
      const int f = finite_of(a, i);
      in = plane_inlier((double)a.x[f], (double)a.y[f], (double)a.z[f], M.ax, M.ay, M.az, M.nx, M.ny, M.nz, M.thr);
    }
    a.member[i] = in ? 1 : 0;
  }
  const int c = __syncthreads_count(in ? 1 : 0);
  if (threadIdx.x == 0 && c) atomicAdd(&a.ctl->cnt, c);
}

// rule 5, the sums (the filter's rule 3): one workgroup reduces an aligned run of kPlaneTreeRun entries as the perfect binary
// tree over them, level by level; entries past `count` and entries of points that are no members are +0.0.  The same kernel
// over the partial sums continues the tree.  LEAF 0: the entries are partial sums, NCH channels `count` apart.  LEAF 1: the
// members' x y z and e e (4 channels).  LEAF 2: the six products of (p - centroid), centroid = the first sums / the count.
// A tree taller than the rule's (2^ceil(log2 n_points) leaves) only adds +0.0 to its result; the one-lane kernels add +0.0
// once more, so that a sum of nothing but -0.0 is +0.0 under every shape.
template <int LEAF, int NCH>
__global__ __launch_bounds__(256) void plane_tree_kernel(PlaneArgs a, const double* in, int count, double* out) {
  static_assert(kPlaneTreeRun == 512, "two entries per lane of a 256-lane workgroup");
  __shared__ double s[NCH][256];
  if (a.ctl->done) return;
  const int t = threadIdx.x;
  const long long base = (long long)blockIdx.x * kPlaneTreeRun + 2 * t;
  double v[NCH][2];
  double cx = 0.0, cy = 0.0, cz = 0.0;
  if (LEAF == 2) {
    const double cnt = (double)a.ctl->cnt;
    cx = __ddiv_rn(__dadd_rn(a.sum_f[0], 0.0), cnt); cy = __ddiv_rn(__dadd_rn(a.sum_f[1], 0.0), cnt); cz = __ddiv_rn(__dadd_rn(a.sum_f[2], 0.0), cnt);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) v[c][k] = 0.0;
    const long long i = base + k;
    if (i >= count) continue;
    if (LEAF == 0) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) v[c][k] = in[(size_t)c * (size_t)count + (size_t)i];
    } else if (a.member[i]) {
      const int f = finite_of(a, (int)i);
      const double x = (double)a.x[f], y = (double)a.y[f], z = (double)a.z[f];
      if (LEAF == 1) {
        const PlaneHyp& M = a.ctl->model;
        const double e = dot3(M.nx, M.ny, M.nz, __dsub_rn(x, M.ax), __dsub_rn(y, M.ay), __dsub_rn(z, M.az));
        v[0][k] = x; v[1][k] = y; v[2][k] = z; v[3 % NCH][k] = __dmul_rn(e, e);
      } else {
        const double dx = __dsub_rn(x, cx), dy = __dsub_rn(y, cy), dz = __dsub_rn(z, cz);
        v[0][k] = __dmul_rn(dx, dx); v[1 % NCH][k] = __dmul_rn(dy, dx); v[2 % NCH][k] = __dmul_rn(dy, dy);
        v[3 % NCH][k] = __dmul_rn(dz, dx); v[4 % NCH][k] = __dmul_rn(dz, dy); v[5 % NCH][k] = __dmul_rn(dz, dz);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) s[c][t] = __dadd_rn(v[c][0], v[c][1]);
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    double p[NCH];
    if (t < w) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) p[c] = __dadd_rn(s[c][2 * t], s[c][2 * t + 1]);
    }
    __syncthreads();
    if (t < w) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) s[c][t] = p[c];
    }
    __syncthreads();
  }
  if (t < NCH) out[(size_t)t * (size_t)gridDim.x + (size_t)blockIdx.x] = s[t][0];
}

// rules 4 and 5, the orientation: with an axis so that n . axis > 0; without one, or at n . axis == 0, so that d > 0, and at
// d == 0 so that the first non-zero of (nz, ny, nx) is positive.  Negation is exact.
__device__ void plane_orient(const PlaneArgs& a, double (&c)[4]) {
  double s = 0.0;
  if (a.has_axis) s = dot3(c[0], c[1], c[2], a.axis[0], a.axis[1], a.axis[2]);
  bool flip = s < 0.0;
  if (s == 0.0) {
    if (c[3] != 0.0) flip = c[3] < 0.0;
    else if (c[2] != 0.0) flip = c[2] < 0.0;
    else if (c[1] != 0.0) flip = c[1] < 0.0;
    else flip = c[0] < 0.0;
  }
  if (flip) { c[0] = -c[0]; c[1] = -c[1]; c[2] = -c[2]; c[3] = -c[3]; }
}

// rule 5, the fit, by one lane: the centroid of the winner's inliers, the cyclic Jacobi of the covariance kernel on the six
// sums, the column of smallest |eigenvalue|; the fit becomes the model of the re-selection
__global__ void plane_fit_kernel(PlaneArgs a, int round) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || a.ctl->done) return;
  PlaneCtl* ctl = a.ctl;
  const double cnt = (double)ctl->cnt;
  const double cx = __ddiv_rn(__dadd_rn(a.sum_f[0], 0.0), cnt), cy = __ddiv_rn(__dadd_rn(a.sum_f[1], 0.0), cnt), cz = __ddiv_rn(__dadd_rn(a.sum_f[2], 0.0), cnt);
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  A[0][0] = __dadd_rn(a.sum_c[0], 0.0);
  A[1][0] = A[0][1] = __dadd_rn(a.sum_c[1], 0.0);
  A[1][1] = __dadd_rn(a.sum_c[2], 0.0);
  A[2][0] = A[0][2] = __dadd_rn(a.sum_c[3], 0.0);
  A[2][1] = A[1][2] = __dadd_rn(a.sum_c[4], 0.0);
  A[2][2] = __dadd_rn(a.sum_c[5], 0.0);
  for (int sweep = 0; sweep < 30; ++sweep) {  // (cov_body's sweep limit, stopping rule and column choice: feature_kernels.hip)
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off <= 1e-300 || off <= 1e-34 * dia) break;
    jacobi_rotate(A, V, 0, 1);
    jacobi_rotate(A, V, 0, 2);
    jacobi_rotate(A, V, 1, 2);
  }
  const double e0 = fabs(A[0][0]), e1 = fabs(A[1][1]), e2 = fabs(A[2][2]);
  int col = 0;
  double em = e0;
  if (e1 <= em) { em = e1; col = 1; }
  if (e2 <= em) { em = e2; col = 2; }
  double c[4];
  c[0] = col == 0 ? V[0][0] : (col == 1 ? V[0][1] : V[0][2]);
  c[1] = col == 0 ? V[1][0] : (col == 1 ? V[1][1] : V[1][2]);
  c[2] = col == 0 ? V[2][0] : (col == 1 ? V[2][1] : V[2][2]);
  c[3] = -dot3(c[0], c[1], c[2], cx, cy, cz);
  plane_orient(a, c);
  PlaneHyp M;
  M.ax = cx; M.ay = cy; M.az = cz;
  M.nx = c[0]; M.ny = c[1]; M.nz = c[2];
  M.nn = dot3(c[0], c[1], c[2], c[0], c[1], c[2]);
  M.thr = __dmul_rn(a.tt, M.nn);
  ctl->model = M;
  ctl->cnt = 0;
  for (int k = 0; k < 4; ++k) a.rec[round].coeff[k] = c[k];
}

// rule 6, the plane's record, by one lane: count, centroid and rms of the final members; with refine = 0 the winner's
// coefficients
__global__ void plane_record_kernel(PlaneArgs a, int round) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || a.ctl->done) return;
  PlaneCtl* ctl = a.ctl;
  PlaneRec& R = a.rec[round];
  const PlaneHyp M = ctl->model;
  if (!a.refine) {
    const double len = __dsqrt_rn(M.nn);
    double c[4];
    c[0] = __ddiv_rn(M.nx, len); c[1] = __ddiv_rn(M.ny, len); c[2] = __ddiv_rn(M.nz, len);
    c[3] = -dot3(c[0], c[1], c[2], M.ax, M.ay, M.az);
    plane_orient(a, c);
    for (int k = 0; k < 4; ++k) R.coeff[k] = c[k];
  }
  const double cnt = (double)ctl->cnt;
  for (int k = 0; k < 3; ++k) R.centroid[k] = __ddiv_rn(__dadd_rn(a.sum_f[k], 0.0), cnt);
  const double q = __ddiv_rn(__dadd_rn(a.sum_f[3], 0.0), M.nn);
  R.rms = __dsqrt_rn(__ddiv_rn(q > 0.0 ? q : 0.0, cnt));
  R.count = ctl->cnt;
  R.pad_ = 0;
  ctl->n_planes = round + 1;
  ctl->n_assigned += ctl->cnt;
}

__global__ __launch_bounds__(256) void plane_assign_kernel(PlaneArgs a, int round) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_caller || a.ctl->done) return;
  if (a.member[i]) a.state[i] = round;
}

inline dim3 grid256(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

#define SICP_PLANE_POINTS(fn, kernel)                                                   \
  hipError_t fn(const PlaneArgs& a, hipStream_t st) {                                   \
    if (a.n_caller <= 0) return hipSuccess;                                             \
    hipLaunchKernelGGL(kernel, grid256(a.n_caller), dim3(256), 0, st, a);               \
    return hipGetLastError();                                                           \
  }
SICP_PLANE_POINTS(launch_plane_init, plane_init_kernel)
SICP_PLANE_POINTS(launch_plane_flags, plane_flag_kernel)
SICP_PLANE_POINTS(launch_plane_compact, plane_compact_kernel)
SICP_PLANE_POINTS(launch_plane_members, plane_member_kernel)
#undef SICP_PLANE_POINTS

hipError_t launch_plane_sample(const PlaneArgs& a, int round, hipStream_t st) {
  hipLaunchKernelGGL(plane_sample_kernel, grid256(a.H), dim3(256), 0, st, a, round);
  return hipGetLastError();
}

// the candidate count stays on the device: the grid covers every caller index, and a tile past the round's candidates returns
hipError_t launch_plane_score(const PlaneArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)plane_tiles(a.n_caller), (unsigned)((a.H + kPlaneHypGroup - 1) / kPlaneHypGroup));
  hipLaunchKernelGGL(plane_score_kernel, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_plane_winner(const PlaneArgs& a, int round, hipStream_t st) {
  hipLaunchKernelGGL(plane_total_kernel, dim3((unsigned)((a.H + 15) / 16)), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(plane_winner_kernel, dim3(1), dim3(256), 0, st, a, round);
  return hipGetLastError();
}

// level l reduces cnt_l entries to cnt_(l+1) = ceil(cnt_l / kPlaneTreeRun) sums per channel; the levels lie one before the
// other in the buffer, so that the last -- one sum per channel -- begins it
hipError_t launch_plane_tree_sums(const PlaneArgs& a, int products, hipStream_t st) {
  double* buf = products ? a.sum_c : a.sum_f;
  size_t end = plane_tree_doubles(a.n_caller);
  const double* in = nullptr;
  int cnt = a.n_caller;
  for (bool leaf = true;; leaf = false) {
    const int blocks = (cnt + kPlaneTreeRun - 1) / kPlaneTreeRun;
    end -= 6 * (size_t)blocks;
    double* out = buf + end;
    const dim3 grid((unsigned)blocks), wg(256);
    if (leaf && products) hipLaunchKernelGGL((plane_tree_kernel<2, 6>), grid, wg, 0, st, a, in, cnt, out);
    else if (leaf) hipLaunchKernelGGL((plane_tree_kernel<1, 4>), grid, wg, 0, st, a, in, cnt, out);
    else if (products) hipLaunchKernelGGL((plane_tree_kernel<0, 6>), grid, wg, 0, st, a, in, cnt, out);
    else hipLaunchKernelGGL((plane_tree_kernel<0, 4>), grid, wg, 0, st, a, in, cnt, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    in = out;
    cnt = blocks;
    if (blocks == 1) return hipSuccess;
  }
}

hipError_t launch_plane_fit(const PlaneArgs& a, int round, hipStream_t st) {
  hipLaunchKernelGGL(plane_fit_kernel, dim3(1), dim3(64), 0, st, a, round);
  return hipGetLastError();
}

hipError_t launch_plane_record(const PlaneArgs& a, int round, hipStream_t st) {
  hipLaunchKernelGGL(plane_record_kernel, dim3(1), dim3(64), 0, st, a, round);
  return hipGetLastError();
}

hipError_t launch_plane_assign(const PlaneArgs& a, int round, hipStream_t st) {
  if (a.n_caller <= 0) return hipSuccess;
  hipLaunchKernelGGL(plane_assign_kernel, grid256(a.n_caller), dim3(256), 0, st, a, round);
  return hipGetLastError();
}

}  // namespace sicp
