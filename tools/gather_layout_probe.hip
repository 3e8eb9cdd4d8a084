// gather_layout_probe.hip -- does the L1 / texture path price the accumulate kernel's target gathers by the LINES they touch?
// ("dense gathers"; the sequel of tools/r06/gather_probe.hip: the same records, the same indices, the same loop.)
// Every lane keeps fetching its own 4 records as unchanged pieces; what changes is where the pieces lie:
//   0  product pattern of rounds 2-6: 16 + 16 + 4 bytes of a 48-byte record (a piece shares its 64-byte line with at most one
//      other record)                                                                                          (12 instr / step)
//   4  variant 0's instructions with every lane on the SAME record (one line per instruction: the floor)
//   5  16 + 16 + 4 bytes from three dense arrays [n] x 16 | [n] x 16 | [n] x 4 (4 / 4 / 16 consecutive targets per line); the
//      address is a uniform base + a 32-bit lane offset                                                       (12 instr / step)
//   6  three 12-byte pieces {nx, x} | {ny, y} | {nz, z} from three dense arrays [n] x 12 (dwordx3 LDS-DMA; 5.3 targets per
//      line, every piece the same width)                                                                      (12 instr / step)
// Variant 0 runs first and last: the spread of the two is the noise of the box.  Every variant reads the staged bytes back
// from LDS and folds them into a checksum.  usage: gather_layout_probe [points] [reps]   (prints one JSON line)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <random>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)
#define GL __attribute__((address_space(1)))
#define LD __attribute__((address_space(3)))
typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

template <int V>
__global__ __launch_bounds__(256, 2) void probe(const int* __restrict__ idx, const char* __restrict__ rec48, const char* __restrict__ dense36,
                                                const char* __restrict__ dense12, int n_points, int steps_total, double* out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  LD char* stage = (LD char*)smem + wave * 16384;
  const int waves = gridDim.x * 4, w = blockIdx.x * 4 + wave;
  const size_t n = (size_t)n_points;
  const GL char* d0 = (const GL char*)dense36;
  const GL char* d1 = d0 + 16 * n;
  const GL char* d2 = d0 + 32 * n;
  const GL char* t0 = (const GL char*)dense12;
  const GL char* t1 = t0 + 12 * n;
  const GL char* t2 = t0 + 24 * n;
  double acc = 0.0;
  for (int step = w; step < steps_total; step += waves) {
    const int base = (step * 64) % n_points;  // this wave-step's 64 source points
    const int4 j = *reinterpret_cast<const int4*>(idx + 4 * (size_t)min(base + lane, n_points - 1));  // (the last step of a lap is ragged)
    const int jj[4] = {V == 4 ? 0 : j.x, V == 4 ? 0 : j.y, V == 4 ? 0 : j.z, V == 4 ? 0 : j.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (V == 0 || V == 4) {
        const char* p = rec48 + 48 * (size_t)jj[c];
        __builtin_amdgcn_global_load_lds((const GL void*)p, (LD void*)(stage + c * 2304), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const GL void*)(p + 16), (LD void*)(stage + c * 2304 + 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const GL void*)(p + 32), (LD void*)(stage + c * 2304 + 2048), 4, 0, 0);
      } else if (V == 5) {
        const unsigned o16 = (unsigned)jj[c] << 4, o4 = (unsigned)jj[c] << 2;
        __builtin_amdgcn_global_load_lds((const GL void*)(d0 + o16), (LD void*)(stage + c * 2304), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const GL void*)(d1 + o16), (LD void*)(stage + c * 2304 + 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const GL void*)(d2 + o4), (LD void*)(stage + c * 2304 + 2048), 4, 0, 0);
      } else {
        const unsigned o12 = (unsigned)jj[c] * 12u;
        __builtin_amdgcn_global_load_lds((const GL void*)(t0 + o12), (LD void*)(stage + c * 2304), 12, 0, 0);
        __builtin_amdgcn_global_load_lds((const GL void*)(t1 + o12), (LD void*)(stage + c * 2304 + 768), 12, 0, 0);
        __builtin_amdgcn_global_load_lds((const GL void*)(t2 + o12), (LD void*)(stage + c * 2304 + 1536), 12, 0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (V == 6) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const LD float* q = (const LD float*)(stage + c * 2304 + 768 * k + 12 * lane);
          acc += (double)(q[0] + q[1] + q[2]);
        }
      } else {
        const v2d a = *(const LD v2d*)(stage + c * 2304 + 16 * lane);
        const v4f b = *(const LD v4f*)(stage + c * 2304 + 1024 + 16 * lane);
        const float z = *(const LD float*)(stage + c * 2304 + 2048 + 4 * lane);
        acc += a.x + a.y + (double)(b.x + b.y + b.z + b.w + z);
      }
    }
  }
  if (acc == 1.2345e300) out[0] = acc;
}

template <int V>
static float run(const int* idx, const char* r48, const char* d36, const char* d12, int n, int steps, double* out, int reps) {
  CK(hipFuncSetAttribute((const void*)probe<V>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int k = 0; k < 2; ++k) hipLaunchKernelGGL((probe<V>), dim3(512), dim3(256), 65536, 0, idx, r48, d36, d12, n, steps, out);
  CK(hipEventRecord(e0, 0));
  for (int k = 0; k < reps; ++k) hipLaunchKernelGGL((probe<V>), dim3(512), dim3(256), 65536, 0, idx, r48, d36, d12, n, steps, out);
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  return 1e3f * ms / reps;
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 100000, reps = argc > 2 ? std::atoi(argv[2]) : 20;
  if (n < 64 || n > (1 << 24) || reps < 1) { std::fprintf(stderr, "points in [64, 2^24], reps >= 1\n"); return 2; }
  const int pairs = 64;  // wave-steps of a launch: pairs x n / 64
  const int steps = (int)((long long)pairs * n / 64);
  // neighbour indices like a K = 4 search between curve-ordered clouds: near the source's own position, shared with its
  // neighbours (the generator of tools/r06/gather_probe.hip, same seed)
  std::mt19937 rng(7);
  std::vector<int> idx((size_t)4 * n);
  std::normal_distribution<float> jitter(0.f, 6.f);
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 4; ++c) {
      int j = i + (int)std::lround(jitter(rng)) + 3 * c;
      idx[4 * (size_t)i + c] = j < 0 ? 0 : (j >= n ? n - 1 : j);
    }
  int* d_idx; char *r48, *d36, *d12; double* out;
  CK(hipMalloc(&d_idx, sizeof(int) * idx.size() + 4096));
  CK(hipMalloc(&r48, (size_t)48 * n + 4096)); CK(hipMalloc(&d36, (size_t)36 * n + 4096)); CK(hipMalloc(&d12, (size_t)36 * n + 4096));
  CK(hipMalloc(&out, 64));
  CK(hipMemcpy(d_idx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice));
  CK(hipMemset(r48, 0, (size_t)48 * n)); CK(hipMemset(d36, 0, (size_t)36 * n)); CK(hipMemset(d12, 0, (size_t)36 * n));
  const float t0 = run<0>(d_idx, r48, d36, d12, n, steps, out, reps);
  const float t4 = run<4>(d_idx, r48, d36, d12, n, steps, out, reps);
  const float t5 = run<5>(d_idx, r48, d36, d12, n, steps, out, reps);
  const float t6 = run<6>(d_idx, r48, d36, d12, n, steps, out, reps);
  const float t0b = run<0>(d_idx, r48, d36, d12, n, steps, out, reps);
  const double recs = (double)steps * 256;
  std::printf("{\"points\": %d, \"wave_steps\": %d, \"records_gathered\": %.0f, \"reps\": %d, \"us_per_launch\": {\"v0_product_16_16_4_of_48B_records\": %.1f, "
              "\"v0_again_at_the_end\": %.1f, \"v4_all_lanes_one_record\": %.1f, \"v5_dense_arrays_16_16_4\": %.1f, \"v6_dense_arrays_3x12\": %.1f}, "
              "\"ns_per_1000_records\": {\"v0\": %.2f, \"v0_again\": %.2f, \"v4\": %.2f, \"v5\": %.2f, \"v6\": %.2f}, "
              "\"relative_to_v0\": {\"v4\": %.3f, \"v5\": %.3f, \"v6\": %.3f}}\n",
              n, steps, recs, reps, t0, t0b, t4, t5, t6, 1e6 * t0 / recs, 1e6 * t0b / recs, 1e6 * t4 / recs, 1e6 * t5 / recs, 1e6 * t6 / recs,
              t4 / t0, t5 / t0, t6 / t0);
  CK(hipFree(d_idx)); CK(hipFree(r48)); CK(hipFree(d36)); CK(hipFree(d12)); CK(hipFree(out));
  return 0;
}
