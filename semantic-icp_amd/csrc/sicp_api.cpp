// sicp_api.cpp -- the C ABI of include/sicp.h (handles, clouds, align, test / bench hooks) on top of the engine
// (engine.hpp).  There is no CPU fallback: every stage runs on the GPU and every entry point fails with
// SICP_ERR_NO_DEVICE / SICP_ERR_HIP if it cannot.  Registration streams: streams.cpp.
#include "bootstrap.hpp"
#include "engine.hpp"

using namespace sicp::host;

// align() with the outer AND the inner loop on the host (lm_on_device = 0; a pair with caller covariances of general form)
int sicp::host::align_host_loop(sicp_context* h, const double* init_qt, double* out_qt, int32_t* outer_iters, sicp_stats* stats) {
  const sicp_params& P = h->params;
  const double t_begin = now_ms();
  h->epoch = next_epoch();
  SICPCHECK(align_begin(h, stats != nullptr));
  OuterState o;
  std::memcpy(o.cur, init_qt, sizeof o.cur);
  while (!o.converged) {
    std::memcpy(o.est, o.cur, sizeof o.est);
    if (P.mode == SICP_MODE_SEMANTIC) o.count++;  // semantic_icp.hpp:47
    SICPCHECK(run_correspondences(h, o.cur, P.knn, true));
    {
      const double t0 = now_ms();
      SolveResult r;
      SICPCHECK(run_solve(h, o.est, o.est, &r));
      h->st.total_lm_iters += r.iterations;
      h->st.final_cost = r.cost;
      h->st.t_solve_ms += now_ms() - t0;
    }
    outer_finish(P, o);
  }
  std::memcpy(out_qt, o.cur, sizeof o.cur);
  SICPCHECK(align_end(h, o, t_begin, outer_iters, stats));
  return SICP_OK;
}

// sicp_set_confusion, uploading on `st` and waiting for it (a stream's slot: on its own stream, not the one it borrows)
int sicp::host::set_confusion(sicp_context* h, int32_t C, const double* cm, hipStream_t st) {
  if (C < 1 || C > 255 || !cm) return SICP_ERR_INVALID_ARGUMENT;
  SICPCHECK(set_device(h));
  h->C = C;
  h->cm.assign(cm, cm + (size_t)C * C);
  {  // FNV-1a of the contents: handles holding the same matrix share the projections of a shared cloud
    unsigned long long id = 1469598103934665603ull ^ (unsigned long long)C;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(h->cm.data());
    for (size_t i = 0; i < sizeof(double) * h->cm.size(); ++i) id = (id ^ b[i]) * 1099511628211ull;
    h->cm_id = id;
  }
  HIPCHECK(h->d_cm.reserve((size_t)C * C));
  HIPCHECK(hipMemcpyAsync(h->d_cm.p, h->cm.data(), sizeof(double) * C * C, hipMemcpyHostToDevice, st));
  HIPCHECK(hipStreamSynchronize(st));
  return SICP_OK;
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

#define SICP_STR2(x) #x
#define SICP_STR(x) SICP_STR2(x)
const char* sicp_version(void) { return "semantic-icp_amd " SICP_STR(SICP_VERSION_MAJOR) "." SICP_STR(SICP_VERSION_MINOR) " (gfx950)"; }

const char* sicp_strerror(int s) {
  switch (s) {
    case SICP_OK: return "ok";
    case SICP_ERR_INVALID_ARGUMENT: return "invalid argument";
    case SICP_ERR_NO_DEVICE: return "no usable HIP device";
    case SICP_ERR_HIP: return "HIP runtime error (see sicp_last_error)";
    case SICP_ERR_NOT_READY: return "clouds / labels / confusion matrix not set for this mode";
    case SICP_ERR_TOO_FEW_POINTS: return "target cloud has fewer points than correspondences requested";
    case SICP_ERR_BAD_LABEL: return "EM label outside 1..C";
    case SICP_ERR_OUT_OF_MEMORY: return "out of memory";
    case SICP_ERR_INTERNAL: return "internal error caught at the ABI boundary (see sicp_last_error)";
    default: return "unknown status";
  }
}

const char* sicp_last_error(sicp_handle h) { return h ? h->last_error.c_str() : ""; }

int sicp_device_count(int* count) {
  return abi_guard([&]() -> int {
    if (!count) return SICP_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return SICP_ERR_NO_DEVICE; }
    *count = n;
    return SICP_OK;
  });
}

int sicp_default_params(int mode, sicp_params* p) {
  return abi_guard([&]() -> int {
    if (!p || mode < SICP_MODE_GICP || mode > SICP_MODE_SEMANTIC) return SICP_ERR_INVALID_ARGUMENT;
    std::memset(p, 0, sizeof *p);
    p->mode = mode;
    p->k_cov = 20;          // em_icp.h:42, gicp.h:34, semantic_point_cloud.h:31
    p->epsilon = 0.001;     // em_icp.h:43
    p->gate_sq = 250.0;     // em_icp.hpp:65, gicp.hpp:70, semantic_icp.hpp:69
    p->min_class_pts = 400; // semantic_icp.hpp:51
    p->max_lm_iterations = 400;         // em_icp.hpp:169
    p->gradient_tolerance = 0.1 * 1e-10; // 0.1 * Sophus::Constants<double>::epsilon(), em_icp.hpp:163
    p->function_tolerance = 0.1 * 1e-10; // em_icp.hpp:164
    p->parameter_tolerance = 1e-8;
    p->initial_radius = 1e4;
    p->max_radius = 1e16;
    p->min_radius = 1e-32;
    p->min_relative_decrease = 1e-3;
    p->min_lm_diagonal = 1e-6;
    p->max_lm_diagonal = 1e32;
    p->max_consecutive_invalid_steps = 5;
    p->jacobi_scaling = 1;
    p->quirk_bool_probability = 1;
    p->quirk_float_products = 1;
    p->nn_method = 1;  // exact box-tree search, packet walk; 2 = per-query walk; 0 = LDS-tiled brute force (same results)
    p->lm_on_device = 1;
    p->lm_batch = 8;   // 16 kernel nodes per graph: longer graphs replay with a ~50 us bubble every 16 nodes
    if (mode == SICP_MODE_EM) {
      p->knn = 4; p->cauchy_a = 3.0; p->use_sqloss = 1;  // em_icp.hpp:60,111,115
      p->outer_tol = 1e-5; p->max_outer = 50;            // em_icp.hpp:180
    } else if (mode == SICP_MODE_GICP) {
      p->knn = 1; p->cauchy_a = 3.0; p->use_sqloss = 1;  // gicp.hpp:69,100,102
      p->outer_tol = 1e-5; p->max_outer = 50;            // gicp.hpp:154
    } else {
      p->knn = 1; p->cauchy_a = 1.5; p->use_sqloss = 0;  // semantic_icp.hpp:68,96
      p->outer_tol = 0.001; p->max_outer = 35;           // semantic_icp.hpp:152
    }
    return SICP_OK;
  });
}

// Handles are recycled like clouds: sicp_destroy parks a handle -- streams, events, pinned mirrors, device buffers, tick
// graphs and all -- in a per-device pool and sicp_create hands it out again, reset to what a new handle is.  The
// reference's drivers construct their registration objects PER PAIR (exec/kitti_eval.cc:176,198, exec/nyu_eval.cc:140,183), and a
// handle made from nothing costs ~4 ms to create, ~5 ms of first-use allocations inside its first align() and ~9 ms to
// destroy (every device buffer given back waits for the device): 49.6 ms per KITTI pair through the class shims against
// ~2 ms of align() (profiles/r06/dropin_calls_before.json).  sicp_release_pool frees the parked handles too.
namespace {
struct HandlePool {
  std::mutex m;
  std::vector<sicp_context*> parked[sicp::host::kPoolDevices];
};
HandlePool& handle_pool() {
  static HandlePool* p = new HandlePool;  // never destroyed: it may outlive the HIP runtime at process exit
  return *p;
}
constexpr size_t kHandlePoolCap = 32;  // per device (a parked handle keeps its buffers: ~12 MB at 100K x 4 slots)

int destroy_for_real(sicp_context* h);
}  // namespace

int sicp_create(int device_id, sicp_handle* out) {
  return abi_guard([&]() -> int {
    if (!out) return SICP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SICP_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= n) return SICP_ERR_INVALID_ARGUMENT;
    {
      HandlePool& pool = handle_pool();
      sicp_context* h = nullptr;
      {
        std::lock_guard<std::mutex> lock(pool.m);
        auto& v = pool.parked[device_id % kPoolDevices];
        for (size_t i = v.size(); i-- > 0;)
          if (v[i]->device == device_id) { h = v[i]; v.erase(v.begin() + (long)i); break; }
      }
      if (h) {
        h->parked = false;
        h->cl[0] = acquire_cloud(device_id);
        h->cl[1] = acquire_cloud(device_id);
        *out = h;
        return SICP_OK;
      }
    }
    sicp_context* h = new (std::nothrow) sicp_context();
    if (!h) return SICP_ERR_OUT_OF_MEMORY;
    h->device = device_id;
    h->cl[0] = acquire_cloud(device_id);
    h->cl[1] = acquire_cloud(device_id);
    bool ok = hipSetDevice(device_id) == hipSuccess && h->own_stream.create() == hipSuccess && h->own_stream2.create() == hipSuccess &&
              h->ev_join.create() == hipSuccess && h->ev0.create(hipEventDefault) == hipSuccess && h->ev1.create(hipEventDefault) == hipSuccess &&
              h->h_out28.resize(28) == hipSuccess && h->h_count.resize(sicp::kLiveCounters) == hipSuccess && h->h_lm.resize(1) == hipSuccess;
    if (!ok) {
      delete h;
      return SICP_ERR_NO_DEVICE;
    }
    h->reset_use();  // (the streams it launches on: its own)
    *out = h;
    return SICP_OK;
  });
}

int sicp_destroy(sicp_handle h) {
  return abi_guard(h, [&]() -> int {
    if (!h) return SICP_OK;
    if (h->parked) return SICP_ERR_INVALID_ARGUMENT;  // destroyed already: the pool's, until sicp_create hands it out again
    // park it: everything it queued has ended, its clouds go back to their pool (or stay with whoever shares them), and
    // what remains is a handle as sicp_create makes them -- with its streams, mirrors, buffers and graphs in place
    bool clean = h->own_stream && h->own_stream2 && hipSetDevice(h->device) == hipSuccess && hipStreamSynchronize(h->own_stream) == hipSuccess &&
                 hipStreamSynchronize(h->own_stream2) == hipSuccess;
    if (clean && h->side_stream) clean = hipStreamSynchronize(h->side_stream) == hipSuccess;
    if (clean && h->feat_stream) clean = hipStreamSynchronize(h->feat_stream) == hipSuccess;
    for (int s2 = 1; clean && s2 < kParts; ++s2)
      if (h->part_stream[s2]) clean = hipStreamSynchronize(h->part_stream[s2]) == hipSuccess;
    if (clean) {
      for (auto& c : h->cl)
        if (c) { settle_cloud(*c); c.reset(); }
      h->reset_use();
      HandlePool& pool = handle_pool();
      std::lock_guard<std::mutex> lock(pool.m);
      auto& v = pool.parked[h->device % kPoolDevices];
      if (v.size() < kHandlePoolCap) { h->parked = true; v.push_back(h); return SICP_OK; }
    }
    return destroy_for_real(h);
  });
}

namespace {
int destroy_for_real(sicp_context* h) {
  {
    (void)hipSetDevice(h->device);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    if (h->own_stream2) (void)hipStreamSynchronize(h->own_stream2);
    for (auto& c : h->cl)
      if (c) settle_cloud(*c);  // before the streams go (see settle_cloud)
    {
      DevArena::FreeScope once(h->device);  // one wait for the device, not one per buffer of the handle
      delete h;  // graphs and pinned mirrors, then events, then streams (engine.hpp: the order of the members)
    }
    return SICP_OK;
  }
}
}  // namespace

int sicp_release_pool(int device_id) {
  return abi_guard([&]() -> int {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return SICP_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= n_dev) return SICP_ERR_INVALID_ARGUMENT;
    CloudPool& pool = cloud_pool();
    std::vector<Cloud*> dead;
    {
      std::lock_guard<std::mutex> lock(pool.m);
      dead.swap(pool.free_list[device_id % kPoolDevices]);
    }
    if (hipSetDevice(device_id) != hipSuccess) return SICP_ERR_NO_DEVICE;
    {  // the parked handles of this device (their buffers are part of what the pool holds)
      std::vector<sicp_context*> idle;
      {
        HandlePool& hp = handle_pool();
        std::lock_guard<std::mutex> lock(hp.m);
        auto& v = hp.parked[device_id % kPoolDevices];
        for (size_t i = v.size(); i-- > 0;)
          if (v[i]->device == device_id) { idle.push_back(v[i]); v.erase(v.begin() + (long)i); }
      }
      for (sicp_context* g : idle) (void)destroy_for_real(g);
    }
    for (Cloud* c : dead) delete c;
    (void)hipDeviceSynchronize();   // nothing may still be running out of a block that goes back to the driver
    dev_arena().release(device_id);  // the slabs no live buffer is carved from
    return SICP_OK;
  });
}

int sicp_set_memory_limit(int device_id, int64_t bytes) {
  return abi_guard([&]() -> int {
    if (device_id < 0 || device_id >= kArenaDevices || bytes < 0) return SICP_ERR_INVALID_ARGUMENT;
    DevArena& A = dev_arena();
    std::lock_guard<std::mutex> lock(A.m);
    A.dev[device_id].limit = (size_t)bytes;
    return SICP_OK;
  });
}

int sicp_memory_reserved(int device_id, int64_t* bytes) {
  return abi_guard([&]() -> int {
    if (device_id < 0 || device_id >= kArenaDevices || !bytes) return SICP_ERR_INVALID_ARGUMENT;
    DevArena& A = dev_arena();
    std::lock_guard<std::mutex> lock(A.m);
    *bytes = (int64_t)A.dev[device_id].reserved;
    return SICP_OK;
  });
}

int sicp_set_params(sicp_handle h, const sicp_params* p) {
  return abi_guard(h, [&]() -> int {
    if (!h || !p) return SICP_ERR_INVALID_ARGUMENT;
    if (p->mode < SICP_MODE_GICP || p->mode > SICP_MODE_SEMANTIC) return SICP_ERR_INVALID_ARGUMENT;
    if (!sicp::nn_k_supported(p->knn)) {
      h->last_error = "sicp_set_params: knn (correspondences per source point) must be 1, 4 or 20";
      return SICP_ERR_INVALID_ARGUMENT;
    }
    if (sicp::nn_list_len(p->k_cov) == 0) {
      h->last_error = "sicp_set_params: k_cov (covariance neighbourhood, the constructors' k) must be in 1..32";
      return SICP_ERR_INVALID_ARGUMENT;
    }
    if (!(p->epsilon > 0) || !(p->cauchy_a > 0) || p->nn_method < 0 || p->nn_method > 2) return SICP_ERR_INVALID_ARGUMENT;
    // The trust-region options reach lm_propose's retry loop inside a kernel (csrc/lm.hpp): a radius that never falls to
    // min_radius (NaN, Inf) under caps near INT_MAX would keep a wave spinning for minutes.  Inside the rule below the
    // loop is bounded without the caps: a finite radius is halved to 0 <= min_radius in at most ~2100 retries.
    if (const char* bad = lm_options_refused(*p)) {
      h->last_error = std::string("sicp_set_params: ") + bad;
      return SICP_ERR_INVALID_ARGUMENT;
    }
    // engine knobs (profiling, batching) do not invalidate the correspondences held on the device
    sicp_params a = h->params, b = *p;
    a.profile = b.profile = 0; a.lm_batch = b.lm_batch = 0; a.lm_on_device = b.lm_on_device = 0;
    if (std::memcmp(&a, &b, sizeof a) != 0) { h->corr_valid = false; h->hint_ok = false; }
    h->params = *p;
    return SICP_OK;
  });
}

int sicp_get_params(sicp_handle h, sicp_params* p) {
  return abi_guard(h, [&]() -> int {
    if (!h || !p) return SICP_ERR_INVALID_ARGUMENT;
    *p = h->params;
    return SICP_OK;
  });
}

int sicp_set_cloud(sicp_handle h, int which, int32_t n, const float* x, const float* y, const float* z,
                   const uint32_t* label) {
  return abi_guard(h, [&]() -> int {
    if (!h || (which != SICP_SOURCE && which != SICP_TARGET) || n < 0) return SICP_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!x || !y || !z)) return SICP_ERR_INVALID_ARGUMENT;
    const StridedCloud in = {(const char*)x, (const char*)y, (const char*)z, (const char*)label, 4, 4};
    return set_cloud_common(h, which, n, in);
  });
}

int sicp_set_cloud_strided(sicp_handle h, int which, int32_t n, const void* xyz, int64_t stride_bytes, const void* label,
                           int64_t label_stride_bytes) {
  return abi_guard(h, [&]() -> int {
    if (!h || (which != SICP_SOURCE && which != SICP_TARGET) || n < 0) return SICP_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!xyz || stride_bytes < 12 || (label && label_stride_bytes < 4))) return SICP_ERR_INVALID_ARGUMENT;
    const char* b = (const char*)xyz;
    const StridedCloud in = {b, b + 4, b + 8, (const char*)label, stride_bytes, label_stride_bytes};
    return set_cloud_common(h, which, n, in);
  });
}

int sicp_set_cloud_device(sicp_handle h, int which, int32_t n, const float* xd, const float* yd, const float* zd,
                          const uint32_t* ld) {
  return abi_guard(h, [&]() -> int {
    if (!h || n < 0 || (n > 0 && (!xd || !yd || !zd))) return SICP_ERR_INVALID_ARGUMENT;
    SICPCHECK(set_device(h));
    // the host keeps a copy of every cloud (regrouping for SICP_MODE_SEMANTIC and the final
    // un-permutation need it), so a device-resident input is mirrored once
    std::vector<float> x(n), y(n), z(n);
    std::vector<uint32_t> l(ld ? n : 0);
    if (n > 0) {
      HIPCHECK(hipMemcpy(x.data(), xd, sizeof(float) * n, hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(y.data(), yd, sizeof(float) * n, hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(z.data(), zd, sizeof(float) * n, hipMemcpyDeviceToHost));
      if (ld) HIPCHECK(hipMemcpy(l.data(), ld, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    }
    return sicp_set_cloud(h, which, n, x.data(), y.data(), z.data(), ld ? l.data() : nullptr);
  });
}

int sicp_share_cloud(sicp_handle h, int which, sicp_handle from, int from_which) {
  return abi_guard(h, [&]() -> int {
    if (!h || !from || (which != SICP_SOURCE && which != SICP_TARGET) || (from_which != SICP_SOURCE && from_which != SICP_TARGET))
      return SICP_ERR_INVALID_ARGUMENT;
    if (h->device != from->device) {
      h->last_error = "sicp_share_cloud: the handles are on different devices";
      return SICP_ERR_INVALID_ARGUMENT;
    }
    if (!from->cloud(from_which).is_set) return SICP_ERR_NOT_READY;
    if (h->cl[which] && h->cl[which] != from->cl[from_which]) settle_cloud(*h->cl[which]);
    h->cl[which] = from->cl[from_which];
    h->corr_valid = false;
    h->hint_ok = false;
    return SICP_OK;
  });
}

int sicp_cloud_size(sicp_handle h, int which, int32_t* n_points, int32_t* n_indexed) {
  return abi_guard(h, [&]() -> int {
    if (!h || (which != SICP_SOURCE && which != SICP_TARGET)) return SICP_ERR_INVALID_ARGUMENT;
    const Cloud& c = h->cloud(which);
    if (!c.is_set) return SICP_ERR_NOT_READY;
    if (n_points) *n_points = c.n_caller;
    if (n_indexed) *n_indexed = c.n;
    return SICP_OK;
  });
}

int sicp_set_confusion(sicp_handle h, int32_t C, const double* cm) {
  return abi_guard(h, [&]() -> int { return h ? set_confusion(h, C, cm, h->stream) : SICP_ERR_INVALID_ARGUMENT; });
}

int sicp_align(sicp_handle h, const double init_qt[7], double out_qt[7], int32_t* outer_iters, sicp_stats* stats) {
  return abi_guard(h, [&]() -> int {
    if (!h || !init_qt || !out_qt) return SICP_ERR_INVALID_ARGUMENT;
    SICPCHECK(set_device(h));
    SICPCHECK(check_ready(h, false));
    const sicp_params& P = h->params;
    // device-resident solve: a lock-step batch of one (the same kernels, hence the same bits, as any batch)
    if (P.lm_on_device && !general_covariances(h)) return sicp_align_batch(&h, 1, init_qt, out_qt, outer_iters, stats);
    return align_host_loop(h, init_qt, out_qt, outer_iters, stats);
  });
}

int sicp_align_batch(sicp_handle* hs, int32_t n, const double* init_qt, double* out_qt, int32_t* outer_iters, sicp_stats* stats) {
  return abi_guard((hs && n > 0) ? hs[0] : nullptr, [&]() -> int {
    return align_batch(hs, n, init_qt, out_qt, outer_iters, stats);
  });
}

int sicp_accumulate_batch(sicp_handle* hs, int32_t n, const double* qt, double* out28, int32_t repeat, double* kernel_ms) {
  return abi_guard((hs && n > 0) ? hs[0] : nullptr, [&]() -> int {
    if (!hs || n < 1 || !qt || !out28) return SICP_ERR_INVALID_ARGUMENT;
    for (int p = 0; p < n; ++p)
      if (hs[p] && general_covariances(hs[p])) {
        hs[p]->last_error = "sicp_accumulate_batch: a handle with caller covariances of general form evaluates one pair at a time (sicp_accumulate)";
        return SICP_ERR_INVALID_ARGUMENT;
      }
    for (int p = 0; p < n; ++p)
      if (!hs[p] || !hs[p]->corr_valid || hs[p]->device != hs[0]->device || hs[p]->corr_K != hs[0]->corr_K) return SICP_ERR_NOT_READY;
    sicp_context* h = hs[0];
    if (n > kMaxActivePairs) return SICP_ERR_INVALID_ARGUMENT;  // one launch holds at most this many pairs
    SICPCHECK(set_device(h));
    SICPCHECK(batch_reserve(h, n));
    h->ts[0].tick_valid = false;
    for (int p = 0; p < n; ++p) {
      sicp_context* g = hs[p];
      const int nb = sicp::accumulate_blocks(g->corr_n * g->corr_K, g->corr_K);
      if (g->partials.reserve((size_t)nb * 28) != hipSuccess) return SICP_ERR_OUT_OF_MEMORY;
      std::memset(&h->ts[0].h_batch[p], 0, sizeof(sicp::BatchArgs));
      fill_acc(g, h->ts[0].h_batch[p].a);
      fill_pose(qt + 7 * p, h->ts[0].h_batch[p].a.pose);
      h->ts[0].h_batch[p].nb = nb;
      HIPCHECK(hipStreamSynchronize(g->stream));  // the pair's correspondences are complete
    }
    *h->ts[0].h_bhdr.p = sicp::BatchHeader{n, 0u, 0u, 0};
    HIPCHECK(hipMemcpyAsync(h->ts[0].d_bhdr.p, h->ts[0].h_bhdr.p, sizeof(sicp::BatchHeader), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->ts[0].d_batch.p, h->ts[0].h_batch.p, sizeof(sicp::BatchArgs) * n, hipMemcpyHostToDevice, h->stream));
    if (repeat < 1) repeat = 1;
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (int r = 0; r < repeat; ++r)
      HIPCHECK(sicp::launch_accumulate_batch(h->corr_K, h->params.use_sqloss, h->ts[0].d_bhdr.p, h->ts[0].d_batch.p, std::min(h->ts[0].cap, kMaxActivePairs),
                                             h->stream));
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    HIPCHECK(sicp::launch_finalize_batch(h->ts[0].d_batch.p, n, h->d_bout28.p, h->stream));
    HIPCHECK(hipMemcpyAsync(h->h_bout28.p, h->d_bout28.p, sizeof(double) * 28 * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    std::memcpy(out28, h->h_bout28.p, sizeof(double) * 28 * n);
    if (kernel_ms) {
      float ms = 0.f;
      HIPCHECK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
      *kernel_ms = (double)ms / repeat;
    }
    return SICP_OK;
  });
}

int sicp_search_batch(sicp_handle* hs, int32_t n, const double* qt, int32_t what, int32_t use_hint, int32_t repeat, double* kernel_ms) {
  return abi_guard((hs && n > 0) ? hs[0] : nullptr, [&]() -> int {
    if (!hs || n < 1 || what < 0 || what > 3 || ((what == 0 || what == 3) && !qt)) return SICP_ERR_INVALID_ARGUMENT;
    sicp_context* h = hs[0];
    SICPCHECK(set_device(h));
    for (int p = 0; p < n; ++p) {
      if (!hs[p] || hs[p]->device != h->device || !same_solver(hs[p]->params, h->params) || hs[p]->params.nn_method != 1) return SICP_ERR_INVALID_ARGUMENT;
      sicp_context* g = hs[p];
      {
        sicp_context* h = g;  // (HIPCHECK / SICPCHECK report into the handle they run on)
        SICPCHECK(check_ready(h, false));
        SICPCHECK(prepare_cloud(h, h->cloud(0)));
        SICPCHECK(prepare_cloud(h, h->cloud(1)));
        if (what == 3) {  // the search as an align() launches it, EM weights included: the features it reads must be there
          if (h->params.mode != SICP_MODE_EM) return SICP_ERR_INVALID_ARGUMENT;
          SICPCHECK(check_ready(h, true));
          for (int c = 0; c < 2; ++c)
            if (!features_current(h, h->cloud(c), true)) { h->epoch = next_epoch(); SICPCHECK(compute_features(h, h->cloud(c), true)); }
          if (!weights_from_histograms(h->params, h->params.knn)) { SICPCHECK(ensure_proj(h, h->cloud(0))); SICPCHECK(ensure_proj(h, h->cloud(1))); }
        }
        HIPCHECK(hipStreamSynchronize(h->stream));
      }
    }
    // the handles' own stage drivers collect the jobs exactly as sicp_align_batch makes them
    JobCollector jc;
    jc.fold_weights = what == 3;
    {
      BatchGuard guard(hs, n, &jc, h->stream);
      for (int p = 0; p < n; ++p) {
        sicp_context* g = hs[p];
        jc.slice = 0;
        if (what == 0 || what == 3) {
          if (!use_hint) g->hint_ok = false;
          const int rc = run_correspondences(g, qt + 7 * p, g->params.knn, what == 3);
          if (rc != SICP_OK) return rc;
        } else {
          g->epoch = next_epoch();
          const int rc = compute_features(g, g->cloud(what == 1 ? SICP_SOURCE : SICP_TARGET), g->params.mode == SICP_MODE_EM);
          if (rc != SICP_OK) return rc;
        }
      }
    }
    if (repeat < 1) repeat = 1;
    const int L = jc.part[0].knn_K;
    HIPCHECK(hipEventRecord(h->ev0, h->stream));
    for (int r = 0; r < repeat; ++r)
      if (!jc.part[0].knn.empty()) HIPCHECK(sicp::launch_bvh_knn_packet_jobs(L, jc.part[0].knn.data(), (int)jc.part[0].knn.size(), h->stream));
    HIPCHECK(hipEventRecord(h->ev1, h->stream));
    // whatever consumes the searches (covariances, histograms, projections) runs once, so the handles stay consistent
    jc.part[0].knn.clear();
    SICPCHECK(flush_jobs(h, jc, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (kernel_ms) {
      float ms = 0.f;
      HIPCHECK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
      *kernel_ms = (double)ms / repeat;
    }
    return SICP_OK;
  });
}

int sicp_transform_source(sicp_handle h, const double qt[7], float* ox, float* oy, float* oz) {
  return abi_guard(h, [&]() -> int {
    if (!h || !qt || !ox || !oy || !oz) return SICP_ERR_INVALID_ARGUMENT;
    SICPCHECK(set_device(h));
    Cloud& S = h->cloud(0);
    SICPCHECK(prepare_cloud(h, S));
    const int n = S.n;
    const size_t m = (size_t)(n > 0 ? n : 1);
    HIPCHECK(h->tmpx.reserve(m)); HIPCHECK(h->tmpy.reserve(m)); HIPCHECK(h->tmpz.reserve(m));
    double M[12];
    matrix34(qt, M);
    sicp::Mat4f Mf;
    for (int i = 0; i < 12; ++i) Mf.m[i] = (float)M[i];  // (trans.matrix()).cast<float>(), em_icp.hpp:193
    Mf.m[12] = Mf.m[13] = Mf.m[14] = 0.f; Mf.m[15] = 1.f;
    HIPCHECK(sicp::launch_transform_float(n, S.x.p, S.y.p, S.z.p, Mf, h->tmpx.p, h->tmpy.p, h->tmpz.p, h->stream));
    std::vector<float> bx(n), by(n), bz(n);
    if (n > 0) {
      HIPCHECK(hipMemcpyAsync(bx.data(), h->tmpx.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
      HIPCHECK(hipMemcpyAsync(by.data(), h->tmpy.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
      HIPCHECK(hipMemcpyAsync(bz.data(), h->tmpz.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    for (int d = 0; d < n; ++d) {
      const int i = S.caller_index(d);
      ox[i] = bx[d]; oy[i] = by[d]; oz[i] = bz[d];
    }
    // the non-finite points that never went to the device: the same float arithmetic, here
    for (size_t k = 0; k < S.drop_i.size(); ++k) {
      const int i = S.drop_i[k];
      const float px = S.drop_xyz[3 * k], py = S.drop_xyz[3 * k + 1], pz = S.drop_xyz[3 * k + 2];
      const float* m = Mf.m;
      // (this file is compiled with -ffp-contract=off: separately rounded products and sums, like transform_float_kernel)
      auto row = [&](int r) { return ((m[4 * r] * px + m[4 * r + 1] * py) + m[4 * r + 2] * pz) + m[4 * r + 3]; };
      ox[i] = row(0); oy[i] = row(1); oz[i] = row(2);
    }
    return SICP_OK;
  });
}

int sicp_set_covariances(sicp_handle h, int which, const double* cov9) {
  return abi_guard(h, [&]() -> int {
    if (!h || !cov9 || (which != SICP_SOURCE && which != SICP_TARGET)) return SICP_ERR_INVALID_ARGUMENT;
    SICPCHECK(set_device(h));
    const sicp_params& P = h->params;
    Cloud& c = h->cloud(which);
    if (!c.is_set) return SICP_ERR_NOT_READY;
    SICPCHECK(prepare_cloud(h, c));
    SICPCHECK(cloud_wait(h, c));  // (perm is read below)
    const double kappa = 1.0 - P.epsilon;
    if (!(kappa > 0.0)) { h->last_error = "sicp_set_covariances: params.epsilon must be below 1"; return SICP_ERR_INVALID_ARGUMENT; }
    const int n = c.n;
    const size_t m = (size_t)(n > 0 ? n : 1);
    std::vector<double> nrm(m * 3, 0.0), c6;
    // The engine's own form, C = I - kappa n n^T  <=>  (I - C) / kappa = n n^T: symmetric, rank one, trace one.  The normal is
    // the column with the largest diagonal entry, scaled; what is left after taking n n^T away is the distance from the form.
    // A cloud whose matrices ALL have it keeps its normals and runs the product kernels.  Otherwise the matrices are kept as
    // they are (symmetric and finite is all the closed-form Jacobian of SURVEY 8a / a7 needs) and the cloud's registrations
    // run through the full-matrix evaluation, one pair at a time (solve_kernels.hip: accumulate_general_kernel).
    constexpr double tol = 1e-8;
    bool normal_form = true;
    int first_general = -1;
    for (int d = 0; d < n; ++d) {
      const int ci = c.caller_index(d);
      const double* C9 = cov9 + (size_t)ci * 9;
      bool finite = true, symmetric = true;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          finite = finite && std::isfinite(C9[3 * a + b]);
          symmetric = symmetric && std::fabs(C9[3 * a + b] - C9[3 * b + a]) <= tol * (1.0 + std::fabs(C9[3 * a + b]));
        }
      if (!finite || !symmetric) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "sicp_set_covariances: the covariance of point %d is not a finite symmetric 3x3 matrix; nothing was changed", ci);
        h->last_error = msg;
        return SICP_ERR_INVALID_ARGUMENT;
      }
      if (!normal_form) continue;
      double M[3][3];
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) M[a][b] = ((a == b ? 1.0 : 0.0) - C9[3 * a + b]) / kappa;
      int col = 0;
      if (M[1][1] > M[col][col]) col = 1;
      if (M[2][2] > M[col][col]) col = 2;
      bool ok = M[col][col] > 0.0;
      double nv[3] = {0, 0, 0};
      if (ok) {
        const double sc = 1.0 / std::sqrt(M[col][col]);
        for (int a = 0; a < 3; ++a) nv[a] = M[a][col] * sc;
        const double len = std::sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
        ok = std::fabs(len - 1.0) <= tol;
        for (int a = 0; a < 3 && ok; ++a)
          for (int b = 0; b < 3; ++b) ok = ok && std::fabs(M[a][b] - nv[a] * nv[b]) <= tol;
        if (ok) for (int a = 0; a < 3; ++a) nv[a] /= len;
      }
      if (!ok) { normal_form = false; first_general = ci; continue; }
      nrm[3 * (size_t)d] = nv[0]; nrm[3 * (size_t)d + 1] = nv[1]; nrm[3 * (size_t)d + 2] = nv[2];
    }
    if (!normal_form) {
      if (P.mode == SICP_MODE_EM) {  // (its align() recomputes covariances and label histograms together: impl/em_icp.hpp:28-29)
        char msg[256];
        std::snprintf(msg, sizeof msg, "sicp_set_covariances: the covariance of point %d is not I - (1 - epsilon) n n^T (epsilon = %g); general matrices are taken "
                                       "in SICP_MODE_GICP / SICP_MODE_SEMANTIC only; nothing was changed", first_general, P.epsilon);
        h->last_error = msg;
        return SICP_ERR_INVALID_ARGUMENT;
      }
      std::fill(nrm.begin(), nrm.end(), 0.0);  // (the records of such a cloud carry positions only)
      c6.assign(m * 6, 0.0);
      for (int d = 0; d < n; ++d) {
        const double* C9 = cov9 + (size_t)c.caller_index(d) * 9;
        double* o = &c6[6 * (size_t)d];
        o[0] = C9[0]; o[1] = 0.5 * (C9[1] + C9[3]); o[2] = 0.5 * (C9[2] + C9[6]); o[3] = C9[4]; o[4] = 0.5 * (C9[5] + C9[7]); o[5] = C9[8];
      }
    }
    HIPCHECK(c.rec.reserve(m));
    HIPCHECK(c.rec_dense.reserve(sicp::dense_rec_bytes(n)));
    if (!normal_form) HIPCHECK(c.cov6.reserve(m * 6));
    DevBuf<double> d_nrm;
    HIPCHECK(d_nrm.reserve(m * 3));
    if (n == 0) HIPCHECK(hipMemsetAsync(c.rec.p, 0, sizeof(sicp::PointRec), h->stream));  // (compute_features: the record dead slots are evaluated on)
    if (n > 0) HIPCHECK(hipMemcpyAsync(d_nrm.p, nrm.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, h->stream));
    if (n > 0 && !normal_form) HIPCHECK(hipMemcpyAsync(c.cov6.p, c6.data(), sizeof(double) * 6 * n, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(sicp::launch_set_normals(n, c.x.p, c.y.p, c.z.p, d_nrm.p, c.rec.p, c.rec_dense.p, n, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));  // (nrm / c6 / d_nrm go out of scope)
    c.rec_dense_n = n;
    c.feat_valid = true;
    c.cov_general = !normal_form;
    c.proj_valid = false;
    c.feat_k = P.k_cov; c.feat_C = 0;
    c.feat_float_products = P.quirk_float_products;
    c.feat_hist = false;
    c.feat_epoch = h->epoch;
    h->corr_valid = false;
    return SICP_OK;
  });
}

int sicp_covariances(sicp_handle h, int which, double* cov9, double* normal3, uint8_t* hist, int32_t* nn_idx) {
  return abi_guard(h, [&]() -> int {
    if (!h || (which != SICP_SOURCE && which != SICP_TARGET)) return SICP_ERR_INVALID_ARGUMENT;
    SICPCHECK(set_device(h));
    const sicp_params& P = h->params;
    if (sicp::nn_list_len(P.k_cov) == 0) return SICP_ERR_INVALID_ARGUMENT;
    Cloud& c = h->cloud(which);
    SICPCHECK(prepare_cloud(h, c));
    const bool with_hist = P.mode == SICP_MODE_EM && c.has_label && P.num_classes >= 1;
    if (hist && !with_hist) return SICP_ERR_NOT_READY;
    if (with_hist && c.n > 0 && (c.label_min < 1 || c.label_max > (uint32_t)P.num_classes)) return SICP_ERR_BAD_LABEL;
    // what align() left behind is returned as it is (getSourceCovariances(), gicp.h:72-90)
    if (!features_current(h, c, with_hist) || (nn_idx && !c.nn.p)) SICPCHECK(compute_features(h, c, with_hist));
    const int n = c.n, k = P.k_cov;
    if (cov9 && !normal3 && !hist && !nn_idx && c.keep.empty() && n > 0) {
      // the covariances alone of a cloud without dropped points (getSourceCovariances() / getTargetCovariances(), gicp.h:72-90,
      // called once per pair by exec/kitti_eval.cc:225-226): formed in the caller's order on the device and copied straight
      // into the caller's array -- one pass instead of a record read-back, a scatter on the host and the caller's own copy
      HIPCHECK(h->tmp9.reserve((size_t)n * 9));
      HIPCHECK(sicp::launch_cov9_caller_order(n, c.rec.p, c.cov_general ? c.cov6.p : nullptr, c.d_perm.p, 1.0 - P.epsilon, h->tmp9.p, h->stream));
      HIPCHECK(hipMemcpyAsync(cov9, h->tmp9.p, sizeof(double) * 9 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
      HIPCHECK(hipStreamSynchronize(h->stream));
      return SICP_OK;
    }
    std::vector<sicp::PointRec> rec(n);
    if (n > 0) HIPCHECK(hipMemcpyAsync(rec.data(), c.rec.p, sizeof(sicp::PointRec) * n, hipMemcpyDeviceToHost, h->stream));
    std::vector<double> g6;  // caller covariances of general form: what is there is what comes back
    if (c.cov_general && n > 0) {
      g6.resize((size_t)n * 6);
      HIPCHECK(hipMemcpyAsync(g6.data(), c.cov6.p, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, h->stream));
    }
    std::vector<uint8_t> hh;
    std::vector<int> nn;
    const size_t HS = (size_t)sicp::hist_stride(P.num_classes);  // rows are padded to 16 bytes on the device
    if (hist && n > 0) {
      hh.resize((size_t)n * HS);
      HIPCHECK(hipMemcpyAsync(hh.data(), c.hist.p, hh.size(), hipMemcpyDeviceToHost, h->stream));
    }
    if (nn_idx && n > 0) {
      nn.resize((size_t)n * k);
      HIPCHECK(hipMemcpyAsync(nn.data(), c.nn.p, sizeof(int) * nn.size(), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    const double ome = 1.0 - P.epsilon;
    for (int i : c.drop_i) {  // points outside the index have no neighbourhood (the reference's values for them are undefined)
      const double nan = std::numeric_limits<double>::quiet_NaN();
      if (normal3) for (int a = 0; a < 3; ++a) normal3[3 * (size_t)i + a] = nan;
      if (cov9) for (int a = 0; a < 9; ++a) cov9[9 * (size_t)i + a] = nan;
      if (hist) std::memset(hist + (size_t)i * P.num_classes, 0, P.num_classes);
      if (nn_idx) for (int j = 0; j < k; ++j) nn_idx[(size_t)i * k + j] = -1;
    }
    for (int d = 0; d < n; ++d) {
      const int i = c.caller_index(d);
      const double v[3] = {rec[d].nx, rec[d].ny, rec[d].nz};
      if (!g6.empty()) {  // (no normal belongs to a general matrix)
        const double* q = &g6[6 * (size_t)d];
        const double full[9] = {q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]};
        if (cov9) std::memcpy(cov9 + 9 * (size_t)i, full, sizeof full);
        if (normal3) for (int a = 0; a < 3; ++a) normal3[3 * (size_t)i + a] = std::numeric_limits<double>::quiet_NaN();
      } else {
      if (normal3) { normal3[3 * (size_t)i] = v[0]; normal3[3 * (size_t)i + 1] = v[1]; normal3[3 * (size_t)i + 2] = v[2]; }
      if (cov9)  // the covariance the kernels use: C = I - (1-eps) n n^T  (== em_icp.hpp:331-338); the upper triangle, mirrored:
        for (int a = 0; a < 3; ++a)  // bit-symmetric, so the rows a caller reads are also the columns Eigen stores
          for (int b = a; b < 3; ++b) {
            const double e = (a == b ? 1.0 : 0.0) - ome * v[a] * v[b];
            cov9[9 * (size_t)i + 3 * a + b] = e;
            cov9[9 * (size_t)i + 3 * b + a] = e;
          }
      }
      if (hist) std::memcpy(hist + (size_t)i * P.num_classes, hh.data() + (size_t)d * HS, P.num_classes);
      if (nn_idx)
        for (int j = 0; j < k; ++j) {
          const int g = c.nn_stride > 0 ? nn[(size_t)j * c.nn_stride + d] : nn[(size_t)d * k + j];
          nn_idx[(size_t)i * k + j] = g < 0 ? -1 : c.caller_index(g);
        }
    }
    return SICP_OK;
  });
}

int sicp_correspondences(sicp_handle h, const double qt[7], int32_t* idx, float* d2, double* w) {
  return abi_guard(h, [&]() -> int {
    if (!h || !qt) return SICP_ERR_INVALID_ARGUMENT;
    SICPCHECK(set_device(h));
    SICPCHECK(check_ready(h, false));
    SICPCHECK(search_at(h, qt));
    const sicp_params& P = h->params;
    Cloud &S = h->cloud(0), &T = h->cloud(1);
    const int n = S.n, K = P.knn;
    const size_t slots = (size_t)n * K;
    std::vector<int> hi(slots);
    std::vector<float> hd(slots);
    std::vector<double> hw(slots);
    if (slots) {
      HIPCHECK(hipMemcpyAsync(hi.data(), h->idx.p, sizeof(int) * slots, hipMemcpyDeviceToHost, h->stream));
      HIPCHECK(hipMemcpyAsync(hd.data(), h->d2.p, sizeof(float) * slots, hipMemcpyDeviceToHost, h->stream));
      if (h->corr_weighted) HIPCHECK(hipMemcpyAsync(hw.data(), h->w.p, sizeof(double) * slots, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    for (int i : S.drop_i)  // a non-finite source point has no correspondences
      for (int c = 0; c < K; ++c) {
        const size_t o = (size_t)i * K + c;
        if (idx) idx[o] = -1;
        if (d2) d2[o] = std::numeric_limits<float>::quiet_NaN();
        if (w) w[o] = 0.0;
      }
    for (int d = 0; d < n; ++d) {
      const int i = S.caller_index(d);
      for (int c = 0; c < K; ++c) {
        const size_t e = (size_t)d * K + c, o = (size_t)i * K + c;
        const int j = hi[e];
        if (idx) idx[o] = j < 0 ? -1 : T.caller_index(j);
        if (d2) d2[o] = hd[e];
        if (w) w[o] = j < 0 ? 0.0 : (h->corr_weighted ? hw[e] : 1.0);
      }
    }
    return SICP_OK;
  });
}

int sicp_accumulate(sicp_handle h, const double qt[7], double out28[28]) {
  return abi_guard(h, [&]() -> int {
    if (!h || !qt || !out28) return SICP_ERR_INVALID_ARGUMENT;
    if (!h->corr_valid) return SICP_ERR_NOT_READY;
    SICPCHECK(set_device(h));
    return eval28(h, qt, out28);
  });
}

int sicp_pose_covariance(sicp_handle h, const double qt[7], double sigma_source, double sigma_target,
                         sicp_pose_covariance_result* out) {
  return abi_guard(h, [&]() -> int {
    return pose_covariance(h, qt, sigma_source, sigma_target, out);
  });
}

int sicp_pose_covariance_batch(sicp_handle* hs, int32_t n, const double* qt, double sigma_source, double sigma_target,
                               sicp_pose_covariance_result* out, int32_t* status) {
  return abi_guard((hs && n > 0) ? hs[0] : nullptr, [&]() -> int {
    return pose_covariance_batch(hs, n, qt, sigma_source, sigma_target, out, status);
  });
}

int sicp_evaluate(sicp_handle h, const double qt[7], double max_dist_sq, int32_t num_classes, int64_t* confusion, int32_t* nn_idx,
                  float* nn_d2, sicp_evaluate_result* out) {
  return abi_guard(h, [&]() -> int {
    return evaluate(h, qt, max_dist_sq, num_classes, confusion, nn_idx, nn_d2, out);
  });
}

int sicp_evaluate_batch(sicp_handle* hs, int32_t n, const double* qt, double max_dist_sq, int32_t num_classes, int64_t* confusion,
                        sicp_evaluate_result* out, int32_t* status) {
  return abi_guard((hs && n > 0) ? hs[0] : nullptr, [&]() -> int {
    return evaluate_batch(hs, n, qt, max_dist_sq, num_classes, confusion, out, status);
  });
}

int sicp_default_merge_params(sicp_merge_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    merge_default_params(p);
    return SICP_OK;
  });
}

int sicp_merge_clouds(sicp_handle* parts, const int32_t* part_which, int32_t n_parts, const double* qt, const sicp_merge_params* p,
                      sicp_handle dst, int dst_which, int32_t capacity, float* x, float* y, float* z, uint32_t* label,
                      uint32_t* count, sicp_merge_info* info) {
  return abi_guard((parts && n_parts > 0) ? parts[0] : nullptr, [&]() -> int {
    return merge_clouds(parts, part_which, n_parts, qt, p, dst, dst_which, capacity, x, y, z, label, count, info);
  });
}

int sicp_default_cluster_params(sicp_cluster_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    cluster_default_params(p);
    return SICP_OK;
  });
}

int sicp_cluster(sicp_handle h, int which, const sicp_cluster_params* p, int32_t* cluster_id, int32_t capacity, uint32_t* label,
                 int32_t* count, int32_t* first_index, double* centroid, float* bbox_min, float* bbox_max, sicp_cluster_info* info) {
  return abi_guard(h, [&]() -> int {
    return cluster(h, which, p, cluster_id, capacity, label, count, first_index, centroid, bbox_min, bbox_max, info);
  });
}

int sicp_default_filter_params(sicp_filter_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    filter_default_params(p);
    return SICP_OK;
  });
}

int sicp_filter(sicp_handle h, int which, const sicp_filter_params* p, const uint8_t* mask, sicp_handle dst, int dst_which, uint8_t* keep,
                double* mean_dist, int32_t* neighbors, sicp_filter_info* info) {
  return abi_guard(h, [&]() -> int {
    return filter(h, which, p, mask, dst, dst_which, keep, mean_dist, neighbors, info);
  });
}

int sicp_deskew(sicp_handle h, int which, const double* times, int32_t n_knots, const double* knot_time, const double* knot_qt,
                const double ref_qt[7], sicp_handle dst, int dst_which, float* ox, float* oy, float* oz, double* knots_out,
                sicp_deskew_info* info) {
  return abi_guard(h, [&]() -> int {
    return deskew(h, which, times, n_knots, knot_time, knot_qt, ref_qt, dst, dst_which, ox, oy, oz, knots_out, info);
  });
}

int sicp_deskew_twist_knots(const double delta_qt[7], double t0, double t1, int32_t n_knots, double* knot_time, double* knot_qt) {
  return abi_guard([&]() -> int { return deskew_twist_knots(delta_qt, t0, t1, n_knots, knot_time, knot_qt); });
}

int sicp_default_range_params(sicp_range_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    range_default_params(p);
    return SICP_OK;
  });
}

int sicp_range_tables(const sicp_range_params* p, const double* beam_elevation, double* cos_half, double* sin_half, double* row_edge) {
  return abi_guard([&]() -> int { return range_tables(p, beam_elevation, cos_half, sin_half, row_edge); });
}

int sicp_range_image(sicp_handle h, int which, const sicp_range_params* p, const double* beam_elevation, const float sensor_origin[3],
                     int32_t* index, float* range_sq, float* x, float* y, float* z, uint32_t* label, uint32_t* count, int32_t* pixel,
                     uint8_t* visible, sicp_range_info* info) {
  return abi_guard(h, [&]() -> int {
    return range_image(h, which, p, beam_elevation, sensor_origin, index, range_sq, x, y, z, label, count, pixel, visible, info);
  });
}

int sicp_range_labels(sicp_handle h, int which, const sicp_range_params* p, const double* beam_elevation, const float sensor_origin[3],
                      const uint32_t* pixel_label, sicp_handle dst, int dst_which, uint32_t* out_label, uint8_t* votes,
                      sicp_range_info* info) {
  return abi_guard(h, [&]() -> int {
    return range_labels(h, which, p, beam_elevation, sensor_origin, pixel_label, dst, dst_which, out_label, votes, info);
  });
}

int sicp_default_camera_params(sicp_camera_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    camera_default_params(p);
    return SICP_OK;
  });
}

int sicp_camera_matrices(const double camera_qt[7], double cam_to_cloud[12], double cloud_to_cam[12]) {
  return abi_guard([&]() -> int { return camera_matrices(camera_qt, cam_to_cloud, cloud_to_cam); });
}

int sicp_camera_image(sicp_handle h, int which, const sicp_camera_params* p, const double camera_qt[7], int32_t* index, float* depth,
                      float* x, float* y, float* z, uint32_t* label, uint32_t* count, int32_t* pixel, float* u, float* v,
                      uint8_t* visible, sicp_camera_info* info) {
  return abi_guard(h, [&]() -> int {
    return camera_image(h, which, p, camera_qt, index, depth, x, y, z, label, count, pixel, u, v, visible, info);
  });
}

int sicp_camera_labels(sicp_handle h, int which, const sicp_camera_params* p, const double camera_qt[7], const uint32_t* pixel_label,
                       sicp_handle dst, int dst_which, uint32_t* out_label, uint8_t* state, sicp_camera_info* info) {
  return abi_guard(h, [&]() -> int {
    return camera_labels(h, which, p, camera_qt, pixel_label, dst, dst_which, out_label, state, info);
  });
}

int sicp_camera_unproject(sicp_handle h, const sicp_camera_params* p, const double camera_qt[7], const uint16_t* depth_u16,
                          const float* depth_f32, const uint32_t* label, sicp_handle dst, int dst_which, float* x, float* y, float* z,
                          uint8_t* valid, sicp_camera_info* info) {
  return abi_guard(h, [&]() -> int {
    return camera_unproject(h, p, camera_qt, depth_u16, depth_f32, label, dst, dst_which, x, y, z, valid, info);
  });
}

int sicp_default_plane_params(sicp_plane_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    plane_default_params(p);
    return SICP_OK;
  });
}

int sicp_segment_planes(sicp_handle h, int which, const sicp_plane_params* p, const uint8_t* mask, int32_t* plane_id, int32_t capacity,
                        double* coeff, int32_t* count, int32_t* hyp_index, int32_t* hyp_count, double* centroid, double* rms,
                        sicp_plane_info* info) {
  return abi_guard(h, [&]() -> int {
    return segment_planes(h, which, p, mask, plane_id, capacity, coeff, count, hyp_index, hyp_count, centroid, rms, info);
  });
}

int sicp_default_ground_params(sicp_ground_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    ground_default_params(p);
    return SICP_OK;
  });
}

int sicp_ground_tables(const sicp_ground_params* p, const double* ring_edge, double* cos_half, double* sin_half, double* edge2) {
  return abi_guard([&]() -> int { return ground_tables(p, ring_edge, cos_half, sin_half, edge2); });
}

int sicp_segment_ground(sicp_handle h, int which, const sicp_ground_params* p, const uint8_t* mask, const double sensor_origin[3],
                        const double* ring_edge, sicp_handle dst, int dst_which, const sicp_ground_out* out, sicp_ground_info* info) {
  return abi_guard(h, [&]() -> int {
    return segment_ground(h, which, p, mask, sensor_origin, ring_edge, dst, dst_which, out, info);
  });
}

int sicp_default_map_params(sicp_map_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    map_default_params(p);
    return SICP_OK;
  });
}

int sicp_default_map_extract_params(sicp_map_extract_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    map_default_extract_params(p);
    return SICP_OK;
  });
}

int sicp_map_create(int device_id, const sicp_map_params* p, sicp_map* out) {
  return abi_guard([&]() -> int { return map_create(device_id, p, out); });
}

int sicp_map_destroy(sicp_map m) {
  return abi_guard([&]() -> int { return map_destroy(m); });
}

int sicp_map_clear(sicp_map m) {
  return abi_guard(m, [&]() -> int {
    if (!m) return SICP_ERR_INVALID_ARGUMENT;
    m->n_voxels = 0;
    m->n_points = 0;
    return SICP_OK;
  });
}

int sicp_map_size(sicp_map m, int64_t* n_voxels, int64_t* n_points) {
  return abi_guard(m, [&]() -> int {
    if (!m) return SICP_ERR_INVALID_ARGUMENT;
    if (n_voxels) *n_voxels = m->n_voxels;
    if (n_points) *n_points = (int64_t)m->n_points;
    return SICP_OK;
  });
}

const char* sicp_map_last_error(sicp_map m) { return m ? m->last_error.c_str() : ""; }

int sicp_map_integrate(sicp_map m, sicp_handle h, int which, const double qt[7], const double crop_center[3], double crop_range,
                       sicp_map_integrate_info* info) {
  return abi_guard(m, [&]() -> int { return map_integrate(m, h, which, qt, crop_center, crop_range, info); });
}

int sicp_map_prune(sicp_map m, const double center[3], double range, int64_t* n_removed) {
  return abi_guard(m, [&]() -> int { return map_prune(m, center, range, n_removed); });
}

int sicp_default_map_carve_params(sicp_map_carve_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    map_default_carve_params(p);
    return SICP_OK;
  });
}

int sicp_map_carve(sicp_map m, sicp_handle h, int which, const double qt[7], const double sensor_origin[3],
                   const sicp_map_carve_params* p, int32_t capacity, uint32_t* miss, sicp_map_carve_info* info) {
  return abi_guard(m, [&]() -> int { return map_carve(m, h, which, qt, sensor_origin, p, capacity, miss, info); });
}

int sicp_default_map_raycast_params(sicp_map_raycast_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    map_default_raycast_params(p);
    return SICP_OK;
  });
}

int sicp_map_raycast(sicp_map m, const double qt[7], const double sensor_origin[3], int32_t n, const float* ex, const float* ey,
                     const float* ez, const sicp_map_raycast_params* p, sicp_handle dst, int dst_which, int32_t* row, int32_t* step,
                     int32_t* length, float* x, float* y, float* z, uint32_t* label, uint32_t* count, double* range_sq,
                     sicp_map_raycast_info* info) {
  return abi_guard(m, [&]() -> int {
    return map_raycast(m, qt, sensor_origin, n, ex, ey, ez, p, dst, dst_which, row, step, length, x, y, z, label, count, range_sq, info);
  });
}

int sicp_default_map_elevation_params(sicp_map_elevation_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    map_default_elevation_params(p);
    return SICP_OK;
  });
}

int sicp_map_elevation(sicp_map m, const double center[2], const sicp_map_elevation_params* p, const sicp_map_elevation_out* out,
                       sicp_handle h, int which, const double qt[7], sicp_map_elevation_info* info) {
  return abi_guard(m, [&]() -> int { return map_elevation(m, center, p, out, h, which, qt, info); });
}

int sicp_default_map_distance_params(sicp_map_distance_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    map_default_distance_params(p);
    return SICP_OK;
  });
}

int sicp_map_distance(sicp_map m, const double center[3], const sicp_map_distance_params* p, const sicp_map_distance_out* out,
                      sicp_handle h, int which, const double qt[7], sicp_map_distance_info* info) {
  return abi_guard(m, [&]() -> int { return map_distance(m, center, p, out, h, which, qt, info); });
}

int sicp_map_extract(sicp_map m, const sicp_map_extract_params* p, sicp_handle dst, int dst_which, int32_t capacity, float* x,
                     float* y, float* z, uint32_t* label, uint32_t* count, uint32_t* hist, sicp_map_extract_info* info) {
  return abi_guard(m, [&]() -> int {
    return map_extract(m, p, dst, dst_which, capacity, x, y, z, label, count, hist, info);
  });
}

int sicp_map_set_confusion(sicp_map m, int32_t C, const double* cm_rowmajor) {
  return abi_guard(m, [&]() -> int { return map_set_confusion(m, C, cm_rowmajor); });
}

int sicp_map_extract_fused(sicp_map m, const sicp_map_extract_params* p, sicp_handle dst, int dst_which, int32_t capacity, float* x,
                           float* y, float* z, uint32_t* label, uint32_t* count, double* confidence, sicp_map_extract_info* info) {
  return abi_guard(m, [&]() -> int {
    return map_extract_fused(m, p, dst, dst_which, capacity, x, y, z, label, count, confidence, info);
  });
}

int sicp_map_fused_labels(sicp_map m, sicp_handle h, int which, const double qt[7], int32_t include_own_label, int32_t min_count,
                          uint32_t* out_labels, double* out_confidence) {
  return abi_guard(m, [&]() -> int {
    return map_fused_labels(m, h, which, qt, include_own_label, min_count, out_labels, out_confidence);
  });
}

int sicp_default_map_merge_params(sicp_map_merge_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    map_default_merge_params(p);
    return SICP_OK;
  });
}

int sicp_map_merge(sicp_map dst, sicp_map src, const double qt[7], const sicp_map_merge_params* p, sicp_map_merge_info* info) {
  return abi_guard(dst, [&]() -> int { return map_merge(dst, src, qt, p, info); });
}

int sicp_map_get_state(sicp_map m, int64_t capacity, uint64_t* key, double* sums, uint32_t* count, uint32_t* hist, int64_t* n_rows) {
  return abi_guard(m, [&]() -> int { return map_get_state(m, capacity, key, sums, count, hist, n_rows); });
}

int sicp_map_set_state(sicp_map m, int64_t n, const uint64_t* key, const double* sums, const uint32_t* count, const uint32_t* hist) {
  return abi_guard(m, [&]() -> int { return map_set_state(m, n, key, sums, count, hist); });
}

int sicp_default_place_params(sicp_place_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    place_default_params(p);
    return SICP_OK;
  });
}

int sicp_place_create(int device_id, const sicp_place_params* p, sicp_place* out) {
  return abi_guard([&]() -> int { return place_create(device_id, p, out); });
}

int sicp_place_destroy(sicp_place db) {
  return abi_guard([&]() -> int { return place_destroy(db); });
}

int sicp_place_clear(sicp_place db) {
  return abi_guard(db, [&]() -> int {
    if (!db) return SICP_ERR_INVALID_ARGUMENT;
    db->n_entries = 0;
    return SICP_OK;
  });
}

int sicp_place_size(sicp_place db, int64_t* n_entries) {
  return abi_guard(db, [&]() -> int {
    if (!db) return SICP_ERR_INVALID_ARGUMENT;
    if (!n_entries) {
      db->last_error = "sicp_place_size: n_entries is NULL";
      return SICP_ERR_INVALID_ARGUMENT;
    }
    *n_entries = db->n_entries;
    return SICP_OK;
  });
}

const char* sicp_place_last_error(sicp_place db) { return db ? db->last_error.c_str() : ""; }

int sicp_place_describe(sicp_place db, sicp_handle h, int which, const double sensor_origin[3], uint8_t* desc,
                        sicp_place_describe_info* info) {
  return abi_guard(db, [&]() -> int { return place_describe(db, h, which, sensor_origin, desc, info); });
}

int sicp_place_add(sicp_place db, sicp_handle h, int which, const double sensor_origin[3], int32_t* id, uint8_t* desc,
                   sicp_place_describe_info* info) {
  return abi_guard(db, [&]() -> int { return place_add(db, h, which, sensor_origin, id, desc, info); });
}

int sicp_place_add_descriptors(sicp_place db, int32_t n, const uint8_t* desc, int32_t* first_id) {
  return abi_guard(db, [&]() -> int { return place_add_descriptors(db, n, desc, first_id); });
}

int sicp_place_get(sicp_place db, int32_t first, int32_t count, uint8_t* desc) {
  return abi_guard(db, [&]() -> int { return place_get(db, first, count, desc); });
}

int sicp_place_query(sicp_place db, sicp_handle h, int which, const double sensor_origin[3], int32_t first, int32_t count,
                     int32_t top_k, double min_score, sicp_place_candidate* out, int32_t* n_found) {
  return abi_guard(db, [&]() -> int {
    return place_query(db, h, which, sensor_origin, first, count, top_k, min_score, out, n_found);
  });
}

int sicp_place_query_descriptors(sicp_place db, int32_t n_q, const uint8_t* desc, int32_t first, int32_t count, int32_t top_k,
                                 double min_score, sicp_place_candidate* out, int32_t* n_found) {
  return abi_guard(db, [&]() -> int {
    return place_query_descriptors(db, n_q, desc, first, count, top_k, min_score, out, n_found);
  });
}

int sicp_place_tables(sicp_place db, double* cos_half, double* sin_half, double* edge2) {
  return abi_guard(db, [&]() -> int { return place_tables(db, cos_half, sin_half, edge2); });
}

// ---- the pose graph (graph.cpp) ------------------------------------------------------------------------------------------
int sicp_default_graph_params(sicp_graph_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    graph_default_params(p);
    return SICP_OK;
  });
}

int sicp_graph_create(int device_id, const sicp_graph_params* p, sicp_graph* out) {
  return abi_guard([&]() -> int { return graph_create(device_id, p, out); });
}

int sicp_graph_destroy(sicp_graph g) {
  return abi_guard([&]() -> int { return graph_destroy(g); });
}

int sicp_graph_clear(sicp_graph g) {
  return abi_guard(g, [&]() -> int { return graph_clear(g); });
}

int sicp_graph_size(sicp_graph g, int64_t* n_nodes, int64_t* n_edges) {
  return abi_guard(g, [&]() -> int { return graph_size(g, n_nodes, n_edges); });
}

const char* sicp_graph_last_error(sicp_graph g) { return g ? g->last_error.c_str() : ""; }

int sicp_graph_add_nodes(sicp_graph g, int32_t n, const double* qt, const uint8_t* fixed, int32_t* first_id) {
  return abi_guard(g, [&]() -> int { return graph_add_nodes(g, n, qt, fixed, first_id); });
}

int sicp_graph_add_edges(sicp_graph g, int32_t m, const int32_t* i, const int32_t* j, const double* z, const double* omega,
                         int32_t* first_id) {
  return abi_guard(g, [&]() -> int { return graph_add_edges(g, m, i, j, z, omega, first_id); });
}

int sicp_graph_add_priors(sicp_graph g, int32_t kind, int32_t m, const int32_t* node, const double* z, const double* omega,
                          int32_t* first_id) {
  return abi_guard(g, [&]() -> int { return graph_add_priors(g, kind, m, node, z, omega, first_id); });
}

int sicp_graph_set_edges_enabled(sicp_graph g, int32_t first, int32_t count, const uint8_t* enabled) {
  return abi_guard(g, [&]() -> int { return graph_set_enabled(g, false, first, count, enabled); });
}

int sicp_graph_get_edges_enabled(sicp_graph g, int32_t first, int32_t count, uint8_t* enabled) {
  return abi_guard(g, [&]() -> int { return graph_get_enabled(g, false, first, count, enabled); });
}

int sicp_graph_set_priors_enabled(sicp_graph g, int32_t first, int32_t count, const uint8_t* enabled) {
  return abi_guard(g, [&]() -> int { return graph_set_enabled(g, true, first, count, enabled); });
}

int sicp_graph_get_priors_enabled(sicp_graph g, int32_t first, int32_t count, uint8_t* enabled) {
  return abi_guard(g, [&]() -> int { return graph_get_enabled(g, true, first, count, enabled); });
}

int sicp_graph_prior_errors(sicp_graph g, double* chi2, double* residual, double* weight, double* cost) {
  return abi_guard(g, [&]() -> int { return graph_prior_errors(g, chi2, residual, weight, cost); });
}

int sicp_graph_counts(sicp_graph g, int64_t* n_nodes, int64_t* n_edges, int64_t* n_edges_enabled, int64_t* n_priors,
                      int64_t* n_priors_enabled) {
  return abi_guard(g, [&]() -> int { return graph_counts(g, n_nodes, n_edges, n_edges_enabled, n_priors, n_priors_enabled); });
}

int sicp_graph_set_poses(sicp_graph g, int32_t first, int32_t count, const double* qt) {
  return abi_guard(g, [&]() -> int { return graph_set_poses(g, first, count, qt); });
}

int sicp_graph_get_poses(sicp_graph g, int32_t first, int32_t count, double* qt) {
  return abi_guard(g, [&]() -> int { return graph_get_poses(g, first, count, qt); });
}

int sicp_graph_set_fixed(sicp_graph g, int32_t first, int32_t count, const uint8_t* fixed) {
  return abi_guard(g, [&]() -> int { return graph_set_fixed(g, first, count, fixed); });
}

int sicp_graph_errors(sicp_graph g, double* chi2, double* residual, double* weight, double* cost) {
  return abi_guard(g, [&]() -> int { return graph_errors(g, chi2, residual, weight, cost); });
}

int sicp_graph_linearize(sicp_graph g, double* gradient, double* diag_blocks, double* cost) {
  return abi_guard(g, [&]() -> int { return graph_linearize(g, gradient, diag_blocks, cost); });
}

int sicp_graph_optimize(sicp_graph g, sicp_graph_info* info) {
  return abi_guard(g, [&]() -> int { return graph_optimize(g, info); });
}

int sicp_default_graph_cov_params(sicp_graph_cov_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    graph_default_cov_params(p);
    return SICP_OK;
  });
}

int sicp_graph_marginals(sicp_graph g, const sicp_graph_cov_params* p, int32_t n, const int32_t* nodes, double* cov, int32_t* status,
                         sicp_graph_cov_info* info) {
  return abi_guard(g, [&]() -> int { return graph_covariances(g, true, p, n, nullptr, nodes, cov, status, info); });
}

int sicp_graph_relative_covariances(sicp_graph g, const sicp_graph_cov_params* p, int32_t n, const int32_t* a, const int32_t* b,
                                    double* cov, int32_t* status, sicp_graph_cov_info* info) {
  return abi_guard(g, [&]() -> int { return graph_covariances(g, false, p, n, a, b, cov, status, info); });
}

int sicp_solve(sicp_handle h, const double init_qt[7], double out_qt[7], int32_t* lm_iters, int32_t* evals,
               double* final_cost) {
  return abi_guard(h, [&]() -> int {
    if (!h || !init_qt || !out_qt) return SICP_ERR_INVALID_ARGUMENT;
    if (!h->corr_valid) return SICP_ERR_NOT_READY;
    SICPCHECK(set_device(h));
    SolveResult r;
    SICPCHECK(run_solve(h, init_qt, out_qt, &r));
    if (lm_iters) *lm_iters = r.iterations;
    if (evals) *evals = r.evaluations;
    if (final_cost) *final_cost = r.cost;
    return SICP_OK;
  });
}

int sicp_fused_labels(sicp_handle h, const double qt[7], uint32_t* out_labels) {
  return abi_guard(h, [&]() -> int {
    if (!h || !qt || !out_labels) return SICP_ERR_INVALID_ARGUMENT;
    SICPCHECK(set_device(h));
    if (h->params.mode != SICP_MODE_EM) return SICP_ERR_INVALID_ARGUMENT;
    SICPCHECK(check_ready(h, true));
    Cloud &S = h->cloud(0), &T = h->cloud(1);
    if (T.n < 4) return SICP_ERR_TOO_FEW_POINTS;
    SICPCHECK(prepare_cloud(h, S));
    SICPCHECK(prepare_cloud(h, T));
    // getFusedLabels reuses what align() left behind (em_icp.hpp:230-241)
    if (!features_current(h, S, true)) SICPCHECK(compute_features(h, S, true));
    if (!features_current(h, T, true)) SICPCHECK(compute_features(h, T, true));
    SICPCHECK(labels_search(h, qt));
    SICPCHECK(labels_launch(h, qt, h->stream));
    std::vector<uint32_t> tmp(S.n);
    if (S.n > 0) HIPCHECK(hipMemcpyAsync(tmp.data(), h->tmpl.p, sizeof(uint32_t) * S.n, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    for (int i : S.drop_i) out_labels[i] = 0;  // no correspondences, no fused label (labels are 1-based: em_icp.hpp:265)
    for (int d = 0; d < S.n; ++d) out_labels[S.caller_index(d)] = tmp[d];
    return SICP_OK;
  });
}

int sicp_se3_device(sicp_handle h, int op, int32_t n, const double* in, double* out) {
  return abi_guard(h, [&]() -> int {
    if (!h || op < SICP_SE3_EXP || op > SICP_LM_SEQUENCE_ONE_LANE || n < 0 || (n > 0 && (!in || !out))) return SICP_ERR_INVALID_ARGUMENT;
    if (n == 0) return SICP_OK;
    SICPCHECK(set_device(h));
    const bool lm_seq = op >= SICP_LM_SEQUENCE;
    const size_t n_in = lm_seq ? (size_t)sicp::kLmSeqIn : op == SICP_SE3_EXP ? 6 : (op == SICP_SE3_PLUS ? 13 : (op == SICP_SE3_MUL ? 14 : 7));
    const size_t n_out = lm_seq ? (size_t)sicp::kLmSeqOut : op == SICP_SE3_LOG ? 6 : 7;
    DevBuf<double> d_in, d_out;
    HIPCHECK(d_in.reserve(n_in * n));
    HIPCHECK(d_out.reserve(n_out * n));
    HIPCHECK(hipMemcpyAsync(d_in.p, in, sizeof(double) * n_in * n, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(sicp::launch_se3_ops(op, n, d_in.p, d_out.p, h->stream));
    HIPCHECK(hipMemcpyAsync(out, d_out.p, sizeof(double) * n_out * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return SICP_OK;
  });
}

int sicp_get_stats(sicp_handle h, sicp_stats* stats) {
  return abi_guard(h, [&]() -> int {
    if (!h || !stats) return SICP_ERR_INVALID_ARGUMENT;
    *stats = h->st;
    return SICP_OK;
  });
}

int sicp_synchronize(sicp_handle h) {
  return abi_guard(h, [&]() -> int {
    if (!h) return SICP_ERR_INVALID_ARGUMENT;
    SICPCHECK(set_device(h));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return SICP_OK;
  });
}

// ---- initial alignment without a pose prior (exec/bootstrap.h; bootstrap.cpp) ----------------------------------------
int sicp_default_bootstrap_params(sicp_bootstrap_params* p) {
  return abi_guard([&]() -> int {
    if (!p) return SICP_ERR_INVALID_ARGUMENT;
    bootstrap_default_params(p);
    return SICP_OK;
  });
}

int sicp_bootstrap(sicp_handle h, const sicp_bootstrap_params* p, double out_qt[7], sicp_bootstrap_info* info) {
  return abi_guard(h, [&]() -> int {
    if (!h) return SICP_ERR_INVALID_ARGUMENT;
    return bootstrap_run(h, p, out_qt, info);
  });
}

int sicp_bootstrap_batch(sicp_handle* hs, int32_t n, const sicp_bootstrap_params* p, double* out_qt, int32_t* status,
                         sicp_bootstrap_info* infos) {
  return abi_guard((hs && n > 0) ? hs[0] : nullptr, [&]() -> int {
    return bootstrap_batch(hs, n, p, out_qt, status, infos);
  });
}

int sicp_bootstrap_keypoints(sicp_handle h, int which, const sicp_bootstrap_params* p, int32_t capacity, int64_t nbr_capacity,
                             int32_t* n_keypoints, int64_t* n_nbrs, float* xyz3, double* normal3, float* fpfh33,
                             int64_t* nbr_offsets, int32_t* nbr_idx) {
  return abi_guard(h, [&]() -> int {
    if (!h) return SICP_ERR_INVALID_ARGUMENT;
    return bootstrap_keypoints(h, which, p, capacity, nbr_capacity, n_keypoints, n_nbrs, xyz3, normal3, fpfh33, nbr_offsets, nbr_idx);
  });
}

int sicp_bootstrap_score(sicp_handle h, const sicp_bootstrap_params* p, int32_t n, const int32_t* src_idx, const int32_t* tgt_idx,
                         double* M12, double* err, int32_t knn_capacity, int32_t* feat_knn) {
  return abi_guard(h, [&]() -> int {
    if (!h) return SICP_ERR_INVALID_ARGUMENT;
    return bootstrap_score(h, p, n, src_idx, tgt_idx, M12, err, knn_capacity, feat_knn);
  });
}

// ---- the label forms of the initial alignment (bootstrap.cpp) -------------------------------------------------------
int sicp_default_bootstrap_label_params(sicp_bootstrap_label_params* lp) {
  return abi_guard([&]() -> int {
    if (!lp) return SICP_ERR_INVALID_ARGUMENT;
    bootstrap_default_label_params(lp);
    return SICP_OK;
  });
}

int sicp_bootstrap_semantic(sicp_handle h, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp, double out_qt[7],
                            sicp_bootstrap_info* info) {
  return abi_guard(h, [&]() -> int {
    if (!h) return SICP_ERR_INVALID_ARGUMENT;
    return bootstrap_semantic_run(h, p, lp, out_qt, info);
  });
}

int sicp_bootstrap_semantic_batch(sicp_handle* hs, int32_t n, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp,
                                  double* out_qt, int32_t* status, sicp_bootstrap_info* infos) {
  return abi_guard((hs && n > 0) ? hs[0] : nullptr, [&]() -> int {
    return bootstrap_semantic_batch(hs, n, p, lp, out_qt, status, infos);
  });
}

int sicp_bootstrap_semantic_keypoints(sicp_handle h, int which, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp,
                                      int32_t capacity, int32_t* n_keypoints, float* xyz3, uint32_t* label) {
  return abi_guard(h, [&]() -> int {
    if (!h) return SICP_ERR_INVALID_ARGUMENT;
    return bootstrap_semantic_keypoints(h, which, p, lp, capacity, n_keypoints, xyz3, label);
  });
}

int sicp_bootstrap_semantic_score(sicp_handle h, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp, int32_t n,
                                  const int32_t* src_idx, const int32_t* tgt_idx, double* M12, double* err, int32_t knn_capacity,
                                  int32_t* feat_knn) {
  return abi_guard(h, [&]() -> int {
    if (!h) return SICP_ERR_INVALID_ARGUMENT;
    return bootstrap_semantic_score(h, p, lp, n, src_idx, tgt_idx, M12, err, knn_capacity, feat_knn);
  });
}

}  // extern "C"
