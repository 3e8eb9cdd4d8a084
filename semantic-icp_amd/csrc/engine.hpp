// engine.hpp -- internal header of the host side of libsicp.so (never installed; include/sicp.h is the boundary).
//
// The host side is split along its seams:
//   memory.cpp    device arena, cloud pool
//   clouds.cpp    staging, upload + search-tree build of a cloud
//   stages.cpp    stage drivers of one align(): searches, covariances, projections, weights, one evaluation
//   solve.cpp     inner solve: ticks, the persistent launch, continuous batching (BatchRun), sicp_align_batch
//   streams.cpp   registration streams (worker thread + sicp_stream_*)
//   pose_cov.cpp  sicp_pose_covariance: the sweep over a group of pairs, the 6x6 algebra
//   evaluate.cpp  sicp_evaluate: overlap, inlier RMSE and label agreement at a pose
//   merge.cpp     sicp_merge_clouds: posed clouds into one voxel-grid cloud
//   cluster.cpp   sicp_cluster: label-aware Euclidean clustering of a cloud
//   filter.cpp    sicp_filter: statistical / radius outlier removal and masked selection of a cloud
//   deskew.cpp    sicp_deskew: a scan's points moved to one instant from per-point times and a knot trajectory
//   range.cpp     sicp_range_image / sicp_range_labels: a scan's spherical projection and the vote back from per-pixel classes
//   camera.cpp    sicp_camera_image / sicp_camera_labels / sicp_camera_unproject: a scan through a pinhole camera, a depth frame out of one
//   plane.cpp     sicp_segment_planes: RANSAC plane extraction of a cloud
//   ground.cpp    sicp_segment_ground: piecewise-planar ground on a polar grid, height above it
//   map.cpp       sicp_map_*: the persistent voxel map (integrate, carve, raycast, prune, extract, merge, state)
//   elevation.cpp sicp_map_elevation: the map as a 2.5-D height grid
//   distance.cpp  sicp_map_distance: a truncated Euclidean distance field of the map
//   graph.cpp     sicp_graph_*: the pose graph (nodes, edges, linearise, optimise, blocks of H^-1)
//   sicp_api.cpp  the remaining C-ABI entry points
// Every extern "C" entry runs inside abi_guard (abi_barrier.hpp): no exception crosses the boundary.
#ifndef SICP_ENGINE_HPP_
#define SICP_ENGINE_HPP_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "abi_barrier.hpp"
#include "build_tree.h"
#include "job_table.hpp"
#include "kernels.h"
#include "lm.hpp"
#include "se3.hpp"
#include "sicp.h"

namespace sicp {
namespace host {

using sicp::se3::matrix34;

// ---- device memory arena -----------------------------------------------------------------------------
// hipMalloc costs 0.1 ... several ms and hipFree synchronises the device; a stream of registrations creates
// clouds and slot buffers all the time (a fresh cloud is ~26 buffers), on the very thread that feeds the GPU.
// Device buffers therefore come from a process-wide arena per device: slabs (64 MB doubling to 1 GB, or the
// request if larger) carved by a bump pointer into blocks of a few size classes (1/16 steps between powers of
// two: at most ~12 % slack); a released block goes to its class's free list and is handed out again for the
// same class.  Nothing is returned to the driver before sicp_release_pool, which frees the slabs of a device
// that hold no live block.  (Measured before: the align-only leg of an open stream took 0.4 or 1.3 s for the same
// 1024 registrations, depending on how the ~3000 hipMalloc calls inside it happened to go.)
constexpr int kArenaDevices = 64;
struct DevArena {
  struct Slab { char* base = nullptr; size_t size = 0, used = 0; long long live = 0; };
  struct Block { void* p; int slab; };
  struct Dev {
    std::vector<Slab> slabs;
    std::unordered_map<size_t, std::vector<Block>> free_by_class;
    size_t reserved = 0;  // bytes of all slabs (what the arena holds of the device's memory)
    size_t limit = 0;     // sicp_set_memory_limit: no new slab beyond this many bytes (0 = none)
  };
  std::mutex m;
  Dev dev[kArenaDevices];
  static size_t size_class(size_t bytes) {
    if (bytes <= 256) return 256;
    size_t p2 = 256;
    while (p2 < bytes) p2 <<= 1;
    const size_t step = std::max<size_t>(p2 >> 4, 256);
    return (bytes + step - 1) / step * step;
  }
  hipError_t alloc(size_t bytes, void** out, int* device, int* slab, size_t* cls_out) {
    int d = 0;
    hipError_t e = hipGetDevice(&d);
    if (e != hipSuccess) return e;
    const size_t cls = size_class(bytes);
    std::lock_guard<std::mutex> lock(m);
    Dev& D = dev[d % kArenaDevices];
    auto it = D.free_by_class.find(cls);
    if (it != D.free_by_class.end() && !it->second.empty()) {
      const Block b = it->second.back();
      it->second.pop_back();
      D.slabs[b.slab].live++;
      *out = b.p; *device = d; *slab = b.slab; *cls_out = cls;
      return hipSuccess;
    }
    int k = -1;
    for (int i = (int)D.slabs.size() - 1; i >= 0 && i >= (int)D.slabs.size() - 4; --i)
      if (D.slabs[i].base && D.slabs[i].size - D.slabs[i].used >= cls) { k = i; break; }
    if (k < 0) {
      size_t want = (size_t)64 << 20;
      for (const Slab& sl : D.slabs) if (sl.base) want = std::min<size_t>(std::max(want, 2 * sl.size), (size_t)1 << 30);
      want = std::max(want, cls);
      if (D.limit && D.reserved + want > D.limit) want = cls;  // (near the caller's limit: the request alone)
      if (D.limit && D.reserved + want > D.limit) return hipErrorOutOfMemory;
      Slab sl;
      e = hipMalloc((void**)&sl.base, want);
      if (e != hipSuccess && want > cls) { want = cls; e = hipMalloc((void**)&sl.base, want); }  // (memory is tight: the request alone)
      if (e != hipSuccess) return e;
      sl.size = want;
      D.reserved += want;
      k = -1;
      for (size_t i = 0; i < D.slabs.size(); ++i) if (!D.slabs[i].base) { k = (int)i; break; }  // (a slot freed by release)
      if (k < 0) { D.slabs.push_back(sl); k = (int)D.slabs.size() - 1; } else D.slabs[k] = sl;
    }
    Slab& S = D.slabs[k];
    *out = S.base + S.used;
    S.used += cls;
    S.live++;
    *device = d; *slab = k; *cls_out = cls;
    return hipSuccess;
  }
  // A block may be handed out again at once, to any thread and stream: like hipFree, giving one back first waits
  // for the device (launches that still read or write it may be in flight on streams the caller knows nothing of).
  // Releases are rare next to allocations: buffers that grow, handles and clouds (beyond the cloud pool) that go.
  // An object that gives back MANY blocks at once (a handle: ~40, a cloud beyond the pool's cap: ~26) waits for the
  // device ONCE: FreeScope does the wait, and the frees of this thread inside it skip theirs -- the blocks are the
  // dying object's own, nothing can be launched on them any more.
  static int& scope_device() { static thread_local int d = -1; return d; }
  struct FreeScope {
    int prev;
    explicit FreeScope(int device) : prev(scope_device()) {
      int cur = -1;
      const bool ok = hipGetDevice(&cur) == hipSuccess;
      const bool switched = ok && cur != device && hipSetDevice(device) == hipSuccess;
      (void)hipDeviceSynchronize();
      if (switched) (void)hipSetDevice(cur);
      scope_device() = device;
    }
    ~FreeScope() { scope_device() = prev; }
    FreeScope(const FreeScope&) = delete;
    FreeScope& operator=(const FreeScope&) = delete;
  };
  // The device scratch of a feature call (or of a stream's covariance pass) going back to the arena: `idle` is its owner's
  // word that every launch that used it has completed -- true only once the stream has been synchronised behind all of
  // them, false after an error.  Then the frees skip the device-wide wait altogether, as inside a FreeScope (which waits
  // once); otherwise, or without a device (nothing was reserved), every free waits as usual.  The scope a caller had is
  // restored.
  template <class... Bufs>
  static void release_scratch(int device, bool idle, Bufs&... bufs) {
    int& scope = scope_device();
    const int prev = scope;
    if (idle && device >= 0) scope = device;
    (bufs.release(), ...);
    scope = prev;
  }
  void free(void* p, int device, int slab, size_t cls) {
    if (scope_device() != device) {
      int cur = -1;
      const bool ok = hipGetDevice(&cur) == hipSuccess;
      const bool switched = ok && cur != device && hipSetDevice(device) == hipSuccess;
      (void)hipDeviceSynchronize();
      if (switched) (void)hipSetDevice(cur);
    }
    std::lock_guard<std::mutex> lock(m);
    Dev& D = dev[device % kArenaDevices];
    D.free_by_class[cls].push_back(Block{p, slab});
    D.slabs[slab].live--;
  }
  // frees the slabs of `device` that hold no live block (the current device must be `device`)
  void release(int device) {
    std::lock_guard<std::mutex> lock(m);
    Dev& D = dev[device % kArenaDevices];
    for (size_t i = 0; i < D.slabs.size(); ++i) {
      Slab& S = D.slabs[i];
      if (!S.base || S.live != 0) continue;
      for (auto& kv : D.free_by_class) {
        std::vector<Block>& v = kv.second;
        v.erase(std::remove_if(v.begin(), v.end(), [&](const Block& b) { return b.slab == (int)i; }), v.end());
      }
      (void)hipFree(S.base);
      D.reserved -= S.size;
      S = Slab();
    }
  }
};
DevArena& dev_arena();  // memory.cpp; never destroyed: it may outlive the HIP runtime at process exit

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  int dev_ = -1, slab_ = -1;
  size_t cls_ = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) dev_arena().free(p, dev_, slab_, cls_);
    p = nullptr;
    cap = 0;
  }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    // 64 elements of slack beyond the capacity: kernels that read whole vectors may touch up to one
    // vector past the last element (the values are never used)
    size_t want = n + n / 8;
    void* q = nullptr;
    hipError_t e = dev_arena().alloc((want + 64) * sizeof(T), &q, &dev_, &slab_, &cls_);
    if (e != hipSuccess) { p = nullptr; return e; }
    p = static_cast<T*>(q);
    cap = want;
    return hipSuccess;
  }
};

// pinned host memory: uploads and read-backs through it are real asynchronous DMA copies
// (flags: hipHostMallocCoherent for memory a running kernel writes while the host polls it)
template <class T>
struct HostBuf {
  T* p = nullptr;
  size_t cap = 0, n = 0;
  unsigned flags = hipHostMallocDefault;
  explicit HostBuf(unsigned alloc_flags = hipHostMallocDefault) : flags(alloc_flags) {}
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { if (p) (void)hipHostFree(p); }
  hipError_t resize(size_t count) {
    if (count > cap) {
      if (p) (void)hipHostFree(p);
      p = nullptr; cap = 0;
      const size_t want = count + count / 8 + 64;
      hipError_t e = hipHostMalloc((void**)&p, want * sizeof(T), flags);
      if (e != hipSuccess) { p = nullptr; n = 0; return e; }
      cap = want;
    }
    n = count;
    return hipSuccess;
  }
  hipError_t assign(const T* src, size_t count) {
    hipError_t e = resize(count);
    if (e == hipSuccess && count) std::memcpy(p, src, count * sizeof(T));
    return e;
  }
  T* data() { return p; }
  const T* data() const { return p; }
  size_t size() const { return n; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};

// A HIP stream / event its holder owns: move-only, destroyed with the holder, used wherever the raw type is.  create()
// makes the object unless it is there already.
struct OwnedStream {
  hipStream_t s = nullptr;
  OwnedStream() = default;
  OwnedStream(OwnedStream&& o) noexcept { std::swap(s, o.s); }
  OwnedStream& operator=(OwnedStream&& o) noexcept { std::swap(s, o.s); return *this; }
  ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create(unsigned flags = hipStreamNonBlocking) { return s ? hipSuccess : hipStreamCreateWithFlags(&s, flags); }
  hipStream_t get() const { return s; }
  operator hipStream_t() const { return s; }
};
struct OwnedEvent {
  hipEvent_t e = nullptr;
  OwnedEvent() = default;
  OwnedEvent(OwnedEvent&& o) noexcept { std::swap(e, o.e); }
  OwnedEvent& operator=(OwnedEvent&& o) noexcept { std::swap(e, o.e); return *this; }
  ~OwnedEvent() { if (e) (void)hipEventDestroy(e); }
  hipError_t create(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
  hipEvent_t get() const { return e; }
  operator hipEvent_t() const { return e; }
};

struct Cloud {
  int n = 0;         // points on the device (the finite ones: what the search index holds)
  int n_caller = 0;  // points the caller handed over (what every per-point output is sized by)
  // Non-finite points are left out of the device cloud, as pcl::KdTreeFLANN::setInputCloud leaves them
  // out of its index (em_icp.h:50-66): keep[i] = caller index of device-side input point i (empty when
  // nothing was dropped), drop_i / drop_xyz = the dropped points themselves (for the final_cloud output).
  std::vector<int> keep, drop_i;
  std::vector<float> drop_xyz;
  bool is_set = false, has_label = false;
  float bb_lo[3] = {0, 0, 0}, bb_hi[3] = {0, 0, 0};  // bounding box of the staged (finite) points
  bool bb_valid = false;
  HostBuf<float> hx, hy, hz;  // caller order (pinned: the staging buffers of the upload)
  HostBuf<uint32_t> hl;
  uint32_t label_min = 0, label_max = 0;  // of hl (EM labels are validated against 1..C)
  // device layout: one segment (GICP / EM) or one segment per label in first-seen order
  // (SEMANTIC); inside a segment the points are in Morton order
  int layout = -1;        // -1 none, 0 flat, 1 grouped
  HostBuf<int> perm;  // device index -> caller index
  std::vector<uint32_t> seg_label;
  std::vector<int> seg_off;  // n_seg + 1
  DevBuf<float> x, y, z;
  DevBuf<uint32_t> label;
  // search structure (bvh.hpp): packed points (x, y, z, caller index), boxes, seed tables
  struct SegTree {
    sicp::TreeLevels lv;
    int n, pt_begin, node_begin, code_begin;
    float lo[3], scale;
  };
  std::vector<SegTree> trees;
  DevBuf<float4> pts4, box_lo, box_hi;
  DevBuf<unsigned long long> leaf_code;
  DevBuf<int> inv;  // caller index -> device index
  // build scratch: the cloud as the caller gave it (the finite points in caller order: they stay valid while layout >= 0, in
  // either layout -- what sicp_merge_clouds reads), sort buffers
  DevBuf<float> rx, ry, rz;
  DevBuf<uint32_t> rl;
  DevBuf<int> ids, d_perm, vals_in, vals_out;
  HostBuf<int> h_ids;
  DevBuf<unsigned long long> keys_in, keys_out;
  DevBuf<unsigned char> sort_temp;
  // the segment table of the build (build_tree.h): one entry for a flat cloud, one per label for a grouped one
  DevBuf<sicp::BuildSegment> d_segs;
  HostBuf<sicp::BuildSegment> h_segs;
  DevBuf<sicp::PointRec> rec;  // position + normal of every point (what the weight / accumulate kernels gather)
  DevBuf<char> rec_dense;      // the same as three dense arrays (what the accumulate kernel streams for the source points and gathers for the targets)
  int rec_dense_n = 0;         // the cloud size they were written for (0: not written); set with rec, cleared wherever feat_valid is cleared
  // Caller-supplied covariances that are NOT of the form I - (1-eps) n n^T (sicp_set_covariances): the six entries xx xy xz yy
  // yz zz of every point's symmetric matrix, device order.  A handle with such a cloud evaluates through
  // accumulate_general_kernel (the literal gicp_cost_function.h:27-73 with full 3x3 matrices), one pair at a time.
  DevBuf<double> cov6;
  bool cov_general = false;
  DevBuf<uint8_t> hist;
  DevBuf<double> proj;  // [n][proj_stride(C)] label distribution x confusion matrix
  bool proj_valid = false;
  DevBuf<int> nn;
  int nn_stride = 0;  // 0: [n][k]; > 0: [k][nn_stride]
  bool feat_valid = false;
  int feat_k = 0, feat_C = 0, feat_float_products = 0;
  bool feat_hist = false;
  // which align() / align_batch() call computed the features last (a cloud shared by two handles of
  // one batch is only searched once per call), and which confusion matrix the projections belong to
  unsigned long long feat_epoch = 0;
  unsigned long long proj_cm_id = 0;
  // the upload + tree build is left running on the uploading handle's stream: whoever uses the cloud
  // next (any handle, any stream, or the host reading `perm`) waits for this event first
  OwnedEvent ready_ev;
  // set by the uploading thread, cleared by whoever waits first (a sequence driver uploads the next
  // batch's scans on a second host thread while the main thread registers clouds that share them)
  std::atomic<bool> pending{false};
  int n_seg() const { return (int)seg_label.size(); }
  int caller_index(int d) const { return keep.empty() ? perm[d] : keep[perm[d]]; }
};

// Clouds (with all their device and pinned buffers) are recycled through a per-device pool: a scan
// sequence uploads a new cloud per registration, and allocating / freeing ~25 buffers each time would
// serialise the pipeline (hipFree synchronises the device).  The pool is never destroyed (it may
// outlive the HIP runtime at process exit); sicp_release_pool frees what it holds.
constexpr int kPoolDevices = 64;
// parked clouds per device beyond which a released cloud is freed instead (two batches of 256 pairs with
// their own source and target clouds fit; ~11 MB of HBM and ~2 MB of pinned memory per 100K-point cloud)
constexpr size_t kPoolCap = 1024;
struct CloudPool {
  std::mutex m;
  std::vector<Cloud*> free_list[kPoolDevices];
};
CloudPool& cloud_pool();
std::shared_ptr<Cloud> acquire_cloud(int device);
unsigned long long next_epoch();
double now_ms();
// developer logs (SICP_KNN_STATS, SICP_SOLO_LOG, SICP_STREAM_LOG, -DSICP_SOLO_TIMING) print to stderr ONLY when
// SICP_DEBUG is set in the environment: without it the library never prints (include/sicp.h)
bool debug_enabled();

// The stage jobs of one launch sequence -- searches, covariances, projections, weights, counts, one job launch per kind
// (kernels.h: launch_*_jobs) in that order on one stream (stages.cpp: launch_slice).  A stage a handle launches for itself
// is such a sequence of one job.
struct JobSlice {
  int knn_K = 0;  // list length of the searches (one launch: one length)
  std::vector<sicp::KnnArgs> knn;
  std::vector<sicp::CovArgs> cov;
  std::vector<sicp::ProjArgs> proj;
  std::vector<sicp::WeightArgs> weight;
  std::vector<sicp::CountJob> count;
  struct Sizes { size_t knn = 0, cov = 0, proj = 0, weight = 0, count = 0; };
  Sizes sizes() const { return {knn.size(), cov.size(), proj.size(), weight.size(), count.size()}; }
  // drops the jobs appended since sizes() returned `s`
  void shrink_to(const Sizes& s) { knn.resize(s.knn); cov.resize(s.cov); proj.resize(s.proj); weight.resize(s.weight); count.resize(s.count); }
  void clear() { shrink_to(Sizes()); }
  bool empty() const { return knn.empty() && cov.empty() && proj.empty() && weight.empty() && count.empty(); }
};

// lock-step batch: instead of launching, the per-pair stages append their jobs here (stages.cpp: hand_off); the batch driver
// launches each kind once for all pairs of a slice (flush_jobs)
constexpr int kParts = 4;  // slices of a batch whose stage sequences run on their own streams

struct JobCollector {
  // EM weights written by the search's own epilogue (stages.cpp: run_correspondences) instead of a weight kernel behind it.
  // In a 16-job launch the epilogue adds 4.8 us to a 100K-point search (24.3 -> 29.1 us), the kernel it replaces takes 13.4 us
  // alone.  Set by:
  //   a batch of at most 4 pairs  every launch is on the critical path of an align() (one pair alone: -46 us of 1.98 ms);
  //   an open stream              256 pairs in flight: 167.9 against 170.6 ms per step, every run faster than every run without
  //                               in each of four alternated blocks (2.4 - 3.5 ms; twice the parent's spread in two of them);
  //   a batch of 16 pairs or more closed 256-pair batch 184.8 against 187.4 ms, 16 full-size pairs 42.3 against 43.6 ms.
  // (profiles/weights_dense/ab.json.  Since the accumulate launches hand their chunks out dynamically a search workgroup that
  // stays longer on a CU no longer delays a launch.  What a step saves is under a third of the 9.5 ms the sum of unit costs
  // predicts: most of the weight kernel ran hidden beside the accumulate launches.  Round 5's static ranges gave 0.5 %.)
  // Batches of 5 to 15 pairs were not measured and keep the kernel.
  bool fold_weights = false;
  int slice = 0;  // slice of the batch the pair whose stage is running belongs to (set by the driver)
  JobSlice part[kParts];
};

// the argument buffers of one stream of ticks (run_tick): argument array + header in HBM with pinned
// mirrors, and the instantiated [accumulate, LM step] x lm_batch graph that reads them
struct TickSet {
  // resources, and the cache that lives as long as they do: `cap`, the capacity in pairs (steps of 32) that keys the graphs
  // and caps the launches
  DevBuf<sicp::BatchArgs> d_batch;
  DevBuf<sicp::BatchHeader> d_bhdr;
  HostBuf<sicp::BatchHeader> h_bhdr;
  HostBuf<sicp::BatchArgs> h_batch;
  HostBuf<sicp::LmJoin> h_join;  // pinned: the pairs that join with the next tick
  DevBuf<sicp::LmJoin> d_join;
  int cap = 0;
  sicp::BatchGraph graph[2];   // [1]: the accumulate nodes carry kAccStaticRanges (static_ranges below)
  // state of the current use (invalidate(): what a recycled handle starts from)
  bool static_ranges = false;  // the next ticks' large accumulate launches keep equal chunk ranges (a stream while scans are being uploaded)
  std::vector<int> tick_act;  // the pairs whose arguments d_batch currently holds
  bool tick_valid = false;
  TickSet() = default;
  TickSet(const TickSet&) = delete;
  TickSet& operator=(const TickSet&) = delete;
  ~TickSet() { sicp::batch_graph_destroy(graph[0]); sicp::batch_graph_destroy(graph[1]); }
  void invalidate() { tick_valid = false; tick_act.clear(); static_ranges = false; }
};

}  // namespace host
}  // namespace sicp

using namespace sicp::host;  // (internal header: only the library's own translation units include it)

// A handle's members are of three kinds, declared apart:
//   * the state of the current use (sicp_use_state): what sicp_set_* / align() leave behind.  A recycled handle gets a
//     default-constructed one, so a member added here needs no edit anywhere else;
//   * resources a parked handle keeps (streams, events, pinned mirrors, device buffers, tick graphs), each held by an
//     owner that frees it when the handle is deleted;
//   * caches that describe the contents of a resource and live exactly as long as it does, each next to its resource.
struct sicp_use_state {
  JobCollector* collect = nullptr;
  sicp_params params;
  unsigned long long epoch = 0;  // id of the running align() / align_batch() call
  int C = 0;
  std::vector<double> cm;
  unsigned long long cm_id = 0;  // changes with every sicp_set_confusion
  // correspondences of the last search (in idx / d2 / w)
  int corr_n = 0, corr_K = 0;
  bool corr_valid = false, corr_weighted = false;
  bool hint_ok = false;  // idx holds this align()'s previous search: usable as the next search's seed hint
  // the persistent solve (solve_one_kernel) of the last pair still iterating
  int solo_pair = 0;  // the pair's state slot
  bool solo_was_init = false, solo_failed = false;  // the launch in flight starts a solve / the last one did not run to its end
  int solo_skip = 0, solo_penalty = 0;  // after a persistent launch timed out: solves that stay with the tick graph before the next try (doubling)
  bool count_stats = false;           // the align() in progress reports statistics: every search also counts its live slots
  bool counted_in_search = false;     // ... and the search kernel of the current correspondences did so itself
  // a slot of a registration stream: an upload that is still in flight (queued by the submitting thread on
  // the stream's upload stream) is waited for ON THE DEVICE, by the stream the slot's kernels run on
  bool wait_on_device = false;
  std::string last_error;
  sicp_stats st = {};
  sicp_use_state() { sicp_default_params(SICP_MODE_GICP, &params); }
};

struct sicp_context : sicp_use_state {
  int device = 0;
  bool parked = false;  // in the handle pool (sicp_destroy ... sicp_create): not the caller's any more
  std::shared_ptr<Cloud> cl[2];
  Cloud& cloud(int which) { return *cl[which]; }
  const Cloud& cloud(int which) const { return *cl[which]; }
  // ---- resources.  Members go in reverse order of declaration: graphs and pinned mirrors, then events, then streams.
  OwnedStream own_stream, own_stream2;  // (the second cloud's feature kernels run beside the first's)
  OwnedStream side_stream;              // batch leader: searches of the pairs between two inner solves
  OwnedStream feat_stream;              // batch leader: the start-up pipelines (features + first search) of a large batch
  OwnedStream part_stream[kParts];
  JobSlice own_jobs;  // the stage job this handle is launching for itself (stages.cpp: hand_off; kept for its vectors' capacity)
  // the streams this handle launches on: its own, or the ones it borrows while it is part of a batch (BatchGuard) or a
  // slot of a registration stream (the leader's side stream).  Never destroyed through these.
  hipStream_t stream = nullptr, stream2 = nullptr;
  OwnedEvent ev0, ev1, ev_join;
  OwnedEvent side_done, side_done2, main_done;
  std::vector<OwnedEvent> chunk_ev;  // one per start-up chunk
  OwnedEvent part_fork, part_done[kParts];
  DevBuf<double> d_cm, d_hval;
  int hval_k = 0;  // cache: the k that d_hval was filled for
  DevBuf<int> idx;
  DevBuf<float> d2;
  DevBuf<double> w;
  DevBuf<unsigned long long> part;
  DevBuf<double> partials, out28;
  DevBuf<long long> d_count;
  DevBuf<sicp::LmState> d_lm;
  HostBuf<sicp::LmState> h_lm;  // pinned mirror of the device-resident LM state
  HostBuf<double> h_out28;      // pinned, 28 doubles
  HostBuf<long long> h_count;   // pinned
  DevBuf<float> tmpx, tmpy, tmpz;
  DevBuf<double> tmp9;  // sicp_covariances: the 3x3 matrices in the caller's order on their way out
  DevBuf<uint32_t> tmpl;
  HostBuf<uint32_t> h_labels;  // pinned: fused labels of a stream slot on their way back
  HostBuf<unsigned char> pc_stage;  // pinned: arguments and results of the pose-covariance sweeps this handle leads (pose_cov.cpp)
  // sicp_evaluate (evaluate.cpp): the K = 1 searches of the pair, [target segments][source points] -- scratch of its own, so that
  // idx / d2 above (the correspondences) stay what they were -- and the pinned stage of the sweeps this handle leads
  DevBuf<int> ev_idx;
  DevBuf<float> ev_d2;
  HostBuf<unsigned char> ev_stage;
  // sicp_merge_clouds (merge.cpp), on the handle that leads a call: the pinned part table + counts, and the pinned result
  // (x | y | z | label | count) on its way to the caller and into dst
  HostBuf<unsigned char> mg_stage;
  HostBuf<uint32_t> mg_out;
  HostBuf<unsigned char> cl_stage;  // pinned: counts, cluster_id and table of sicp_cluster on their way back (cluster.cpp)
  // sicp_filter (filter.cpp): the pinned mask / caller indices on their way up and counts / per-point outputs on their way
  // back, and the pinned kept points (x | y | z | label) on their way into dst
  HostBuf<unsigned char> fl_stage;
  HostBuf<uint32_t> fl_out;
  // sicp_deskew (deskew.cpp): the pinned times / knots / caller indices on their way up and the counts on their way back, and the
  // pinned moved points (x | y | z | label, the caller's indices) on their way to the caller and into dst
  HostBuf<unsigned char> dk_stage;
  HostBuf<uint32_t> dk_out;
  // sicp_range_image / sicp_range_labels (range.cpp): the pinned tables / caller indices / pixel classes on their way up, the
  // counts, images and per-point outputs on their way back, and the points (x | y | z) on their way into dst
  HostBuf<unsigned char> rg_stage;
  // sicp_camera_image / sicp_camera_labels / sicp_camera_unproject (camera.cpp): the pinned caller indices / pixel classes / depth
  // frame on their way up, the counts, images and per-point outputs on their way back, and the points (x | y | z) on their way
  // into dst
  HostBuf<unsigned char> cm_stage;
  // sicp_segment_planes (plane.cpp): the pinned finite positions / mask on their way up, the control block, plane records and
  // per-point states on their way back
  HostBuf<unsigned char> pl_stage;
  // sicp_segment_ground (ground.cpp): the pinned tables / finite positions / mask on their way up, the control block, cell rows
  // and per-point outputs on their way back, and the pinned selected points (x | y | z | label) on their way into dst
  HostBuf<unsigned char> gr_stage;
  HostBuf<uint32_t> gr_out;
  // lock-step batch (sicp_align_batch), owned by the batch's first handle: one BatchArgs and one LM
  // state per pair, pinned mirrors, and the captured [accumulate_batch, lm_step_batch] x lm_batch graph
  TickSet ts[2];  // two sets: the halves of a batch alternate, one's tick runs while the host turns the other around
  DevBuf<sicp::LmState> d_bstates;
  DevBuf<double> d_bout28;
  // per-pair state mirrors, sized in steps of 32 pairs (batch_reserve).  h_bstates is also written by the persistent solve's
  // master while the host polls: coherent
  HostBuf<sicp::LmState> h_bstates{hipHostMallocCoherent};
  HostBuf<double> h_bout28;
  DevBuf<unsigned> d_solo_sync;  // hand-off words of the persistent solve
  // caches of d_solo_sync: the tags used so far (a launch uses solo_tag + 1 ...: the words are never zeroed in between), and
  // the launch counter (the state's pad_ word echoes it at a regular end; process-wide, so never stale)
  unsigned solo_tag = 0;
  int solo_seq = 0;
  // pinned, coherent: the persistent solve's master writes its launch number here at a regular end (solve.cpp: solo_wait);
  // behind the word, the landing area of the fallback copy
  HostBuf<int> h_solo_flag{hipHostMallocCoherent};

  // what a new handle is, for one that has been used: the resources and their caches stay
  void reset_use() {
    static_cast<sicp_use_state&>(*this) = sicp_use_state();
    stream = own_stream;
    stream2 = own_stream2;
    for (TickSet& S : ts) S.invalidate();
  }
};

// ---- a registration stream (sicp_stream_*): the continuous batching of sicp_align_batch without the closed
// batch.  Clouds are uploaded by the submitting thread on the stream's own upload stream; a worker thread owns
// `cap` handles (slots) and runs the tick loop: admit queued registrations into free slots, one turn, retire.
struct StreamCloudRef;
namespace sicp {
namespace host {
// the raw sums of a pose covariance: what remains to be done with them is host algebra with the caller's sigmas
struct PoseCovSums {
  double out28[28];  // hessian 21 | gradient 6 | cost
  double sums[42];   // S_src 21 | S_tgt 21
  long long active;
};
struct PoseCovStream;  // pose_cov.cpp: a stream's covariance scratch and pinned stages
}  // namespace host
}  // namespace sicp
struct sicp_stream_ctx {
  int device = 0, cap = 0;
  sicp_params params;
  int C = 0;
  std::vector<double> cm;
  std::vector<sicp_context*> slots;      // slots[0] leads: tick sets, LM states, side stream
  sicp_context* uploader = nullptr;      // runs the uploads + search-tree builds (caller's thread, own stream)
  std::mutex up_m;                       // one upload at a time
  // ---- shared between the caller's threads and the worker, under `m`
  std::mutex m;
  std::condition_variable cv_work, cv_done, cv_space;
  struct Submission {
    long long ticket;
    std::shared_ptr<Cloud> src, tgt;
    double init[7];
    unsigned flags;  // SICP_SUBMIT_*
    int overtaken = 0;  // admission rounds in which it waited for a live registration to let go of its clouds (worker only)
  };
  std::deque<Submission> queue;
  std::deque<sicp_stream_result> done;
  std::unordered_map<long long, std::vector<uint32_t>> labels;  // ticket -> getFusedLabels of a SICP_SUBMIT_FUSED_LABELS registration, until taken
  std::unordered_map<long long, PoseCovSums> cov_sums;  // ticket -> sums of a SICP_SUBMIT_POSE_COVARIANCE registration, until taken
  std::unordered_map<long long, std::shared_ptr<Cloud>> clouds;
  long long next_cloud = 1, next_ticket = 1;
  long long submitted = 0, completed = 0, busy_evals = 0, slot_evals = 0;
  std::atomic<double> last_add_ms{-1e18};  // when the last scan was added (its upload + tree build run beside the ticks)
  int draining = 0;  // callers blocked in sicp_stream_poll(wait >= 2): nothing new will be submitted by them meanwhile
  int in_flight = 0;
  bool stop = false;
  int error = 0;
  std::string error_msg;   // why the worker stopped (fatal for the stream)
  std::string api_error;   // what an entry point caught at the ABI barrier
  std::string error_copy;  // what sicp_stream_last_error last handed out (stable until its next call)
  // ---- worker only
  std::vector<long long> slot_ticket;
  std::vector<double> slot_t0;
  std::vector<unsigned> slot_flags;
  std::vector<OwnedEvent> slot_ev;  // SICP_SUBMIT_FUSED_LABELS: recorded behind the label kernel + read-back of the slot
  PoseCovStream* cov = nullptr;     // SICP_SUBMIT_POSE_COVARIANCE: reserved with the first flagged registration, released with the stream
  std::vector<int> slot_cov_stage, slot_cov_row;  // the stage of the slot's covariance pass and its row there
  std::thread worker;
};

// ---- a persistent voxel map (sicp_map_*; map.cpp): the rows of kernels.h's MapRows, sorted by key, in two sets of arena
// buffers -- a call that changes the map writes the spare set and swaps once nothing can refuse any more
struct sicp_map_ctx {
  int device = 0;
  sicp_map_params params;
  OwnedStream stream;
  struct Rows {
    DevBuf<unsigned long long> key;
    DevBuf<double> sx, sy, sz;
    DevBuf<uint32_t> cnt, hist;
  } rows[2];
  int cur = 0;               // the set that holds the map
  long long n_voxels = 0;    // <= 2^31 - 1
  unsigned long long n_points = 0;  // <= 2^32 - 1: no row's count can overflow
  DevBuf<double> logcm;      // sicp_map_set_confusion: log cm[r][s], num_classes^2 doubles (the host takes the logarithms)
  bool has_cm = false;
  HostBuf<unsigned char> stage;  // pinned: the counts' read-back
  HostBuf<uint32_t> out;         // pinned: an extract's result (x | y | z | label | count | hist rows | confidence) on its way out; an
                                 // elevation's control words and arrays
  HostBuf<uint32_t> rays;        // pinned: a ray cast's ends on their way up, then its per-ray results on their way out
  std::string last_error;
};

// ---- a database of scan descriptors (sicp_place_*; place.cpp): the entries' R*S bytes one after another in one of two arena
// buffers -- growth copies into the spare one and swaps last, so a refused call leaves the entries as they were
struct sicp_place_ctx {
  int device = 0;
  sicp_place_params params;
  int rs = 0;                      // bytes of a descriptor: n_rings * n_sectors
  OwnedStream stream;
  std::vector<double> tables;      // edge2[R + 1] | cos_half[S / 2] | sin_half[S / 2] (rule 2: host libm, in double)
  DevBuf<double> d_tables;
  DevBuf<uint8_t> store[2];
  int cur = 0;                     // the buffer that holds the entries
  long long n_entries = 0, cap_entries = 0;
  DevBuf<uint8_t> qdesc;           // the descriptors of the running call (describe's result, a query's upload)
  HostBuf<unsigned char> stage;    // pinned: read-backs and uploads on their way
  const char* call = "sicp_place";  // the entry point that is running: the head of a HIP failure's text
  std::string last_error;
};

// ---- a pose graph (sicp_graph_*; graph.cpp): nodes and edges one after another in one of two sets of arena buffers -- growth
// copies into the spare set and swaps last, so a refused call leaves the graph as it was.  The work buffers of linearise and
// optimise are sized when they are needed and kept.
struct sicp_graph_ctx {
  int device = 0;
  sicp_graph_params params;
  OwnedStream stream;
  struct Nodes { DevBuf<double> pose; DevBuf<uint8_t> fixed; } nodes[2];
  struct Edges { DevBuf<int> i, j; DevBuf<double> z, omega; DevBuf<uint8_t> enabled; } edges[2];
  struct Priors { DevBuf<int> node, kind; DevBuf<double> z, omega; DevBuf<uint8_t> enabled; } priors[2];  // z[7], omega[36] per prior
  int ncur = 0, ecur = 0, pcur = 0;   // the sets that hold the graph
  long long n_nodes = 0, n_edges = 0, n_priors = 0, cap_nodes = 0, cap_edges = 0, cap_priors = 0;
  long long n_fixed = 0, n_edges_enabled = 0, n_priors_enabled = 0;
  std::vector<uint8_t> h_fixed;       // the host's copy of the flags (optimize refuses a graph without a fixed node)
  std::vector<int32_t> h_ei, h_ej;    // the host's copy of the edge ends (the covariance calls' connectivity)
  std::vector<uint8_t> h_een;         // the host's copies of the enabled flags and of the priors' nodes and kinds
  std::vector<uint8_t> h_pen;
  std::vector<int32_t> h_pnode, h_pkind;
  std::vector<uint8_t> anchored;      // per node: its component over the enabled edges holds a fixed node or an enabled pose prior
  bool anchored_stale = true;         // nodes, edges, priors or flags have changed since
  bool incidence_stale = true;        // nodes, edges or priors have been added, or an enabled flag flipped, since the tables were built
  DevBuf<double> C, B, r, s, w, ec, H, g, L, x, rr, zz, p, q, cand, part;
  DevBuf<double> PC, pr, ps, pw;      // per prior: the record, the residual, chi2, the weight
  DevBuf<unsigned long long> keys, inc;
  DevBuf<int> deg, off, pinc, poff;   // pinc, poff: the enabled priors by node, built on the host
  DevBuf<uint8_t> pheld;              // per node: it has an enabled pose prior
  DevBuf<unsigned char> temp;
  DevBuf<sicp::GraphScalars> scalars;
  HostBuf<unsigned char> stage;       // pinned: uploads and read-backs on their way
  HostBuf<sicp::GraphScalars> rec;    // pinned: the scalars' read-back
  // the covariance calls' own work buffers (sicp_graph_marginals / _relative_covariances), sized on first use and kept; of the
  // optimiser's they reuse what every sicp_graph_optimize rewrites before it reads (the linearisation, L)
  DevBuf<double> cov_x, cov_r, cov_z, cov_p, cov_q, cov_part, cov_J, cov_out;
  DevBuf<int> cov_query, cov_bad;
  DevBuf<sicp::GraphCovColumn> cov_cols;
  HostBuf<sicp::GraphCovColumn> cov_rec;  // pinned: the columns' read-back
  HostBuf<int> cov_hquery;                // pinned: a pass's query nodes on their way up
  HostBuf<double> cov_hout;               // pinned: a pass's blocks on their way down
  const char* call = "sicp_graph";    // the entry point that is running: the head of a HIP failure's text
  std::string last_error;
};

namespace sicp {
namespace host {

template <class Body>
inline int abi_guard(sicp_graph_ctx* g, Body&& body) noexcept {
  return abi_guard_note(static_cast<Body&&>(body), [g](const char* what) {
    if (g && what) g->last_error = std::string("internal: ") + what;
  });
}

template <class Body>
inline int abi_guard(sicp_place_ctx* db, Body&& body) noexcept {
  return abi_guard_note(static_cast<Body&&>(body), [db](const char* what) {
    if (db && what) db->last_error = std::string("internal: ") + what;
  });
}

// the barrier of an entry point that has a handle / a stream: the description lands in sicp_last_error /
// sicp_stream_last_error
template <class Body>
inline int abi_guard(sicp_context* h, Body&& body) noexcept {
  return abi_guard_note(static_cast<Body&&>(body), [h](const char* what) {
    if (h && what) h->last_error = std::string("internal: ") + what;
  });
}
template <class Body>
inline int abi_guard(sicp_stream_ctx* S, Body&& body) noexcept {
  return abi_guard_note(static_cast<Body&&>(body), [S](const char* what) {
    if (!S || !what) return;
    std::lock_guard<std::mutex> lock(S->m);
    S->api_error = std::string("internal: ") + what;
  });
}

template <class Body>
inline int abi_guard(sicp_map_ctx* m, Body&& body) noexcept {
  return abi_guard_note(static_cast<Body&&>(body), [m](const char* what) {
    if (m && what) m->last_error = std::string("internal: ") + what;
  });
}

#define HIPCHECK(expr)                                                                         \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      h->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
      return _e == hipErrorOutOfMemory ? SICP_ERR_OUT_OF_MEMORY : SICP_ERR_HIP;                \
    }                                                                                          \
  } while (0)

#define SICPCHECK(expr)          \
  do {                           \
    int _s = (expr);             \
    if (_s != SICP_OK) return _s; \
  } while (0)

struct KernelTimer {
  // brackets a group of launches with events when params.profile is on
  sicp_context* h;
  bool on;
  KernelTimer(sicp_context* ctx, int bit) : h(ctx), on((ctx->params.profile & bit) != 0) {
    if (on) (void)hipEventRecord(h->ev0, h->stream);
  }
  // returns elapsed ms (synchronises the stream up to here); 0 when profiling is off
  double stop() {
    if (!on) return 0.0;
    float ms = 0.f;
    if (hipEventRecord(h->ev1, h->stream) != hipSuccess) return 0.0;
    if (hipEventSynchronize(h->ev1) != hipSuccess) return 0.0;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) return 0.0;
    return (double)ms;
  }
};

// developer aid of the feature calls (SICP_DEBUG + SICP_MERGE_LOG / SICP_MAP_LOG; tools/merge_timing.py and tools/map_timing.py
// read it): HIP-event times of a call's stages on stderr
struct StageLog {
  static constexpr int kMax = 12;
  bool on = false;
  hipStream_t st = nullptr;
  OwnedEvent ev[kMax];
  const char* name[kMax] = {};
  int n = 0;
  StageLog(bool enable, hipStream_t stream) : on(enable), st(stream) {}
  void mark(const char* what) {  // the end of stage `what` (the first mark opens the first stage)
    if (!on || n >= kMax) return;
    if (ev[n].create(hipEventDefault) != hipSuccess) { on = false; return; }
    (void)hipEventRecord(ev[n], st);
    name[n++] = what;
  }
  void print(std::string s) {  // `s`: the line's head ("sicp_merge: n_in=... n_out=...")
    if (!on || n < 2) return;
    for (int i = 1; i < n; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[i - 1], ev[i]) != hipSuccess) return;
      s += std::string(" ") + name[i] + "_ms=" + std::to_string(ms);
    }
    std::fprintf(stderr, "%s\n", s.c_str());
  }
};

// the searches of a call that must leave the handle as it was (sicp_evaluate, sicp_filter) add to its counters and timers
// (run_nn): the keeper gives them back as they were
struct StatsKeeper {
  sicp_context* h;
  sicp_stats st;
  explicit StatsKeeper(sicp_context* ctx) : h(ctx), st(ctx->st) {}
  ~StatsKeeper() { h->st = st; }
};

int set_device(sicp_context* h);

// ---- clouds.cpp ------------------------------------------------------------------------------------
void settle_cloud(Cloud& c);
int cloud_wait(sicp_context* h, Cloud& c);
// host side of an upload: the caller's arrays -> the cloud's pinned staging buffers.  The caller's layout is a base
// pointer per coordinate and one byte stride (SoA: three arrays, stride 4; a pcl::PointXYZL array: one base + 0 / 4 /
// 8, stride 32), labels likewise.  ONE pass over the cloud: finite test, copy, bounding box, label range (a scan
// sequence stages a cloud per registration on the thread that submits them: five passes were 0.3 ms per 100K points).
struct StridedCloud {
  const char *x, *y, *z, *label;  // label may be null
  long long stride, label_stride;
};
int stage_cloud(sicp_context* h, Cloud& c, int32_t n, const StridedCloud& in);
int prepare_cloud(sicp_context* h, Cloud& c);
int reserve_features(sicp_context* h, Cloud& c);
int set_cloud_common(sicp_handle h, int which, int32_t n, const StridedCloud& in);

// ---- stages.cpp ------------------------------------------------------------------------------------
// (fold: the EM weights written by the search's epilogue -- KnnArgs::w_* -- or nullptr)
struct WeightFold {
  const sicp::PointRec *srec, *trec;
  const double *sproj, *tproj;
  double* w;
  double one_m_eps;
  int C, bool_probability;
};
int run_nn(sicp_context* h, int K, const Cloud& Qc, int q_begin, int q_count, const double* M34, const Cloud& Tc,
           int tseg, bool self, float gate_sq, int* out_i, float* out_d, int timer_bit, hipStream_t stream, int out_stride = 0,
           const WeightFold* fold = nullptr);
int ensure_hval(sicp_context* h, int k, hipStream_t st = nullptr);  // (st: the handle's stream unless given)
int set_confusion(sicp_context* h, int32_t C, const double* cm, hipStream_t st);  // sicp_set_confusion, uploading on st
int ensure_proj(sicp_context* h, Cloud& c);
int compute_features(sicp_context* h, Cloud& c, bool with_hist, hipStream_t stream = nullptr);
bool features_current(const sicp_context* h, const Cloud& c, bool with_hist);
int check_ready(sicp_context* h, bool need_cm);
void fill_pose(const double* qt, sicp::Pose& p);
int segment_of(const Cloud& c, uint32_t label);
int count_active(sicp_context* h);
bool weights_from_histograms(const sicp_params& P, int K);
int run_weights(sicp_context* h, const double* qt);
int run_correspondences(sicp_context* h, const double* qt, int K, bool weights);
// sicp_correspondences without the read-back: clouds, features (and EM projections), then run_correspondences(qt, knn)
int search_at(sicp_context* h, const double* qt);
void fill_acc(sicp_context* h, sicp::AccArgs& a);
constexpr int kMaxActivePairs = 256;  // pairs one launch evaluates (12 bytes of LDS each in the accumulate kernel)
int eval28(sicp_context* h, const double* qt, double* out28);
// ---- pieces of align() shared by the single-pair and the lock-step batch drivers ---------------
struct OuterState {
  double cur[7], est[7];
  int outer = 0, count = 0;
  bool converged = false;
};

int align_begin(sicp_context* h, bool want_stats);
void outer_finish(const sicp_params& P, OuterState& o);
int align_end(sicp_context* h, const OuterState& o, double t_begin, int32_t* outer_iters, sicp_stats* stats);
int batch_slice(int p, int n, int knn);
int flush_jobs(sicp_context* h, JobCollector& jc, hipStream_t base = nullptr);

// ---- solve.cpp -------------------------------------------------------------------------------------
sicp::LmOptions lm_options(const sicp_params& P);
const char* lm_options_refused(const sicp_params& P);  // nullptr, or what sicp_set_params says about the first bad field
struct SolveResult {
  int status = 0, iterations = 0, evaluations = 0;
  double cost = 0;
};

int side_reserve(sicp_context* h);  // the leader's side stream (a batch's / a stream's searches and feature kernels) and its events
bool solo_allowed(sicp_context* h);
bool general_covariances(const sicp_context* h);  // either cloud carries caller covariances of general form
int align_host_loop(sicp_context* h, const double* init_qt, double* out_qt, int32_t* outer_iters, sicp_stats* stats);
int run_solve(sicp_context* h, const double* init_qt, double* out_qt, SolveResult* res);
bool same_solver(const sicp_params& a, const sicp_params& b);
int tickset_reserve(sicp_context* h, TickSet& S, int n);
int batch_reserve(sicp_context* h, int n);
// while a lock-step batch runs, all its handles work on the leader's stream and collect their jobs.  A handle that collects
// has ONE stream (stream2 == stream, here and for the slots of a registration stream): align_begin reads that as "nothing runs
// side by side" and queues no join.
struct BatchGuard {
  sicp_handle* hs; int n;
  std::vector<hipStream_t> s1, s2;
  BatchGuard(sicp_handle* handles, int count, JobCollector* jc, hipStream_t stream) : hs(handles), n(count), s1(count), s2(count) {
    for (int p = 0; p < n; ++p) {
      s1[p] = hs[p]->stream; s2[p] = hs[p]->stream2;
      if (jc) { hs[p]->collect = jc; hs[p]->stream = stream; hs[p]->stream2 = stream; }
    }
  }
  // from here on the pairs' own launches (memsets, searches outside the job lists) go to `stream`
  void retarget(hipStream_t stream) {
    for (int p = 0; p < n; ++p) { hs[p]->stream = stream; hs[p]->stream2 = stream; }
  }
  ~BatchGuard() {
    for (int p = 0; p < n; ++p) { hs[p]->collect = nullptr; hs[p]->stream = s1[p]; hs[p]->stream2 = s2[p]; }
  }
};
int tick_launch(sicp_context* h, TickSet& S, hipStream_t M, sicp_handle* hs, int lo, int hi, const std::vector<int>& act,
                const std::vector<int>& joining, const double (*start)[7], int len, int solo_evals = 0);
int tick_wait(sicp_context* h, hipStream_t M);
int solo_check(sicp_context* h);
int run_tick(sicp_context* h, hipStream_t M, sicp_handle* hs, int n, const std::vector<int>& act, const std::vector<int>& joining,
             const double (*start)[7], int len, int solo_evals);
// ---- continuous batching: what sicp_align_batch (a closed set of pairs) and sicp_stream_* (pairs that come
// and go) share.  Every pair runs its own sequence
//     search (transform + kNN + weights) -> inner solve -> convergence test -> search -> ...
// and the run advances in TICKS of `len` LM evaluations: one graph launch evaluates every pair that is
// inside an inner solve, while the searches of the pairs that have just finished one run on a second
// stream beside it; those pairs rejoin at the next tick.  No pair waits for another pair's solve or outer
// loop -- only for the end of the current tick.
// PAIR_FIRST: the pair's start-up pipeline (features, first search, weights) is queued on the start-up stream; it joins
// the ticks when the event of its chunk has completed
// PAIR_PASS (streams only): converged; the passes its flags ask for at the final pose (getFusedLabels, the pose covariance's
// sums) are queued and the slot waits for their read-back
enum { PAIR_FREE = -1, PAIR_NEED_SEARCH = 0, PAIR_JOINING, PAIR_SOLVING, PAIR_DONE, PAIR_FIRST, PAIR_PASS };

// pairs [lo, hi) that advance together: one tick stream, one argument set
struct TickGroup {
  int lo = 0, hi = 0;
  hipStream_t M = nullptr;
  TickSet* S = nullptr;
  hipEvent_t side_done = nullptr;
  bool pending = false, side_recorded = false;
  bool force_wait = false;  // the next tick must wait for what the side stream has been given so far (a stream's ordered feature rewrite)
  int round = 0;
  std::vector<int> act, joining, finished;
};

struct BatchRun {
  sicp_context* L = nullptr;    // leader: owns the tick sets, the LM states and the side stream
  sicp_context** hs = nullptr;  // slot -> handle
  int n = 0;                    // slots
  sicp_params P;                // what every pair of the run agrees on (same_solver)
  int len = 8;                  // LM evaluations per tick
  bool one_launch = true, want_stats = false;
  bool solo = false;            // the last pair still iterating may run its solve as persistent launches (lm_on_device != 2)
  bool acc_static = false;      // equal chunk ranges in the accumulate launches of the next tick (TickSet::static_ranges)
  hipStream_t side = nullptr;   // searches / features of the pairs between two inner solves
  struct Start { double q[7]; };
  std::vector<OuterState> o;
  std::vector<int> phase, search_round;
  std::vector<Start> starts;
  double dbg_wait_ms = 0, dbg_search_ms = 0, dbg_launch_ms = 0; long long dbg_ticks = 0, dbg_act = 0;  // developer aid (SICP_STREAM_LOG)
  bool solo_now = false;        // the tick in flight is a persistent solve
  std::vector<int> evals_seen;  // evaluations of the pair's running solve already counted in the statistics
  std::vector<int> first_chunk;        // PAIR_FIRST: the start-up chunk the pair belongs to
  std::vector<hipEvent_t> chunk_ev;    // recorded behind each chunk's start-up pipeline
  // pairs whose start-up pipeline has completed join the ticks; with `block` the host waits for the first chunk
  // that is still running (nothing else is left to do)
  int promote_started(const TickGroup& G, bool block) {
    int waiting = 0, promoted = 0;
    for (int pass = 0; pass < 2; ++pass) {
      waiting = promoted = 0;
      int first_unfinished = -1;
      for (int p = G.lo; p < G.hi; ++p) {
        if (phase[p] != PAIR_FIRST) continue;
        const hipError_t q = hipEventQuery(chunk_ev[first_chunk[p]]);
        if (q == hipSuccess) { phase[p] = PAIR_JOINING; search_round[p] = 0; ++promoted; }
        else if (q == hipErrorNotReady) { ++waiting; if (first_unfinished < 0) first_unfinished = first_chunk[p]; }
        else return -1;
      }
      if (promoted || !block || first_unfinished < 0) break;
      if (hipEventSynchronize(chunk_ev[first_unfinished]) != hipSuccess) return -1;
    }
    return waiting;
  }
  void resize(int slots) {
    n = slots;
    o.assign(slots, OuterState());
    phase.assign(slots, PAIR_FREE);
    search_round.assign(slots, 0);
    starts.assign(slots, Start());
    first_chunk.assign(slots, 0);
    evals_seen.assign(slots, 0);
  }
  // pair p starts its align() at init_qt (its handle's align_begin has run)
  void start_pair(int p, const double* init_qt) {
    o[p] = OuterState();
    std::memcpy(o[p].cur, init_qt, sizeof o[p].cur);
    phase[p] = PAIR_NEED_SEARCH;
    search_round[p] = 0;
  }
  int live(const TickGroup& G) const {
    int k = 0;
    for (int p = G.lo; p < G.hi; ++p) k += phase[p] == PAIR_NEED_SEARCH || phase[p] == PAIR_JOINING || phase[p] == PAIR_SOLVING || phase[p] == PAIR_FIRST;
    return k;
  }
  int turn(TickGroup& G, JobCollector& jc);
};

// getFusedLabels (em_icp.hpp:202-268) in two halves, so that a stream slot need not wait for it: queue the K = 4 search
// (collected into the handle's job list when it has one: flush before `labels_launch`) ...
int labels_search(sicp_context* h, const double* qt);
// ... and the label kernel behind it on `st`, device order -> h->tmpl
int labels_launch(sicp_context* h, const double* qt, hipStream_t st);
int align_batch(sicp_handle* hs, int32_t n, const double* init_qt, double* out_qt, int32_t* outer_iters, sicp_stats* stats);
// sicp_pose_covariance / _batch (pose_cov.cpp): argument checks, then the search, the accumulate sweep and the sums
int pose_covariance(sicp_context* h, const double* qt, double sigma_source, double sigma_target, sicp_pose_covariance_result* out);
int pose_covariance_batch(sicp_handle* hs, int32_t n, const double* qt, double sigma_source, double sigma_target,
                          sicp_pose_covariance_result* out, int32_t* status);
// A stream's covariance pass: the sweep of the slots whose searches at their final poses are queued on `side`, with the
// read-back and one event per sweep behind it (slot_cov_stage / slot_cov_row say where a slot's sums arrive) ...
int stream_cov_pass(sicp_stream_ctx* S, const std::vector<int>& slots, const std::vector<const double*>& qts, hipStream_t side);
hipEvent_t stream_cov_event(sicp_stream_ctx* S, int slot);
// ... the slot's sums once that event has completed (once per slot and pass), and the end of the stream's scratch (idle:
// the side stream has been waited for)
void stream_cov_take(sicp_stream_ctx* S, int slot, PoseCovSums* out);
void stream_cov_destroy(sicp_stream_ctx* S, bool idle);
// the caller's result from the sums: SICP_ERR_INVALID_ARGUMENT (nothing written) for a NULL out or a sigma that is negative or not finite
int pose_covariance_from_sums(const PoseCovSums& u, double sigma_source, double sigma_target, sicp_pose_covariance_result* out);
// sicp_evaluate / _batch (evaluate.cpp): argument checks, the K = 1 searches per target segment, the evaluation sweep
int evaluate(sicp_context* h, const double* qt, double max_dist_sq, int32_t num_classes, int64_t* confusion, int32_t* nn_idx,
             float* nn_d2, sicp_evaluate_result* out);
int evaluate_batch(sicp_handle* hs, int32_t n, const double* qt, double max_dist_sq, int32_t num_classes, int64_t* confusion,
                   sicp_evaluate_result* out, int32_t* status);
// sicp_merge_clouds (merge.cpp): argument checks, the key / sort / reduce kernels on the parts' device copies, the result's
// read-back and its way into dst (set_cloud_common)
void merge_default_params(sicp_merge_params* p);
int merge_clouds(sicp_handle* parts, const int32_t* part_which, int32_t n_parts, const double* qt, const sicp_merge_params* p,
                 sicp_context* dst, int dst_which, int32_t capacity, float* x, float* y, float* z, uint32_t* label, uint32_t* count,
                 sicp_merge_info* info);
// sicp_cluster (cluster.cpp): argument checks, the cell grid / union-find / table kernels on the cloud's device copy, the
// read-backs
void cluster_default_params(sicp_cluster_params* p);
int cluster(sicp_context* h, int which, const sicp_cluster_params* p, int32_t* cluster_id, int32_t capacity, uint32_t* label,
            int32_t* count, int32_t* first_index, double* centroid, float* bbox_min, float* bbox_max, sicp_cluster_info* info);
float cells_per_metre(float t);  // the grid's cells per metre for a tolerance / radius t (cluster.cpp)
// sicp_filter (filter.cpp): argument checks, the searches and the mean-distance / tree-sum / radius-count / flag kernels on
// the cloud's device copy, one read-back, and the kept points' way into dst (set_cloud_common)
void filter_default_params(sicp_filter_params* p);
int filter(sicp_context* h, int which, const sicp_filter_params* p, const uint8_t* mask, sicp_context* dst, int dst_which, uint8_t* keep,
           double* mean_dist, int32_t* neighbors, sicp_filter_info* info);
// sicp_deskew (deskew.cpp): argument checks, the relative knots composed on the host, the one kernel on the cloud's device copy,
// one read-back, and the moved cloud's way into dst (set_cloud_common); sicp_deskew_twist_knots: host only
int deskew(sicp_context* h, int which, const double* times, int32_t n_knots, const double* knot_time, const double* knot_qt,
           const double* ref_qt, sicp_context* dst, int dst_which, float* ox, float* oy, float* oz, double* knots_out,
           sicp_deskew_info* info);
int deskew_twist_knots(const double* delta_qt, double t0, double t1, int32_t n_knots, double* knot_time, double* knot_qt);
// sicp_range_image / sicp_range_labels (range.cpp): argument checks, the tables formed on the host, the projection / resolve /
// visible or vote kernels on the cloud's device copy, one read-back, and the relabelled cloud's way into dst (set_cloud_common);
// sicp_range_tables: host only
void range_default_params(sicp_range_params* p);
int range_tables(const sicp_range_params* p, const double* beam, double* cos_half, double* sin_half, double* row_edge);
int range_image(sicp_context* h, int which, const sicp_range_params* p, const double* beam, const float* origin, int32_t* index,
                float* range_sq, float* x, float* y, float* z, uint32_t* label, uint32_t* count, int32_t* pixel, uint8_t* visible,
                sicp_range_info* info);
int range_labels(sicp_context* h, int which, const sicp_range_params* p, const double* beam, const float* origin,
                 const uint32_t* pixel_label, sicp_context* dst, int dst_which, uint32_t* out_label, uint8_t* votes, sicp_range_info* info);
// sicp_camera_image / sicp_camera_labels / sicp_camera_unproject (camera.cpp): argument checks, the two matrices formed on the
// host, the projection / resolve / visible or labels kernels on the cloud's device copy, or the unprojection of a depth frame,
// one read-back, and the cloud's way into dst (set_cloud_common); sicp_camera_matrices: host only
void camera_default_params(sicp_camera_params* p);
int camera_matrices(const double* qt, double* cam_to_cloud, double* cloud_to_cam);
int camera_image(sicp_context* h, int which, const sicp_camera_params* p, const double* qt, int32_t* index, float* depth, float* x,
                 float* y, float* z, uint32_t* label, uint32_t* count, int32_t* pixel, float* u, float* v, uint8_t* visible,
                 sicp_camera_info* info);
int camera_labels(sicp_context* h, int which, const sicp_camera_params* p, const double* qt, const uint32_t* pixel_label,
                  sicp_context* dst, int dst_which, uint32_t* out_label, uint8_t* state, sicp_camera_info* info);
int camera_unproject(sicp_context* h, const sicp_camera_params* p, const double* qt, const uint16_t* depth_u16, const float* depth_f32,
                     const uint32_t* label, sicp_context* dst, int dst_which, float* x, float* y, float* z, uint8_t* valid,
                     sicp_camera_info* info);
// sicp_segment_planes (plane.cpp): argument checks, every round of the plane kernels queued on the handle's stream, one
// read-back
void plane_default_params(sicp_plane_params* p);
int segment_planes(sicp_context* h, int which, const sicp_plane_params* p, const uint8_t* mask, int32_t* plane_id, int32_t capacity,
                   double* coeff, int32_t* count, int32_t* hyp_index, int32_t* hyp_count, double* centroid, double* rms,
                   sicp_plane_info* info);
// sicp_segment_ground (ground.cpp): argument checks, the tables, the key / sort / segment / fit / point kernels queued on the
// handle's stream, one read-back, and the selection's way into dst (set_cloud_common); sicp_ground_tables: host only
void ground_default_params(sicp_ground_params* p);
int ground_tables(const sicp_ground_params* p, const double* ring_edge, double* cos_half, double* sin_half, double* edge2);
int segment_ground(sicp_context* h, int which, const sicp_ground_params* p, const uint8_t* mask, const double* sensor_origin,
                   const double* ring_edge, sicp_context* dst, int dst_which, const sicp_ground_out* out, sicp_ground_info* info);
// sicp_map_* (map.cpp): the persistent voxel map
void map_default_params(sicp_map_params* p);
void map_default_extract_params(sicp_map_extract_params* p);
int map_create(int device_id, const sicp_map_params* p, sicp_map_ctx** out);
int map_destroy(sicp_map_ctx* m);
int map_integrate(sicp_map_ctx* m, sicp_context* h, int which, const double* qt, const double* crop_center, double crop_range,
                  sicp_map_integrate_info* info);
int map_prune(sicp_map_ctx* m, const double* center, double range, int64_t* n_removed);
void map_default_carve_params(sicp_map_carve_params* p);
int map_carve(sicp_map_ctx* m, sicp_context* h, int which, const double* qt, const double* sensor_origin, const sicp_map_carve_params* p,
              int32_t capacity, uint32_t* miss, sicp_map_carve_info* info);
void map_default_raycast_params(sicp_map_raycast_params* p);
int map_raycast(sicp_map_ctx* m, const double* qt, const double* sensor_origin, int32_t n, const float* ex, const float* ey,
                const float* ez, const sicp_map_raycast_params* p, sicp_context* dst, int dst_which, int32_t* row, int32_t* step,
                int32_t* length, float* x, float* y, float* z, uint32_t* label, uint32_t* count, double* range_sq,
                sicp_map_raycast_info* info);
// sicp_map_elevation (elevation.cpp): argument checks, the window, the key / sort / segment / cell / stencil / point kernels
// queued on the map's stream, one read-back through the map's pinned buffer
void map_default_elevation_params(sicp_map_elevation_params* p);
int map_elevation(sicp_map_ctx* m, const double* center, const sicp_map_elevation_params* p, const sicp_map_elevation_out* out,
                  sicp_context* h, int which, const double* qt, sicp_map_elevation_info* info);
// sicp_map_distance (distance.cpp): argument checks, the window, the init / seed / sweep / final / point kernels queued on the
// map's stream, one read-back through the map's pinned buffer
void map_default_distance_params(sicp_map_distance_params* p);
int map_distance(sicp_map_ctx* m, const double* center, const sicp_map_distance_params* p, const sicp_map_distance_out* out,
                 sicp_context* h, int which, const double* qt, sicp_map_distance_info* info);
int map_extract(sicp_map_ctx* m, const sicp_map_extract_params* p, sicp_context* dst, int dst_which, int32_t capacity, float* x,
                float* y, float* z, uint32_t* label, uint32_t* count, uint32_t* hist, sicp_map_extract_info* info);
int map_set_confusion(sicp_map_ctx* m, int32_t C, const double* cm);
int map_extract_fused(sicp_map_ctx* m, const sicp_map_extract_params* p, sicp_context* dst, int dst_which, int32_t capacity, float* x,
                      float* y, float* z, uint32_t* label, uint32_t* count, double* confidence, sicp_map_extract_info* info);
int map_fused_labels(sicp_map_ctx* m, sicp_context* h, int which, const double* qt, int32_t include_own_label, int32_t min_count,
                     uint32_t* out_labels, double* out_confidence);
void map_default_merge_params(sicp_map_merge_params* p);
int map_merge(sicp_map_ctx* dst, sicp_map_ctx* src, const double* qt, const sicp_map_merge_params* p, sicp_map_merge_info* info);
int map_get_state(sicp_map_ctx* m, int64_t capacity, uint64_t* key, double* sums, uint32_t* count, uint32_t* hist, int64_t* n_rows);
int map_set_state(sicp_map_ctx* m, int64_t n, const uint64_t* key, const double* sums, const uint32_t* count, const uint32_t* hist);
// sicp_place_* (place.cpp): the database of scan descriptors
void place_default_params(sicp_place_params* p);
int place_create(int device_id, const sicp_place_params* p, sicp_place_ctx** out);
int place_destroy(sicp_place_ctx* db);
int place_describe(sicp_place_ctx* db, sicp_context* h, int which, const double* sensor_origin, uint8_t* desc, sicp_place_describe_info* info);
int place_add(sicp_place_ctx* db, sicp_context* h, int which, const double* sensor_origin, int32_t* id, uint8_t* desc,
              sicp_place_describe_info* info);
int place_add_descriptors(sicp_place_ctx* db, int32_t n, const uint8_t* desc, int32_t* first_id);
int place_get(sicp_place_ctx* db, int32_t first, int32_t count, uint8_t* desc);
int place_query(sicp_place_ctx* db, sicp_context* h, int which, const double* sensor_origin, int32_t first, int32_t count, int32_t top_k,
                double min_score, sicp_place_candidate* out, int32_t* n_found);
int place_query_descriptors(sicp_place_ctx* db, int32_t n_q, const uint8_t* desc, int32_t first, int32_t count, int32_t top_k,
                            double min_score, sicp_place_candidate* out, int32_t* n_found);
int place_tables(sicp_place_ctx* db, double* cos_half, double* sin_half, double* edge2);
// sicp_graph_* (graph.cpp): the pose graph
void graph_default_params(sicp_graph_params* p);
int graph_create(int device_id, const sicp_graph_params* p, sicp_graph_ctx** out);
int graph_destroy(sicp_graph_ctx* g);
int graph_clear(sicp_graph_ctx* g);
int graph_size(sicp_graph_ctx* g, int64_t* n_nodes, int64_t* n_edges);
int graph_add_nodes(sicp_graph_ctx* g, int32_t n, const double* qt, const uint8_t* fixed, int32_t* first_id);
int graph_add_edges(sicp_graph_ctx* g, int32_t m, const int32_t* i, const int32_t* j, const double* z, const double* omega, int32_t* first_id);
int graph_set_poses(sicp_graph_ctx* g, int32_t first, int32_t count, const double* qt);
int graph_get_poses(sicp_graph_ctx* g, int32_t first, int32_t count, double* qt);
int graph_set_fixed(sicp_graph_ctx* g, int32_t first, int32_t count, const uint8_t* fixed);
int graph_add_priors(sicp_graph_ctx* g, int32_t kind, int32_t m, const int32_t* node, const double* z, const double* omega, int32_t* first_id);
// priors = false: the edges' flags
int graph_set_enabled(sicp_graph_ctx* g, bool priors, int32_t first, int32_t count, const uint8_t* enabled);
int graph_get_enabled(sicp_graph_ctx* g, bool priors, int32_t first, int32_t count, uint8_t* enabled);
int graph_prior_errors(sicp_graph_ctx* g, double* chi2, double* residual, double* weight, double* cost);
int graph_counts(sicp_graph_ctx* g, int64_t* n_nodes, int64_t* n_edges, int64_t* n_edges_enabled, int64_t* n_priors, int64_t* n_priors_enabled);
int graph_errors(sicp_graph_ctx* g, double* chi2, double* residual, double* weight, double* cost);
int graph_linearize(sicp_graph_ctx* g, double* gradient, double* diag_blocks, double* cost);
int graph_optimize(sicp_graph_ctx* g, sicp_graph_info* info);
void graph_default_cov_params(sicp_graph_cov_params* p);
// a == NULL with marginals = true: sicp_graph_marginals of the nodes b
int graph_covariances(sicp_graph_ctx* g, bool marginals, const sicp_graph_cov_params* p, int32_t n, const int32_t* a, const int32_t* b,
                      double* cov, int32_t* status, sicp_graph_cov_info* info);

}  // namespace host
}  // namespace sicp
#endif
