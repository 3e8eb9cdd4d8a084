// kernels.h -- argument blocks and launch wrappers of the gfx950 kernels (every *_kernels.hip; the job-table convention: job_table.hpp).
#ifndef SICP_KERNELS_H_
#define SICP_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh.hpp"
#include "lm.hpp"

#ifndef SICP_HD
#define SICP_HD
#endif

namespace sicp {

struct Pose {
  double R[9];  // row-major rotation (Eigen Quaternion::toRotationMatrix of the pose)
  double t[3];
};

struct Mat4f {
  float m[16];
};

// One point as the weight / accumulate kernels gather it: position (the float32 the search ran on) and
// the unit normal of its k-neighbourhood in double (its covariance is I - (1-eps) n n^T), 48 bytes =
// three loads instead of one load from each of six arrays.  Written by cov_jobs_kernel.
// Field order: the batched accumulate kernel moves a record into LDS with three LDS-DMA loads of
// 16 + 16 + 4 bytes (the 36 bytes that carry data).
struct alignas(16) PointRec {
  double nx, ny;
  double nz;
  float x, y;
  float z;
  uint32_t pad_[3];
};
static_assert(sizeof(PointRec) == 48, "PointRec is read with three dwordx4 / dwordx2 loads");

// Build-time shape of the accumulate kernels (tuning: see DESIGN.md section 3):
//   SICP_SG4     slots per group when K is a multiple of 4 (4 = the K = 4 slots of one source point per
//                step, 2 = half of them: fewer live registers per lane)
//   SICP_ACC_OCC workgroups (of 4 waves) per CU the batched kernel is compiled for = waves per SIMD
#ifndef SICP_SG4
#define SICP_SG4 4
#endif
#ifndef SICP_ACC_OCC
#define SICP_ACC_OCC 2
#endif
constexpr int acc_slots_per_group(int K) { return K % 4 == 0 ? SICP_SG4 : 2; }

// Decomposition of a pair's correspondence slots into chunks (solve_kernels.hip): groups of
// `slots_per_group` slots; a chunk = what one 256-lane workgroup sums = 2048 m slots (m = 1 up to 1024
// chunks), every lane taking `steps` = 8 m / slots_per_group groups, 256 apart; one row of 28 partial
// sums per chunk.  Host and device compute it from the slot count alone.
struct AccGeometry {
  int n_groups, steps, chunk_groups, n_chunks;
};
SICP_HD inline AccGeometry acc_geometry(int total_slots, int slots_per_group) {
  AccGeometry g;
  const int per_lane = 8 / slots_per_group;  // groups per lane and chunk at m = 1
  g.n_groups = (total_slots + slots_per_group - 1) / slots_per_group;
  int m = (g.n_groups + 256 * per_lane * 1024 - 1) / (256 * per_lane * 1024);
  if (m < 1) m = 1;
  g.steps = per_lane * m;
  g.chunk_groups = 256 * g.steps;
  g.n_chunks = (g.n_groups + g.chunk_groups - 1) / g.chunk_groups;
  if (g.n_chunks < 1) g.n_chunks = 1;
  return g;
}

struct LossArgs {
  double cauchy_a;
  int use_sqloss;
};

// brute force: queries [q_begin, q_begin+q_count) (SoA, device order) against the packed points
// pts4[t_begin .. t_begin+t_count) = (x, y, z, caller index bits)
struct NNArgs {
  const float *qx, *qy, *qz;
  int q_begin, q_count;
  int do_xform;   // 1: query = float(M * p) (pcl::transformPointCloud), 0: query = p
  double M[12];   // rows 0..2 of the 4x4 pose matrix
  const float4* pts4;
  int t_begin, t_count;
  int chunk_len;              // targets per grid.y slice
  unsigned long long* part;   // [n_chunks][q_count][K] keys
};

struct MergeArgs {
  int q_begin, q_count, n_chunks;
  const unsigned long long* part;
  const int* inv;   // caller index -> device index of the target cloud
  float gate_sq;    // +inf for the covariance self-query
  int* out_i;       // [n][k_out] device indices of the target cloud, -1 = none / gated out
  float* out_d;     // [n][k_out] or nullptr
  int k_out;        // neighbours written per query (<= the list length K the kernels run with)
};

// one tree = one cloud segment (bvh.hpp)
struct TreeArgs {
  const float4* pts4;     // packed points of the whole cloud, every segment padded to kLeaf
  const float4* box_lo;   // boxes of all segments
  const float4* box_hi;
  const unsigned long long* leaf_code;  // first Morton code of every leaf, all segments
  TreeLevels lv;
  int n;                  // points in this segment
  int pt_begin;           // first packed point of the segment
  int node_begin;         // first box of the segment
  int code_begin;
  float lo[3];
  float scale;
};

struct KnnArgs {
  const float *qx, *qy, *qz;
  int q_begin, q_count;
  int do_xform;
  double M[12];
  TreeArgs tree;
  int self;        // queries are the tree's own points (covariance neighbourhoods)
  float gate_sq;
  const int* inv;
  int* out_i;
  float* out_d;
  int* dbg;        // nullable: [q_count][2] = (boxes tested, leaves scanned), debugging only
  const int* seed_hint;  // nullable, packet kernel: [query][hint_K] device indices found by the previous search of
                         // the same queries (the seed of the walk; any valid target index is a legal hint)
  int hint_K, t_begin;   // t_begin = device index of the target segment's first point
  int out_stride;  // 0: out_i / out_d are [query][k_out]; > 0: [k_out][out_stride] (packet kernel only: coalesced
                   // for the covariance kernel, which reads one neighbour rank of 64 points at a time)
  int k_out;       // neighbours written per query (<= the list length K the kernel runs with)
  unsigned long long* live_cnt;  // nullable, packet kernel: kLiveCounters partial counters; every wave adds the number of
                                 // neighbours it wrote that passed the gate (statistics: sicp_stats.total_active)
  // EM weights in the search's epilogue (packet kernel, K = 4, at most 16 classes; w_out == nullptr: not wanted).  The lane
  // that writes a neighbour's index already holds everything em_weight_rows4_jobs_kernel would re-read -- the index, the query's
  // place -- so it gathers the two records and projection rows and writes the slot's weight beside the index: the same
  // operations in the same order as that kernel (em_icp.hpp:84-89,108), hence the same bits.  The pose is M (rows [R | t]).
  const PointRec *w_srec, *w_trec;
  const double *w_sproj, *w_tproj;  // [n][proj_stride(w_C)]
  double* w_out;                    // [query][k_out]
  double w_one_m_eps;
  int w_C, w_bool_probability;
};
constexpr int kLiveCounters = 1024;  // (spread: ~6 of a 100K-query search's 6250 waves per counter)

struct CovArgs {
  int n, k, C;
  const float *x, *y, *z;
  const uint32_t* label;  // nullable
  const int* nn;          // neighbour lists, device indices: [n][k], or [k][nn_stride] when nn_stride > 0
  int nn_stride;
  int float_products;
  PointRec* rec;          // out: position + normal of every point
  uint8_t* hist;          // [n][hist_stride(C)] or nullptr
  char* rec_dense;        // out, nullable: the same 36 data bytes per point as three dense arrays (dense_rec_*)
  int rec_dense_n;        // points the dense arrays are laid out for (their pitch)
};

// The records again, dense: [n] x 16 B (nx ny) | [n] x 16 B (nz x y) | [n] x 4 B (z).  What the accumulate kernel STREAMS
// -- the source points of a pass, in order -- is read from here: 36 bytes per point from HBM instead of the 48 of a
// record.  Its GATHERS of target records come from here too: neighbouring source points hit neighbouring targets, and 4 (16)
// consecutive targets share a 64-byte line of a 16-byte (4-byte) array where a 48-byte record shares its lines with at most
// one neighbour ("dense gathers").  Every writer of `rec` writes this copy beside it.
SICP_HD inline size_t dense_rec_bytes(int n) { return (size_t)(n > 0 ? n : 1) * 36; }
// The accumulate kernel's GATHERS of target records come from the dense arrays too (AccArgs::trec_dense), addressed as an
// array's base plus a 32-bit byte offset 16 j: clouds beyond this size keep the record path.
constexpr int kDenseGatherMaxPoints = 1 << 27;

// rows of the label histograms (uint8 neighbour counts) are padded to 16 bytes: one aligned dwordx4 load fetches the row of up
// to 16 classes (the EM weight kernel gathers a target's 16-byte row instead of its 96-byte projection row)
SICP_HD inline int hist_stride(int C) { return (C + 15) & ~15; }

// rows of the projection arrays are padded to an even number of doubles: 16-byte aligned, read with
// dwordx4 loads by the weight kernels
SICP_HD inline int proj_stride(int C) { return (C + 1) & ~1; }

struct ProjArgs {
  int n, C;
  const uint8_t* hist;  // [n][hist_stride(C)] neighbour counts
  const double* cm;     // C*C row-major
  const double* hval;   // hval[c] = c additions of 1/k (em_icp.hpp:279,301)
  double* proj;         // [n][proj_stride(C)]
};

struct WeightArgs {
  int n_s, K, C;
  const int* idx;
  const PointRec *srec, *trec;
  const double *s_proj, *t_proj;  // [n][proj_stride(C)] label distributions projected through CM (proj_*_jobs_kernel); unused with histograms
  // K = 4, C <= 16: the weights straight from the label histograms (rows of hist_stride(C) = 16 bytes), the projections
  // formed in the kernel -- the same sums in the same order as proj_body's, so the same bits -- from cm / hval
  const uint8_t *s_hist, *t_hist;  // nullable: then s_proj / t_proj are read
  const double *cm, *hval;         // C*C row-major; hval[c] = c additions of 1/k
  Pose pose;
  double one_m_eps;
  int bool_probability;
  double* w;
};

struct AccArgs {
  int n_s, K;
  const int* idx;
  const double* w;  // nullable (weight 1)
  const PointRec *srec, *trec;
  const char* srec_dense;  // nullable: the source records as dense arrays (dense_rec_*), pitch n_s
  const char* trec_dense;  // nullable: the target records as dense arrays, pitch n_t: the staged kernel gathers from them
  int n_t, pad_;           // (null: from the 48-byte records)
  Pose pose;            // used when lm == nullptr
  const LmState* lm;    // device-resident solve: evaluate at lm->pose, skip when it has finished
  LmState* lm_step;     // batched solve: the state lm_step_batch_kernel advances (== lm)
  double one_m_eps;
  LossArgs loss;
  double* partials;  // [28][accumulate_blocks]
};

// One evaluation of ONE pair whose covariances are (partly) the caller's own, of general form: full symmetric 3x3 matrices
// (six doubles per point, device order; nullptr: that cloud's are I - (1-eps) n n^T from its records).  Same columns of
// partials[28][n_chunks] as the product kernel writes, summed by the same finalize_batch_kernel.
struct GenAccArgs {
  AccArgs a;
  const double *scov6, *tcov6;
  int n_chunks, pad_;
};
hipError_t launch_accumulate_general(const GenAccArgs& g, hipStream_t st);

// job arrays passed by value to one launch (every stage job of a lock-step batch's slice; one job when a handle launches a
// stage for itself); sized to stay inside the 4 KB of kernel arguments
constexpr int kMaxKnnJobs = 8;
constexpr int kMaxSmallJobs = 16;
struct KnnJobs { KnnArgs job[kMaxKnnJobs]; };
struct CovJobs { CovArgs job[kMaxSmallJobs]; };
struct ProjJobs { ProjArgs job[kMaxSmallJobs]; };
struct WeightJobs { WeightArgs job[kMaxKnnJobs]; };
struct CountJob { const int* idx; int n; unsigned long long* out; };
struct CountJobs { CountJob job[kMaxSmallJobs]; };
static_assert(sizeof(KnnJobs) <= 4000 && sizeof(WeightJobs) <= 4000 && sizeof(CovJobs) <= 4000, "kernel argument segment");
// What every launch_*_jobs wrapper does with its n jobs: chunk after chunk of at most as many as one array holds, copied
// into it, handed to launch(array, jobs in it, largest work(job) among them) -- unless none of them has any work.
template <class Jobs, class Job, class Work, class Launch>
inline void for_job_chunks(const Job* jobs, int n, Work work, Launch launch) {
  constexpr int cap = (int)(sizeof(Jobs) / sizeof(Job));
  for (int b = 0; b < n; b += cap) {
    const int cnt = n - b < cap ? n - b : cap;
    Jobs J;
    int mx = 0;
    for (int i = 0; i < cnt; ++i) {
      J.job[i] = jobs[b + i];
      const int w = work(J.job[i]);
      mx = w > mx ? w : mx;
    }
    if (mx > 0) launch(J, cnt, mx);
  }
}

// one pair of a lock-step batch (sicp_align_batch); an array of these lives in HBM
struct BatchArgs {
  AccArgs a;
  int nb;    // columns of this pair's partials ([28][nb]): its chunks
  int pad_;
};
// what the batched kernels need to know about the current launch; lives in HBM next to the BatchArgs
// array, so the instantiated graph never changes
//
// next_run / runs_left: the work-split counters of accumulate_staged_kernel (the next run to hand out, the workgroups that
// have left the launch).  The host uploads them as zeros with the header; a launch that takes the dynamic split leaves them
// at zero again (its last workgroup out resets them), and one that does not never touches them.  So two launches that may
// take the split must never be in flight on one header at once.  A handle's TickSet header (engine.hpp) is read by the ticks
// tick_launch queues on its stream M -- a pair's own solve (run_solve, M = h->stream), a lock-step batch (the leader's two
// streams, one TickSet each), an open stream (its worker's stream, slot 0's ts[0]) -- and, ts[0]'s, by the evaluation hook
// (eval28, sicp_accumulate_batch) on h->stream.  Every one of these calls queues its launches on ONE stream, in order, and
// waits for them before it returns; a handle is driven by one thread at a time (include/sicp.h), and a stream's slots are
// the library's own handles.  So the accumulate launches on one header run one after another.
struct BatchHeader {
  int n_pairs;          // entries of the BatchArgs array (pairs whose solve has ended are skipped on the device)
  unsigned next_run;    // first chunk of the next run to hand out
  unsigned runs_left;   // workgroups of the launch that have left
  int pad_;
};
static_assert(sizeof(BatchHeader) == 16, "the header is uploaded as one 16-byte record");

// [accumulate, lm_step_batch] x len of a lock-step batch as an instantiated graph with explicit
// kernel nodes and fixed grids (solve_kernels.hip)
constexpr int kMaxBatchLen = 32;
struct BatchGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int len = 0, K = 0, sqloss = 0, capacity = 0, static_ranges = 0;
  const BatchArgs* batch = nullptr;
  const BatchHeader* hdr = nullptr;
};
// *built is set to 1 when the graph had to be (re)instantiated
// static_ranges: every accumulate node carries kAccStaticRanges
hipError_t batch_graph_prepare(BatchGraph& g, int K, int use_sqloss, BatchHeader* hdr, const BatchArgs* batch, int capacity, int len,
                               int* built, int static_ranges = 0);
void batch_graph_destroy(BatchGraph& g);

// neighbour-list length the search kernels run with for a request of k neighbours (the k nearest
// are the first k of any longer exact list): 1, 4, 20 or 32; 0 = unsupported (k < 1 or k > 32)
int nn_list_len(int k);
bool nn_k_supported(int K);
int nn_queries_per_thread(int K);
hipError_t launch_nn_partial(int K, const NNArgs& a, int n_chunks, hipStream_t st);
hipError_t launch_nn_merge(int K, const MergeArgs& m, hipStream_t st);
hipError_t launch_bvh_knn_quad(int K, const KnnArgs& a, hipStream_t st);
// sicp_covariances' fast path: the n 3x3 matrices (row-major) in the CALLER's point order, formed on the device from the records'
// normals (C = I - (1 - eps) n n^T) or from the caller's own general matrices (cov6 != nullptr); perm = device -> caller index
hipError_t launch_cov9_caller_order(int n, const PointRec* rec, const double* cov6, const int* perm, double one_m_eps, double* out9, hipStream_t st);
// caller-supplied normals (sicp_set_covariances): the point records and their dense copy, as cov_jobs_kernel writes them
hipError_t launch_set_normals(int n, const float* x, const float* y, const float* z, const double* normal3, PointRec* rec, char* rec_dense,
                              int rec_dense_n, hipStream_t st);
hipError_t launch_fused_labels(const WeightArgs& a, uint32_t* out, hipStream_t st);
hipError_t launch_bvh_knn_packet_jobs(int K, const KnnArgs* jobs, int n, hipStream_t st);
// The one stage that keeps a single-job kernel: a search with a list longer than 1 (K = 4, 20 or 32) that a handle launches
// for itself.  As one job of the job kernel the K = 4 search of a 100K-point pair took 56.2-57.3 us against 54.4-54.8, the
// k = 20 self-search 76.9-79.0 against 76.2-76.7 (profiles/single_job_launches/ab.json, the block of the earlier builds; an
// earlier set of k = 20 rounds, 77.3-78.1 against 76.2-77.5, was still inside the parent's range; K = 32 is k = 20's two-wave
// form and goes with it, unmeasured); the K = 1 search and every other stage measure the same either way.
hipError_t launch_bvh_knn_packet(int K, const KnnArgs& a, hipStream_t st);
hipError_t launch_cov_jobs(const CovArgs* jobs, int n, hipStream_t st);
hipError_t launch_proj_jobs(const ProjArgs* jobs, int n, hipStream_t st);
hipError_t launch_em_weight_jobs(const WeightArgs* jobs, int n, hipStream_t st);
hipError_t launch_count_active_jobs(const CountJob* jobs, int n, hipStream_t st);
int accumulate_blocks(int total, int K);  // chunks of a pair with `total` slots, K correspondences per source point
// every pair of the batch in one launch: hdr / batch in HBM (the launch may use hdr's work-split counters), capacity = slots
// of the batch buffers; flags = kAccStaticRanges: equal contiguous chunk ranges even for a large launch (see
// accumulate_staged_kernel)
constexpr int kAccStaticRanges = 0x40000000;
hipError_t launch_accumulate_batch(int K, int use_sqloss, BatchHeader* hdr, const BatchArgs* batch, int capacity, hipStream_t st, int flags = 0);
hipError_t launch_lm_step_batch(const BatchHeader* hdr, const BatchArgs* batch, int capacity, hipStream_t st);
// one pair alone: the whole inner solve of batch[0] in one persistent launch (one workgroup per chunk); its partials
// buffer holds TWO sets of columns, sync = max_evals + 1 words (word 0 is raised when a device-wide wait timed out)
bool solve_one_fits(int total_slots, int K);
constexpr int kSoloMaxEvals = 1024;   // evaluations one persistent launch may run (a solve that needs more is relaunched)
constexpr int kSoloSyncWords = 288;   // its hand-off words (zeroed once, when allocated); 16 words of developer timers follow

hipError_t launch_finalize_batch(const BatchArgs* batch, int n, double* out28, hipStream_t st);
// pairs that start an inner solve with the next tick: their LM states are initialised ON the device from
// one small upload (states[j.pair] = lm_init(j.opt, j.start)) instead of one 800-byte copy per pair
struct LmJoin {
  int pair, pad_;
  double start[7];
  LmOptions opt;
};
hipError_t launch_lm_init(const LmJoin* joins, int n, LmState* states, hipStream_t st);
// One persistent launch of the last pair still iterating (solve_kernels.hip: solve_one_kernel); everything it
// needs travels in the kernel arguments: no upload, no state initialisation kernel, no memset ahead of it.
struct SoloArgs {
  AccArgs a;           // the pair; a.lm_step = its trust-region state in HBM
  unsigned* sync;      // kSoloSyncWords hand-off words (+ 16 developer timers)
  int max_evals;       // evaluations this launch may run
  int wait_ticks;      // 100 MHz ticks before a wait gives up
  unsigned tag_base;   // the launch's hand-off tags are tag_base + 1 ... tag_base + max_evals: older words never match
  int init;            // 1: the inner solve starts with this launch (state := lm_init(opt, start)), 0: it continues
  int seq;             // written to the state's pad_ word at a regular end: the host's proof the launch ran to it
  int pad_;
  // nullable: pinned, device-visible host memory.  At a regular end the master also writes the state THERE (plain stores, a
  // system-scope fence) and then `seq` into *host_flag: the host polls that word instead of waiting for a read-back copy
  // behind the kernel (copy kernel + completion signal + wake-up: ~30 us between an inner solve and the next search of a
  // pair alone, four or five times per align()).
  LmCore* host_state;
  int* host_flag;
  double start[7];
  LmOptions opt;
};
hipError_t launch_solve_one(int K, int use_sqloss, const SoloArgs& args, int n_chunks, hipStream_t st);
int solo_wait_ticks();
// test hook: csrc/se3.hpp on the device, one lane per item (op = SICP_SE3_*; in/out strides per op)
// op 5 / 6: the trust-region machine fed with a given sequence of evaluations, as the kernels run it (a whole wave) / as the host
// runs it (one lane): in = n x kLmSeqIn (start pose | kLmSeqEvals x 28 sums), out = n x kLmSeqOut (the final state)
constexpr int kLmSeqEvals = 24, kLmSeqIn = 7 + 28 * kLmSeqEvals, kLmSeqOut = 37;
hipError_t launch_se3_ops(int op, int n, const double* in, double* out, hipStream_t st);
hipError_t launch_transform_float(int n, const float* x, const float* y, const float* z, const Mat4f& M,
                                  float* ox, float* oy, float* oz, hipStream_t st);

// ---- the pose covariance's sums (pose_cov_kernels.hip; driver: pose_cov.cpp) ----
// Per active slot i, B_i^p and B_i^q = d g_i / d p and d g_i / d q (6x3 each, g_i the slot's share of the gradient); per source
// point G_j = sum of its slots' B^p, per target point G_k = sum of B^q over the slots that hit it; S = sum G G^T (21 sums each).
// No float atomics: source points are a lane's own slots, target points are summed through the slots sorted by (target, slot).
constexpr int kPoseCovTile = 8;  // sorted slots per lane of the target-side pass (the split unit of long target lists)
struct PoseCovArgs {
  int n_s, K;
  const int* idx;           // [n_s][K] device target indices, -1 = gated out
  const double* w;          // nullable: weight 1
  const PointRec *srec, *trec;
  Pose pose;
  double one_m_eps, cauchy_a;
  int use_sqloss, pad_;
  double* bq;               // out: [n_s * K][18] B^q of every active slot, row-major 6x3
  unsigned long long* key;  // out: [n_s * K] job | target | slot (PoseCovJob), target = n_t for a gated-out slot
  double* part_src;         // out: [21][pose_cov_blocks(n_s)]
  long long* part_active;   // out: [pose_cov_blocks(n_s)]
};
SICP_HD inline int pose_cov_blocks(int items) { return items > 0 ? (items + 255) / 256 : 0; }
SICP_HD inline int pose_cov_tiles(int total) { return (total + kPoseCovTile - 1) / kPoseCovTile; }
// Job form (job_table.hpp): one launch of each kernel over every pair of a group (a lone call is a group of one).  A job's
// workgroups: pose_cov_blocks(n_s) of the source kernel, pose_cov_blocks(tiles) of the tile and the owner kernel, 43 of the
// finalize (which indexes the jobs by position).  A job keeps the column layout and the summation order of a launch of
// its own -- column = workgroup within the job, the butterfly per wave, the four waves in order, the columns in order -- so
// its sums have the same bits whatever else the launch holds.
// The keys of all jobs are sorted at once: key = job << (tgt_bits + slot_bits) | target << slot_bits | slot, target = n_t for a
// gated-out slot (last within its job), the three widths those of the group's largest job.  Job j's keys occupy
// [off_j, off_j + n_s K) of the key array before and after the sort, so a tile never spans two jobs.
struct PoseCovJob {
  PoseCovArgs a;                   // a.key: the job's range of the group's key array
  const unsigned long long* skey;  // the same range of the sorted keys
  double* piece;                   // [tiles][2][18] partial target sums of lists that cross a tile edge
  int* flag;                       // [tiles]
  double* part_tgt;                // [21][2 * pose_cov_blocks(tiles)]
  double* out42;                   // [S_src 21 | S_tgt 21]
  long long* active;               // active slots
  unsigned long long job_key;      // job << (tgt_bits + slot_bits)
  int n_t, slot_bits, tgt_bits, pad_;
};
hipError_t launch_pose_cov_src_jobs(const PoseCovJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st);
// (between the two: prim_sort_keys of the group's keys, bits [0, end_bit))
hipError_t launch_pose_cov_tile_jobs(const PoseCovJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st);
hipError_t launch_pose_cov_owner_jobs(const PoseCovJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st);
// fixed-order sums of the partial columns -> out42, active of every job
hipError_t launch_pose_cov_finalize_jobs(const PoseCovJob* jobs, int nj, hipStream_t st);

// ---- how well the clouds fit at a pose (evaluate_kernels.hip; driver: evaluate.cpp) ----
// sicp_evaluate: per source point the nearest target of the whole target cloud (K = 1 searches, one per target segment, their
// winners merged by (d^2, caller index)), the gate, and over the inliers: counts, the sum of d^2, the label confusion table.
// Job form (job_table.hpp): one launch over every pair of a group, eval_blocks(n_s) workgroups per job; the finalize indexes
// the jobs by position.
constexpr int kEvalChunk = 256;         // queries per partial sum: fixed, whatever the launch looks like
constexpr int kEvalChunksPerBlock = 8;  // consecutive chunks one workgroup walks (what its LDS table collects before it is flushed)
constexpr int kEvalLdsClasses = 64;     // confusion tables up to 64 x 64 are privatised in LDS (16 KB of 32-bit counts)
struct EvalOut {
  long long inliers, label_agree, label_outside;
  double sum_d2;
};
struct EvalJob {
  int n_s, n_seg;          // queries (device order of the source); target segments whose winners are merged
  const int* idx;          // [n_seg][n_s] device target indices, -1 = gated out (the search's own strict float compare)
  const float* d2;         // [n_seg][n_s] float32 d^2 of every segment's winner, gated out or not
  const uint32_t *slabel, *tlabel;  // device order; both null when either cloud has no labels
  const int *sperm, *tperm;         // device index -> caller index (among the finite points)
  float gate_sq;
  int C;                   // classes of the table (0: none)
  unsigned long long* conf;  // nullable: [C][C], zeroed before the launch
  int* nn_idx;             // nullable: [n_s] by source caller index: the winner's caller index, -1 when it is no inlier
  float* nn_d2;            // nullable: [n_s] likewise, the winner's d^2 whatever the gate says
  double* part_sum;        // [eval_chunks(n_s)] sum of the inliers' d^2 per chunk
  int* part_cnt;           // [eval_chunks(n_s)][4] inliers, equal labels, labels outside 1..C, unused
  EvalOut* out;
};
SICP_HD inline int eval_chunks(int n_s) { return n_s > 0 ? (n_s + kEvalChunk - 1) / kEvalChunk : 0; }
SICP_HD inline int eval_blocks(int n_s) { return (eval_chunks(n_s) + kEvalChunksPerBlock - 1) / kEvalChunksPerBlock; }
hipError_t launch_evaluate_jobs(const EvalJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st);
// the chunk partials of every job in index order, by one wave per job -> out
hipError_t launch_evaluate_finalize_jobs(const EvalJob* jobs, int nj, hipStream_t st);

// ---- posed clouds into one voxel-grid cloud (merge_kernels.hip; driver: merge.cpp) ----
// sicp_merge_clouds: every finite point of every part, transformed as the search transforms its queries, cropped, keyed by
// its voxel of an absolute grid, sorted (stable: the global indices ascend inside a voxel), and reduced per voxel in that
// order.  All parts go through ONE key launch: the parts are its jobs (job_table.hpp), 256 points per workgroup.
constexpr int kMergeBias = 1 << 20;  // |voxel coordinate| < 2^20: three biased 21-bit fields, z highest, bit 63 clear
struct MergePart {
  const float *x, *y, *z;  // the part's finite points in caller order (Cloud::rx ...)
  const uint32_t* label;   // nullable
  double M[12];            // rows 0..2 of the pose's 4x4 matrix
  int n, off;              // points; global index of the first
};
struct MergeKeyArgs {
  const MergePart* parts;
  const int* blk_end;
  int n_parts;
  int voxel, crop;         // leaf_size > 0; crop_range > 0
  float inv_leaf;          // 1.0f / (float)leaf_size
  float cx, cy, cz;        // (float)crop_center
  double range_sq;         // crop_range * crop_range
  float *tx, *ty, *tz;     // [n_in] transformed points by global index
  uint32_t* tlabel;        // [n_in], nullable
  unsigned long long* key; // [n_in] voxel key (0 without a grid), ~0 for a cropped point
  int* val;                // [n_in] global index
  int* res;                // kMergeRes words, zeroed before the launch
};
enum { kMergeKept = 0, kMergeOut = 1, kMergeRange = 2, kMergeMaxCount = 3, kMergeRes = 4 };
struct MergeReduceArgs {
  int n;                          // n_in
  int voxel, labels;
  const unsigned long long* skey; // sorted keys
  const int* sval;                // their global indices
  int *flag, *pos, *heads;        // [n] first-of-voxel flags, their exclusive scan, first sorted position of every voxel
  const float *tx, *ty, *tz;
  const uint32_t* tlabel;
  float *gx, *gy, *gz;            // [n] the transformed points in sorted order
  unsigned long long* lkey;       // [n] voxel rank << 32 | label in sorted order (~0 past the kept points)
  const unsigned long long* lsorted;  // lkey sorted (lkey itself without a grid: every voxel is one point)
  float *ox, *oy, *oz;            // [n] the result
  uint32_t *olabel, *ocount;
  int* res;
};
hipError_t launch_merge_keys(const MergeKeyArgs& a, int blocks, hipStream_t st);
// (the sorts and the scan between them: prim_kernels.hip)
hipError_t launch_merge_heads(const MergeReduceArgs& a, hipStream_t st);    // flag
hipError_t launch_merge_gather(const MergeReduceArgs& a, hipStream_t st);   // heads, res[kept, out], gx gy gz, lkey
hipError_t launch_merge_centroids(const MergeReduceArgs& a, hipStream_t st);  // ox oy oz, ocount, res[max count]
hipError_t launch_merge_labels(const MergeReduceArgs& a, hipStream_t st);   // olabel

// ---- label-aware Euclidean clustering (cluster_kernels.hip; driver: cluster.cpp) ----
// sicp_cluster: the finite points of one cloud in caller order (Cloud::rx ...; index i below is a position in that order).
// A cell grid finds the close pairs, a union-find over i in HBM joins them, integer atomics size the components, a scan over
// the roots numbers the clusters, and a sort by (cluster, i) feeds the ordered per-cluster sums.
constexpr int kClusterCellLimit = (1 << 20) - 1;  // |cell coordinate| < 2^20 - 1: a neighbour's biased coordinate stays in its 21-bit field
constexpr int kClusterMaxIgnore = 64;             // SICP_CLUSTER_MAX_IGNORE
enum { kClKept = 0, kClCells = 1, kClRange = 2, kClComponents = 3, kClClusters = 4, kClMaxCount = 5, kClClustered = 6, kClRes = 8 };
struct ClusterArgs {
  int n;                           // finite points
  int same_label, labels;          // params; the cloud has labels
  int n_ignore;
  int min_points, max_points;      // max_points: INT_MAX for "no limit"
  float inv, t2;                   // cells per metre (cluster_kernels.hip: the proof); (float)tol * (float)tol
  uint32_t ignore[kClusterMaxIgnore];
  const float *x, *y, *z;
  const uint32_t* label;           // nullable
  unsigned long long *key, *skey;  // [n] cell key by i (~0: not a vertex); sorted
  int *val, *sval;                 // [n] i; i in sorted order
  int *flag, *pos;                 // [n] scratch of the two scans
  int* heads;                      // [n + 1] first sorted position of every cell; heads[n_cells] = n_kept
  unsigned long long* ckey;        // [n] key of every cell, ascending
  float4* spt;                     // [n] sorted order: x, y, z, label bits
  int* parent;                     // [n] union-find; after the flatten pass the root (the component's smallest i)
  int* size;                       // [n] component size at its root
  int* cid;                        // [n] cluster number by i, -1 outside every cluster
  unsigned long long *mkey, *msorted;  // [n] cluster << 32 | i (~0 outside every cluster); sorted
  unsigned long long *lkey, *lsorted;  // [n] cluster << 32 | label; sorted (same_label = 0 with labels only)
  int* mheads;                     // [n + 1] first position of every cluster in msorted; mheads[n_clusters] = n_clustered
  uint32_t* olabel;                // [n_clusters] the table
  int *ocount, *ofirst;
  double* ocentroid;               // [3 n_clusters]
  float *obmin, *obmax;            // [3 n_clusters]
  int* res;                        // kClRes words, zeroed before the first launch
};
hipError_t launch_cluster_keys(const ClusterArgs& a, hipStream_t st);       // key, val, parent = i, size = 0, res[range]
// (prim_sort_pairs key, val -> skey, sval)
hipError_t launch_cluster_cell_flags(const ClusterArgs& a, hipStream_t st); // flag
// (prim_scan_int flag -> pos)
hipError_t launch_cluster_cells(const ClusterArgs& a, hipStream_t st);      // heads, ckey, spt, res[kept, cells]
hipError_t launch_cluster_pairs(const ClusterArgs& a, hipStream_t st);      // parent: a workgroup per cell and chunk of its points
hipError_t launch_cluster_sizes(const ClusterArgs& a, hipStream_t st);      // parent flattened, size
hipError_t launch_cluster_root_flags(const ClusterArgs& a, hipStream_t st); // flag, res[components, max count, clustered]
// (prim_scan_int flag -> pos)
hipError_t launch_cluster_ids(const ClusterArgs& a, hipStream_t st);        // cid, mkey, lkey, res[clusters]
// (prim_sort_keys mkey -> msorted, lkey -> lsorted)
hipError_t launch_cluster_member_heads(const ClusterArgs& a, hipStream_t st);              // mheads
hipError_t launch_cluster_table(const ClusterArgs& a, int n_clusters, hipStream_t st);    // the table: one wave per cluster

// ---- outlier removal and masked selection (filter_kernels.hip; driver: filter.cpp) ----
// sicp_filter: the finite points of one cloud in caller order (Cloud::rx ...; index f below is a position in that order, `caller`
// maps it to the caller's index when points were dropped).  The cloud's own search trees give every query its distance list,
// a lane per query turns it into the mean distance, a fixed binary tree over the caller's indices sums them, the cluster's
// cell grid (launch_cluster_keys ... launch_cluster_cells with the radius as the tolerance) counts the neighbours inside the
// radius, and a flag per point, its scan and a gather write the kept cloud.
constexpr int kFilterMaxLabels = 16;  // SICP_FILTER_MAX_LABELS
constexpr int kFilterTreeRun = 512;   // caller indices one workgroup of the tree sum reduces: a power of two
enum { kFlTested = 0, kFlProtected = 1, kFlKept = 2, kFlFailStat = 3, kFlFailRadius = 4, kFlRes = 8 };
enum { kFlRemoved = 0, kFlProtect = 1, kFlTest = 2 };  // a point's class (rule 1)
struct FilterStats { double s1, s2, mean, stddev, threshold; };
struct FilterArgs {
  int n, n_caller;                 // finite points; points the caller handed over
  int labels;                      // the cloud has labels
  int mean_k, min_neighbors;       // mean_k = 0: the statistical test is off; min_neighbors = 0: the radius test is off
  int n_drop, n_protect;
  uint32_t drop[kFilterMaxLabels], protect[kFilterMaxLabels];
  double std_mul;
  float r2;                        // (float)radius * (float)radius
  const float *x, *y, *z;          // [n] by f
  const uint32_t* label;           // nullable
  const int* caller;               // [n] f -> caller index; nullptr: the identity
  const uint8_t* mask;             // [n_caller] nullable
  const int* perm;                 // [n] device order -> f (Cloud::d_perm)
  uint8_t* cls;                    // [n] kFlRemoved / kFlProtect / kFlTest by f
  float *list, *list2;             // [n][list_k] ascending d2 per query in device order: the merged lists; one segment's
  int list_k;                      // mean_k + 1
  // the cell grid (ClusterArgs of the same names)
  const int* heads;
  const unsigned long long* ckey;
  const float4* spt;
  const int* sval;
  const int* grid_res;             // the grid's kClRes words
  int* nb;                         // [n] by f: min(neighbours inside the radius, min_neighbors), zeroed before the count
  int *flag, *pos;                 // [n] kept flags by f and their exclusive scan
  // outputs by caller index
  uint8_t* okeep;                  // [n_caller]
  double* omd;                     // [n_caller] NaN unless tested with the statistical test on
  int* onb;                        // [n_caller] -1 unless tested with the radius test on
  float *ox, *oy, *oz;             // [n] the kept points, ascending caller index
  uint32_t* ol;
  FilterStats* stats;
  int* res;                        // kFlRes words, zeroed before the first launch
};
hipError_t launch_filter_classes(const FilterArgs& a, hipStream_t st);     // cls, okeep = 0, omd = NaN, onb = -1, res[tested, protected]
hipError_t launch_filter_merge_lists(const FilterArgs& a, hipStream_t st); // list <- the list_k smallest of list and list2
hipError_t launch_filter_mean_dist(const FilterArgs& a, hipStream_t st);   // omd of the tested points
// one level of the tree sums: count entries -> ceil(count / kFilterTreeRun) partial sums.  first: the entries are omd (NaN is
// an absent entry: +0.0), the sums are of m and of m m; else the entries are the partials in1 / in2
hipError_t launch_filter_tree_sum(const double* in1, const double* in2, int count, int first, double* out1, double* out2, hipStream_t st);
hipError_t launch_filter_threshold(const FilterArgs& a, const double* s1, const double* s2, hipStream_t st);  // stats
hipError_t launch_filter_radius_count(const FilterArgs& a, hipStream_t st);  // nb: a workgroup per cell and chunk of its points
hipError_t launch_filter_flags(const FilterArgs& a, hipStream_t st);       // flag, okeep, onb, res[fail stat, fail radius]
// (prim_scan_int flag -> pos)
hipError_t launch_filter_gather(const FilterArgs& a, hipStream_t st);      // ox oy oz ol, res[kept]

// ---- deskewing a scan (deskew_kernels.hip; driver: deskew.cpp) ----
// sicp_deskew: the finite points of one cloud in caller order (Cloud::rx ...; index f is a position in that order, `caller` maps
// it to the caller's index when points were dropped), every point's time at its caller index, and the relative knots the host
// composed (rule 2).  One launch: the table goes to LDS, a lane finds its interval by binary search, blends the two knots,
// forms the rotation and moves its point; the outputs sit at the caller's index.
constexpr int kDeskewMaxKnots = 1024;  // SICP_DESKEW_MAX_KNOTS
constexpr int kDeskewMaxGroups = 512;  // the launch is at most this many workgroups of 256: more points stride over them
enum { kDkMoved = 0, kDkBadTime = 1, kDkClampedLo = 2, kDkClampedHi = 3, kDkRes = 4 };
struct DeskewArgs {
  int n;                    // finite points
  int n_knots;
  const float *x, *y, *z;   // [n] by f
  const int* caller;        // [n] f -> caller index; nullptr: the identity
  const double* times;      // [n_caller]
  const double* knot_time;  // [n_knots]
  const double* knot_qt;    // [n_knots][7]
  float *ox, *oy, *oz;      // [n_caller]; only the entries of finite points are written
  int* res;                 // kDkRes words, zeroed before the launch
};
hipError_t launch_deskew(const DeskewArgs& a, hipStream_t st);

// ---- range image and labels from it (range_kernels.hip; driver: range.cpp) ----
// sicp_range_image / sicp_range_labels: the finite points of one cloud in caller order (Cloud::rx ...; index f, `caller` as in
// DeskewArgs) projected into H x W pixels.  Project: the tables in LDS, a lane per point, two bisections, one 64-bit atomicMin
// on the pixel's key (bits(r2) << 32 | f: f ascends with the caller's index) and one atomicAdd on its count.  Resolve: a lane per
// pixel decodes the key, gathers the winner into a 16-byte record (x, y, z, word) and writes the dense outputs.  Then a lane
// per point either marks the winners (visible) or votes over the records of its window.
constexpr int kRangeMaxWidth = 4096;   // SICP_RANGE_MAX_WIDTH
constexpr int kRangeMaxHeight = 256;   // SICP_RANGE_MAX_HEIGHT
constexpr int kRangeMaxWindow = 7;     // SICP_RANGE_MAX_WINDOW
constexpr int kRangeMaxK = 16;         // SICP_RANGE_MAX_K
constexpr int kRangeMaxGroups = 1024;  // a per-point launch is at most this many workgroups of 256: more points stride over them
constexpr unsigned long long kRangeEmptyKey = ~0ull;  // no point holds it: the bits of r2 are those of a finite float
enum { kRgKept = 0, kRgOutsideFov = 1, kRgPixelsHit = 2, kRgVoted = 3, kRgRes = 4 };
struct RangeArgs {
  int n, n_caller;             // finite points; points the caller handed over
  int W, H;
  int clockwise, col_shift;
  int window, k;               // the vote
  float ox, oy, oz;            // the sensor's origin
  double min_sq, max_sq;       // the range bounds, squared on the host
  double max_dist_sq;          // the vote
  const float *x, *y, *z;      // [n] by f
  const uint32_t* label;       // [n] by f, nullable
  const int* caller;           // [n] f -> caller index; nullptr: the identity
  const double* tables;        // row_edge [H + 1] | cos_half [W / 2] | sin_half [W / 2]
  const uint32_t* pixel_label; // [H W] the vote; nullptr: the records' word is the cloud's label
  unsigned long long* key;     // [H W] set to kRangeEmptyKey before the projection
  uint32_t* count;             // [H W] zeroed before the projection
  int* pix;                    // [n] by f: row W + col or -1
  float4* rec;                 // [H W] the winner's x, y, z and a word; x = NaN in an empty pixel
  // dense outputs, [H W], every one nullable
  int* o_index;
  float *o_range_sq, *o_x, *o_y, *o_z;
  uint32_t* o_label;
  // per-point outputs by caller index, [n_caller], preset for the points that are not finite; every one nullable
  int* o_pixel;                // preset -1
  uint8_t* o_visible;          // preset 0
  uint32_t* o_out_label;       // preset 0
  uint8_t* o_votes;            // preset 0
  int* res;                    // kRgRes words, zeroed before the first launch
};
hipError_t launch_range_project(const RangeArgs& a, hipStream_t st);  // key, count, pix, o_pixel, res[kept, outside fov]
hipError_t launch_range_resolve(const RangeArgs& a, hipStream_t st);  // rec, the dense outputs, res[pixels hit]
hipError_t launch_range_visible(const RangeArgs& a, hipStream_t st);  // o_visible
hipError_t launch_range_vote(const RangeArgs& a, hipStream_t st);     // o_out_label, o_votes, res[voted]

// ---- camera: depth frames and image labels (camera_kernels.hip; driver: camera.cpp) ----
// sicp_camera_image / sicp_camera_labels: the finite points of one cloud in caller order (index f, `caller` as in DeskewArgs)
// through cloud -> camera, the depth gate, the Brown-Conrady distortion and the pinhole into H x W pixels.  Project: a lane per
// point, everything in double, one 64-bit atomicMin on the pixel's key (bits((float)Zc) << 32 | f) and one atomicAdd on its
// count.  Resolve: a lane per pixel decodes the key and gathers the winner into a 16-byte record (x, y, z, depth; depth = +inf
// in an empty pixel).  Then a lane per point either marks the winners (visible) or takes the smallest depth of its window
// and decides between seen, occluded and unclassed.  sicp_camera_unproject: a lane per pixel of a depth frame, the fixed-count
// undistortion in registers, the point through camera -> cloud.
constexpr int kCameraMaxWidth = 4096;   // SICP_CAMERA_MAX_WIDTH
constexpr int kCameraMaxHeight = 4096;  // SICP_CAMERA_MAX_HEIGHT
constexpr int kCameraMaxWindow = 15;    // SICP_CAMERA_MAX_WINDOW
constexpr int kCameraMaxIterations = 64;
constexpr int kCameraMaxGroups = 1024;  // a per-point launch is at most this many workgroups of 256: more points stride over them
constexpr unsigned long long kCameraEmptyKey = ~0ull;  // no point holds it: f is below 2^31
enum { kCmKept = 0, kCmOutside = 1, kCmPixelsHit = 2, kCmLabelled = 3, kCmOccluded = 4, kCmUnclassed = 5, kCmValid = 6, kCmRes = 8 };
struct CameraArgs {
  int n, n_caller;             // finite points; points the caller handed over
  int W, H;
  int window, iterations;
  double m[12];                // project: cloud -> camera; unproject: camera -> cloud (rows of 4)
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
  double min_depth, max_depth, max_tan_sq, depth_scale;
  double occlusion_abs, occlusion_rel;
  const float *x, *y, *z;      // [n] by f
  const uint32_t* label;       // [n] by f, nullable
  const int* caller;           // [n] f -> caller index; nullptr: the identity
  const uint32_t* pixel_label; // [H W] sicp_camera_labels
  unsigned long long* key;     // [H W] set to kCameraEmptyKey before the projection
  uint32_t* count;             // [H W] zeroed before the projection
  int* pix;                    // [n] by f: row W + col or -1
  float* zf;                   // [n] by f: (float)Zc of a point with a pixel
  float4* rec;                 // [H W] the winner's x, y, z and depth; depth = +inf in an empty pixel
  // dense outputs, [H W], every one nullable
  int* o_index;
  float *o_depth, *o_x, *o_y, *o_z;
  uint32_t* o_label;
  // per-point outputs by caller index, [n_caller], preset for the points that are not finite; every one nullable
  int* o_pixel;                // preset -1
  float *o_u, *o_v;            // preset NaN
  uint8_t* o_visible;          // preset 0
  uint32_t* o_out_label;       // preset 0
  uint8_t* o_state;            // preset 0
  // sicp_camera_unproject: exactly one of the two depths; the points and flags per pixel
  const uint16_t* depth_u16;
  const float* depth_f32;
  float *p_x, *p_y, *p_z;      // [H W]
  uint8_t* p_valid;            // [H W] nullable
  int* res;                    // kCmRes words, zeroed before the first launch
};
hipError_t launch_camera_project(const CameraArgs& a, hipStream_t st);    // key, count, pix, zf, o_pixel, o_u, o_v, res[kept, outside]
hipError_t launch_camera_resolve(const CameraArgs& a, hipStream_t st);    // rec, the dense outputs, res[pixels hit]
hipError_t launch_camera_visible(const CameraArgs& a, hipStream_t st);    // o_visible
hipError_t launch_camera_labels(const CameraArgs& a, hipStream_t st);     // o_out_label, o_state, res[labelled, occluded, unclassed]
hipError_t launch_camera_unproject(const CameraArgs& a, hipStream_t st);  // p_x p_y p_z, p_valid, res[valid]

// ---- RANSAC plane extraction (plane_kernels.hip; driver: plane.cpp) ----
// sicp_segment_planes: every array below that is [n_caller] long is indexed by the caller's index i; `finv` maps it to the
// position f of the point among the finite ones (Cloud::rx ...), -1 for a point that is not finite.  A round compacts the
// candidates not yet assigned, a lane per hypothesis samples a plane, the score kernel counts every hypothesis' inliers per
// tile of candidates with plain stores, a sum and an argmax pick the winner, and the membership pass, the tree sums (the
// filter's scheme: a perfect binary tree over the caller's indices), the one-lane fit and the re-selection make the plane.
// Every kernel of a round returns at once when ctl->done is set: the rounds are queued without a host synchronisation.
constexpr int kPlaneMaxIgnore = 16;      // SICP_PLANE_MAX_IGNORE
constexpr int kPlaneMaxPlanes = 16;      // SICP_PLANE_MAX_PLANES
constexpr int kPlaneLanePoints = 4;      // candidates a lane of the score kernel keeps in registers
constexpr int kPlaneTile = 256 * kPlaneLanePoints;  // candidates one workgroup of the score kernel tests
constexpr int kPlaneHypGroup = 64;       // hypotheses one workgroup of the score kernel loops over
constexpr int kPlaneTreeRun = 512;       // caller indices one workgroup of a tree sum reduces: a power of two
struct PlaneHyp { double ax, ay, az, nx, ny, nz, thr, nn; };  // a point, a normal, thr = (t t) nn (-1: invalid), nn = n . n
struct PlaneRec { double coeff[4], centroid[3], rms; int count, hyp_index, hyp_count, pad_; };
struct PlaneCtl {
  int done, m, n_planes, rounds;   // the call has ended; candidates of the round; planes found; rounds scored
  int cnt, n_candidates, n_assigned, pad_;  // members of the pass under way; candidates of round 0; points in planes
  long long n_invalid;             // invalid hypotheses over the rounds scored
  PlaneHyp model;                  // the plane the membership pass tests: the winner, then the fit
};
struct PlaneArgs {
  int n, n_caller, labels;         // finite points; points the caller handed over; the cloud has labels
  int H, min_inliers, refine, n_ignore, has_axis;
  uint32_t ignore[kPlaneMaxIgnore];
  double tt, axis[3], mc2, aa;     // t t; the axis, min_cos min_cos and axis . axis (has_axis only)
  unsigned long long seed;
  const float *x, *y, *z;          // [n] by f
  const uint32_t* label;           // [n] nullable
  const int* finv;                 // [n_caller] i -> f or -1; nullptr: the identity
  const uint8_t* mask;             // [n_caller] nullable
  int* state;                      // [n_caller] -2: no candidate; -1: a candidate not yet assigned; r: the round that took it
  int *flag, *pos;                 // [n_caller] state == -1 and its exclusive scan
  float *cx, *cy, *cz;             // [m] the round's candidates in ascending caller index
  uint8_t* member;                 // [n_caller] the pass' members
  PlaneHyp* hyp;                   // [H]
  int* partial;                    // [tiles][H] inliers per tile of candidates
  int* total;                      // [H]
  double *sum_f, *sum_c;           // the tree sums' levels, the last one first: x y z e e (4 channels); the six products
  PlaneCtl* ctl;
  PlaneRec* rec;                   // [kPlaneMaxPlanes]
};
inline int plane_tiles(long long m) { return (int)((m + kPlaneTile - 1) / kPlaneTile); }
// doubles the levels of a tree sum over n_caller entries take: 6 per workgroup of every level
inline size_t plane_tree_doubles(long long n_caller) {
  size_t total = 0;
  for (long long cnt = n_caller > 0 ? n_caller : 1;;) {
    cnt = (cnt + kPlaneTreeRun - 1) / kPlaneTreeRun;
    total += 6 * (size_t)cnt;
    if (cnt == 1) return total;
  }
}
hipError_t launch_plane_init(const PlaneArgs& a, hipStream_t st);          // state, ctl->n_candidates
hipError_t launch_plane_flags(const PlaneArgs& a, hipStream_t st);         // flag
// (prim_scan_int flag -> pos)
hipError_t launch_plane_compact(const PlaneArgs& a, hipStream_t st);       // cx cy cz, ctl->m
hipError_t launch_plane_sample(const PlaneArgs& a, int round, hipStream_t st);  // hyp
hipError_t launch_plane_score(const PlaneArgs& a, hipStream_t st);         // partial: a workgroup per tile and hypothesis group
hipError_t launch_plane_winner(const PlaneArgs& a, int round, hipStream_t st);  // total; ctl->model, done, rounds, n_invalid; rec hyp_*
hipError_t launch_plane_members(const PlaneArgs& a, hipStream_t st);       // member, ctl->cnt
hipError_t launch_plane_tree_sums(const PlaneArgs& a, int products, hipStream_t st);  // sum_f (products = 0) or sum_c, every level
hipError_t launch_plane_fit(const PlaneArgs& a, int round, hipStream_t st);      // refine = 1: ctl->model and rec coeff from the sums
hipError_t launch_plane_record(const PlaneArgs& a, int round, hipStream_t st);   // rec, ctl->n_planes, n_assigned
hipError_t launch_plane_assign(const PlaneArgs& a, int round, hipStream_t st);   // state of the members

// ---- piecewise-planar ground on a polar grid (ground_kernels.hip; driver: ground.cpp) ----
// sicp_segment_ground: arrays [n_caller] long are indexed by the caller's index i, `finv` as in PlaneArgs.  The key kernel gives
// every point its cell and sort key (a point that is no candidate sorts behind every cell, under cell R*S), one stable sort of
// the pairs, a pass that finds every cell's segment and writes the sorted coordinates densely, the fit kernel -- one wave per
// cell -- and the per-point flag / height pass.  Nothing waits for the host.
constexpr int kGroundMaxRings = 64, kGroundMaxSectors = 256;  // SICP_GROUND_MAX_RINGS, SICP_GROUND_MAX_SECTORS
constexpr int kGroundMaxIgnore = 16;                          // SICP_GROUND_MAX_IGNORE
constexpr int kGroundSortBits = 32 + 15;                      // cell <= R*S = 2^14 above the 32 bits of z
enum { kGroundEmpty = 0, kGroundOk = 1, kGroundTooFew = 2, kGroundNotUpright = 3, kGroundTooHigh = 4, kGroundTooThick = 5 };
struct GroundCell { double normal[3], centroid[3], lambda_min, lpr; int status, n_members, n_ground, n_fit; };  // centroid: g of rule 5
struct GroundCtl { int n_candidates, n_below, n_selected, pad_; };
struct GroundArgs {
  int n, n_caller, labels;         // finite points; points the caller handed over; the cloud has labels
  int R, S, n_lpr, n_iter, min_points, elevation_rings, select, n_ignore;
  uint32_t ignore[kGroundMaxIgnore];
  double org[3];                   // sensor_origin
  double below, elev;              // -(sensor_height + max_below); -sensor_height + max_elevation
  double th_seeds, th_dist, min_cos, thick2;  // thick2: max_thickness max_thickness, 0: the test is off
  const double* tables;            // edge2 [R+1] | cos_half [S/2] | sin_half [S/2]
  const float *x, *y, *z;          // [n] by f
  const uint32_t* label;           // [n] nullable
  const int* finv;                 // [n_caller] i -> f or -1; nullptr: the identity
  const uint8_t* mask;             // [n_caller] nullable
  unsigned long long *key, *skey;  // [n_caller] rule 3's key, before and after the sort
  int *val, *sval;                 // [n_caller] the caller's index, likewise
  int* cellv;                      // [n_caller] the cell of an inside point, -1 otherwise
  uint8_t* cand;                   // [n_caller]
  float *sx, *sy, *sz;             // [n_caller] the candidates' coordinates in sorted order
  int *seg_begin, *seg_end;        // [R*S + 1] a cell's segment of the sorted arrays; zeroed before
  GroundCell* cells;               // [R*S]
  uint8_t* oground;                // [n_caller]
  double* oheight;                 // [n_caller]
  int *flag, *pos;                 // [n_caller] selected for dst and its exclusive scan (select != 0)
  float *gx, *gy, *gz;             // [n_selected] the selection in ascending caller index
  uint32_t* gl;                    // nullable
  GroundCtl* ctl;                  // zeroed before
};
hipError_t launch_ground_keys(const GroundArgs& a, hipStream_t st);      // key, val, cellv, cand, ctl->n_candidates, n_below
// (prim_sort_pairs key, val -> skey, sval over bits [0, kGroundSortBits))
hipError_t launch_ground_segments(const GroundArgs& a, hipStream_t st);  // seg_begin, seg_end, sx sy sz
hipError_t launch_ground_fit(const GroundArgs& a, hipStream_t st);       // cells
hipError_t launch_ground_points(const GroundArgs& a, hipStream_t st);    // oground, oheight, flag
// (prim_scan_int flag -> pos)
hipError_t launch_ground_select(const GroundArgs& a, hipStream_t st);    // gx gy gz gl, ctl->n_selected

// ---- the persistent voxel map (map_kernels.hip; driver: map.cpp) ----
// sicp_map_*: per occupied voxel of merge's grid one row -- key, f64 sums, count, label histogram -- in arrays sorted by key.
// An integrate keys and sorts the SCAN (the key arithmetic of voxel_key.hpp, merge's heads and gather launches), finds every
// scan voxel in the map by binary search, moves the map's rows once into the spare buffers with the new voxels' rows opened
// between them, and continues every touched row's sums in point order by the one lane that owns it.  The map is never sorted.
struct MapRows {
  unsigned long long* key;  // ascending
  double *sx, *sy, *sz;
  uint32_t* cnt;
  uint32_t* hist;           // [rows][stride], nullptr when the map keeps no labels
};
// the words of an integrate's read-back; the first two are merge's (launch_merge_gather writes them)
enum { kMapKept = kMergeKept, kMapScanVoxels = kMergeOut, kMapRange = 2, kMapBadLabel = 3, kMapNew = 4, kMapOut = 5, kMapMaxCount = 6, kMapRes = 8 };
struct MapKeyArgs {
  const float *x, *y, *z;   // the scan's finite points in caller order (Cloud::rx ...)
  const uint32_t* label;    // nullptr when the map keeps no labels
  double M[12];
  int n, crop, num_classes;
  float inv_leaf, cx, cy, cz;
  double range_sq;
  float *tx, *ty, *tz;      // [n] transformed points
  unsigned long long* key;  // [n] voxel key, ~0 for a dropped point
  int* val;                 // [n] point index
  int* res;                 // kMapRes words, zeroed before the launch
};
struct MapFoldArgs {
  int n;                           // scan points: the bound of its voxels (their number is res[kMapScanVoxels])
  int n_map, n_new;                // rows before the call; rows it opens (known after the first read-back)
  int stride;                      // num_classes + 1; 0 without labels
  const unsigned long long* skey;  // the scan's sorted keys
  const int* heads;                // first sorted position of every scan voxel
  const float *gx, *gy, *gz;       // the transformed points in sorted order
  const unsigned long long* lkey;  // low word: the label in sorted order
  int *rank, *miss, *mpos;         // [n] per scan voxel: lower bound among the map's keys; 1 when absent; exclusive scan of that
  unsigned long long* miss_key;    // [n_new] the absent keys, ascending
  int* miss_rank;                  // [n_new] their lower bounds
  int* src_of;                     // [n_map + n_new] the old row a new row continues, -1 for an opened one
  int* res;
  MapRows from, to;
};
hipError_t launch_map_keys(const MapKeyArgs& a, hipStream_t st);
hipError_t launch_map_lookup(const MapFoldArgs& a, hipStream_t st);   // rank, miss
hipError_t launch_map_misses(const MapFoldArgs& a, hipStream_t st);   // miss_key, miss_rank, res[kMapNew]
hipError_t launch_map_scatter(const MapFoldArgs& a, hipStream_t st);  // to.{key, sums, cnt}, src_of
// to[r][*] = src_of[r] >= 0 ? from[src_of[r]][*] : 0 for `rows` histogram rows of `stride` bins
hipError_t launch_map_move_hist(const uint32_t* from, uint32_t* to, const int* src_of, long long rows, int stride, hipStream_t st);
hipError_t launch_map_fold(const MapFoldArgs& a, hipStream_t st);     // to.{sums, cnt, hist} of the touched rows
// prune and extract: a flag per row, its scan (prim_scan_int), a gather
struct MapSelectArgs {
  int n_map, stride;
  long long min_count;
  int crop;
  float cx, cy, cz;
  double range_sq;
  MapRows rows;
  int *flag, *pos, *src_of;             // [n_map]
  MapRows to;                           // prune: the survivors' rows
  unsigned long long* kept_points;      // prune: the sum of the survivors' counts (zeroed before the launch)
  float *ox, *oy, *oz;                  // extract: [n_map] centroids, counts, arg-max labels (nullptr without labels)
  uint32_t *ocount, *olabel;
  int* res;                             // res[kMapOut]: selected rows; res[kMapMaxCount]: extract's largest count
};
hipError_t launch_map_select(const MapSelectArgs& a, hipStream_t st);
hipError_t launch_map_prune(const MapSelectArgs& a, hipStream_t st);
hipError_t launch_map_extract(const MapSelectArgs& a, hipStream_t st);
// free-space carving (sicp_map_carve): every ray of a scan, from the sensor's voxel to its return's, walks the grid by the
// arithmetic of voxel_key.hpp (VoxelRay) and looks every candidate voxel up among the map's keys; a row counts the rays that
// pass through it (integer atomics: any order gives the same counts) and is flagged when a return lands in it.  A wave owns
// kCarveRaysPerWave consecutive rays and hands them to its lanes as they fall idle, so a long ray does not hold 63 finished
// lanes; a step along x finds its row beside the previous one (the key moves by 1), a step along y gallops from it.  The rows
// to keep then go through prune's scan and compaction.
constexpr int kCarveRaysPerWave = 128;
constexpr int kMapMaxProtect = 64;  // SICP_MAP_MAX_PROTECT
enum { kCarveRays = 0, kCarveSteps, kCarveTouched, kCarveHit, kCarveRemoved, kCarveSparedHit, kCarveSparedLabel, kCarveStats = 8 };
struct MapCarveArgs {
  const float *x, *y, *z;   // the scan's finite points in caller order (Cloud::rx ...)
  double M[12];
  int n;
  float inv_leaf;
  float sx, sy, sz;         // (float)sensor_origin, transformed in the kernels as a point is
  int ranged;               // max_range > 0
  double range_sq;
  int end_margin;
  const unsigned long long* key;  // the map's keys, ascending
  int n_map;
  int* hit;                 // [n_map] zeroed: 1 where a return lands
  uint32_t* miss;           // [n_map] zeroed: rays that pass through
  unsigned long long* stat; // kCarveStats words, zeroed
  int* res;                 // res[kMapRange]: the origin lies beyond the key's range (zeroed before the launch)
};
struct MapCarveSelectArgs {
  int n_map, stride, min_rays, n_protect;
  uint32_t protect[kMapMaxProtect];
  const uint32_t* hist;     // nullptr when the map keeps no labels
  const int* hit;
  const uint32_t* miss;
  int* flag;                // [n_map] 1: the row stays
  unsigned long long* stat;
};
hipError_t launch_map_carve_hits(const MapCarveArgs& a, hipStream_t st);    // hit, res[kMapRange] (launched for n = 0 too)
hipError_t launch_map_carve_walk(const MapCarveArgs& a, hipStream_t st);    // miss, stat[rays, steps]
hipError_t launch_map_carve_select(const MapCarveSelectArgs& a, hipStream_t st);  // flag, stat[touched ... spared]
// ray casting (sicp_map_raycast): carve's walk, stopped at the first voxel whose row is opaque.  One lane per row first writes
// an opaque byte (count >= min_count and the fullest bin not ignored), so the walk reads a byte per row it finds and never a
// histogram; a wave owns kRaycastRaysPerWave consecutive rays and deals them to idle lanes as carve does, the step's lookup is
// the one device function both walks call.  The lane that owns a ray stores its outputs; a hit stores visible[row] = 1.
constexpr int kRaycastRaysPerWave = 128;
constexpr int kMapMaxIgnore = 64;  // SICP_MAP_RAYCAST_MAX_IGNORE
enum { kRaycastRays = 0, kRaycastSteps, kRaycastHits, kRaycastVisible, kRaycastStats = 4 };
struct MapRaycastArgs {
  const float *x, *y, *z;   // [n] the ends, sensor frame (any value: an end that is not finite casts no ray)
  double M[12];
  int n;
  float inv_leaf;
  float sx, sy, sz;         // (float)sensor_origin, transformed in the kernels as a point is
  int ranged;               // max_range > 0
  double range_sq;
  int start_margin;
  long long min_count;
  int n_ignore;
  uint32_t ignore[kMapMaxIgnore];
  MapRows rows;             // hist: nullptr when the map keeps no labels
  int n_map, stride;
  unsigned char* opaque;    // [n_map]
  int* visible;             // [n_map] zeroed: 1 where a ray hits
  int *orow, *ostep, *olength;      // [n] per ray
  float *ox, *oy, *oz;
  uint32_t *olabel, *ocount;
  double* orange_sq;
  unsigned long long* stat; // kRaycastStats words, zeroed
  int* res;                 // res[kMapRange]: the origin lies beyond the key's range (zeroed before the launch)
};
hipError_t launch_map_raycast_opaque(const MapRaycastArgs& a, hipStream_t st);   // opaque, res[kMapRange] (launched for n_map = 0 too)
hipError_t launch_map_raycast_walk(const MapRaycastArgs& a, hipStream_t st);     // the per-ray outputs, visible, stat[rays, steps, hits]
hipError_t launch_map_raycast_visible(const MapRaycastArgs& a, hipStream_t st);  // stat[visible]
// the 2.5-D height grid (sicp_map_elevation; elevation_kernels.hip, driver: elevation.cpp).  One lane per map row writes
// (cell << 21) | (vz + bias) for a row that counts and all ones for one that does not; one stable sort over the cell's and the
// level's bits puts a cell's rows together, its levels ascending and equal levels in ascending map row -- the order in which
// the rule adds a level's sums -- and the rows that do not count behind (the cell field is wide enough that all ones is no
// cell).  Heads, their scan and a gather list the occupied cells with where their rows begin; one lane per occupied cell walks
// its rows, finds the runs and writes the cell; one lane per cell of the window then looks at its eight neighbours and
// classifies it.  A cell's index is a function of the lane id everywhere: nothing is dealt through a counter.
constexpr int kElevMaxLabels = 64;  // SICP_MAP_ELEVATION_MAX_LABELS
constexpr int kElevLevelBits = 21;
// the control words: rows that count, occupied cells, the cells per class
enum { kElevValid = 0, kElevOccupied = 1, kElevClass = 2, kElevCtl = 10 };
inline int elevation_cell_bits(long long cells) {  // the smallest k with 2^k > cells
  int k = 0;
  while ((1ll << k) <= cells) ++k;
  return k;
}
struct MapElevationArgs {
  MapRows rows;                    // hist: nullptr when the map keeps no labels
  int n_map, stride;
  int W, H, B, x0, y0;             // the window (rule 1)
  int lo, hi;                      // the levels seen
  long long min_count;
  int clearance, use_ref, vref, max_extent, min_neighbors;
  double min_clearance, max_step;
  int n_ignore, n_blocked, n_drivable;
  uint32_t ignore[kElevMaxLabels], blocked[kElevMaxLabels], drivable[kElevMaxLabels];
  unsigned long long *key, *skey;  // [n_map]
  int *val, *sval;                 // [n_map] the map row
  int *flag, *pos;                 // [n_map] a cell's first sorted row and its exclusive scan
  int *occ_cell, *occ_begin;       // [min(n_map, W*H)] the occupied cells, ascending, and their first sorted row
  int* ctl;                        // kElevCtl words, zeroed
  uint8_t *state, *neighbors, *cls;  // [W*H] each
  float *elevation, *bottom, *ceiling, *step;
  uint32_t *label, *count;
  int *level_top, *level_bottom, *n_levels;
  const float *px, *py, *pz;       // the slot's finite points in caller order (Cloud::rx ...)
  const int* keep;                 // [n] their caller indices; nullptr when nothing was dropped
  double M[12];
  int n, n_caller;
  float inv_leaf;
  int* point_cell;                 // [n_caller]
  float* point_height;
};
hipError_t launch_elevation_init(const MapElevationArgs& a, hipStream_t st);      // every cell EMPTY; every point -1 / NaN
hipError_t launch_elevation_keys(const MapElevationArgs& a, hipStream_t st);      // key, val
// (prim_sort_pairs key, val -> skey, sval over bits [0, kElevLevelBits + elevation_cell_bits(W * H)))
hipError_t launch_elevation_heads(const MapElevationArgs& a, hipStream_t st);     // flag, ctl[kElevValid]
// (prim_scan_int flag -> pos)
hipError_t launch_elevation_segments(const MapElevationArgs& a, hipStream_t st);  // occ_cell, occ_begin, ctl[kElevOccupied]
hipError_t launch_elevation_cells(const MapElevationArgs& a, hipStream_t st);     // rule 5's arrays of the occupied cells
hipError_t launch_elevation_stencil(const MapElevationArgs& a, hipStream_t st);   // step, neighbors, cls, ctl[kElevClass ..]
hipError_t launch_elevation_points(const MapElevationArgs& a, hipStream_t st);    // point_cell, point_height of the finite points
// the truncated distance field (sicp_map_distance; distance_kernels.hip, driver: distance.cpp).  A cell's state is one packed
// 64-bit key (d^2 << 32) | map row: an obstacle cell is seeded with (0, row), every other cell with kDistNone, whose d^2 field
// is above every reachable sum and survives three additions of up to 64^2.  A sweep along an axis replaces a cell's key by the
// minimum over s in -R..R of key[cell + s along the axis] + (s^2 << 32), cells outside the window taking no part; an addition
// to the high field keeps the order of the packed keys, so after the sweeps along x, y and z the key is the lexicographic
// minimum of (d^2, row) over the cube, and the test d^2 <= R^2 makes it the ball's.  Integer arithmetic, plain stores (one
// 64-bit atomicMin per row when seeding a column in planar mode): the bytes do not depend on the launch shape.
constexpr int kDistMaxLabels = 64;  // SICP_MAP_DISTANCE_MAX_LABELS
constexpr int kDistMaxR = 64;
constexpr unsigned long long kDistNone = (0x40000000ull << 32) | 0xffffffffull;
// the control words: obstacle cells, reached cells, the largest d^2 + 1 (0: none), points inside the window
enum { kDistObstacles = 0, kDistReached = 1, kDistMaxPlus1 = 2, kDistInside = 3, kDistCtl = 4 };
constexpr int kDistLineTile = 256;  // the x sweep: cells of a line per workgroup, R of halo on either side in LDS
constexpr int kDistTileX = 32;      // the y and z sweeps: a workgroup's tile is kDistTileX lanes along x (256 contiguous bytes a
constexpr int kDistTileA = 64;      // row) by kDistTileA cells along the axis plus 2 R of halo: (64 + 2 R) * 256 bytes of LDS,
                                    // 48 KiB at R = 64 (three workgroups a CU), 21 KiB at R = 10
struct MapDistanceArgs {
  MapRows rows;                    // hist: nullptr when the map keeps no labels
  int n_map, stride;
  int nx, ny, nz, x0, y0, z0;      // the window (rule 1)
  int planar, lo, hi;              // rule 3's band
  int R;
  long long min_count;
  int n_ignore, n_only;
  uint32_t ignore[kDistMaxLabels], only[kDistMaxLabels];
  unsigned long long* key;         // [cells] the buffer the seeds go to
  uint32_t* row_label;             // [n_map] the fullest bin of the obstacle rows (nullptr without labels)
  int* ctl;                        // kDistCtl words, zeroed
  int *dist_sq, *nearest;          // [cells]
  uint32_t* label;
  const float *px, *py, *pz;       // the slot's finite points in caller order (Cloud::rx ...)
  const int* keep;                 // [n] their caller indices; nullptr when nothing was dropped
  double M[12];
  int n, n_caller;
  float inv_leaf;
  int *point_cell, *point_dist_sq, *point_nearest;  // [n_caller]
  float* point_range_sq;
};
hipError_t launch_distance_init(const MapDistanceArgs& a, hipStream_t st);    // every key kDistNone; every point -1 / NaN
hipError_t launch_distance_seed(const MapDistanceArgs& a, hipStream_t st);    // the obstacle cells' keys, row_label, ctl[kDistObstacles]
// one sweep, src -> dst: axis 0 along x, 1 along y, 2 along z
hipError_t launch_distance_sweep(const MapDistanceArgs& a, int axis, const unsigned long long* src, unsigned long long* dst, hipStream_t st);
hipError_t launch_distance_final(const MapDistanceArgs& a, const unsigned long long* src, hipStream_t st);  // dist_sq, nearest, label, ctl
hipError_t launch_distance_points(const MapDistanceArgs& a, hipStream_t st);  // the point arrays of the finite points, ctl[kDistInside]
// label fusion through the confusion matrix (sicp_map_extract_fused, sicp_map_fused_labels).  logcm[r * C + s] = log cm[r][s]
// (observed label r + 1, class s + 1; -inf for a zero entry).  A histogram row's score of class s is the sum over its
// non-zero bins r = 1..C, ascending, of (double)h[r] * logcm[r - 1][s - 1], each product and each sum rounded once.  An item
// (a voxel, a point) is scored by map_fuse_width(C) neighbouring lanes of a wave, lane j of them owning the classes j + 1,
// j + 1 + 64, ...: it walks the row's non-zero bins, never C^2 products.  Up to kMapFuseLdsClasses classes every workgroup
// stages logcm in LDS (8 * 64 * 64 bytes = 32 KiB); above, it reads it from global memory.  The same arithmetic either way.
constexpr int kMapFuseLdsClasses = 64;
inline int map_fuse_width(int C) {  // lanes per item: the power of two >= C in 4..64
  int w = 4;
  while (w < C && w < 64) w <<= 1;
  return w;
}
struct MapFuseArgs {
  const double* logcm;      // [C][C]
  int C, stride;            // stride = C + 1
  MapRows rows;
  int n_map;
  // extract: the selected rows (src_of[j] for j < res[kMapOut], written by launch_map_extract on the same stream)
  const int* src_of;
  const int* res_in;
  // relabel: the scan's finite points in caller order, their labels (nullptr: none), the pose
  const float *x, *y, *z;
  const uint32_t* label;
  double M[12];
  int n, include_own;
  long long min_count;
  float inv_leaf;
  int* res;                 // relabel: res[kMapBadLabel] (zeroed before the launch)
  uint32_t* olabel;         // [items] the fused label; without evidence 0 (extract) / the point's own label (relabel)
  double* oconf;            // [items] its posterior probability; 0 without evidence
};
hipError_t launch_map_posterior(const MapFuseArgs& a, hipStream_t st);  // olabel, oconf of the selected rows
hipError_t launch_map_relabel(const MapFuseArgs& a, hipStream_t st);    // olabel, oconf of the n points; res[kMapBadLabel]
// one map into another at a pose (sicp_map_merge; map_merge_kernels.hip).  SRC's rows are the items: one lane per row moves its
// sums by the pose in double, keys the float centroid of the moved sums on DST's grid, and the (key, row) pairs are sorted -- a
// stable sort, so rows ascend inside a run of equal keys.  The runs' heads are a sorted list of distinct keys, which is what
// integrate's rank merge takes (launch_map_lookup / _misses / _scatter / _move_hist, through a MapFoldArgs).  Then one lane per
// touched dst row continues its sums with the run's moved sums in ascending src row, and a second launch, parallel over
// (touched row, bin), adds the run's histogram rows: consecutive lanes read consecutive bins of one src row.
struct MapMergeArgs {
  int n;                    // src rows
  int n_map, n_new;         // dst rows before the call; rows it opens (known after the first read-back)
  int n_runs, n_kept;       // touched dst rows; kept src rows (the sorted pairs before the dropped ones): after the read-back
  int stride;               // dst's num_classes + 1 (= src's); 0: dst keeps no labels and src's histograms are not read
  int crop;
  long long min_count;
  double M[12];
  float inv_leaf, cx, cy, cz;  // dst's 1.0f / (float)leaf_size; (float)crop_center
  double range_sq;
  MapRows src;
  double *mx, *my, *mz;     // [n] the moved sums by src row (written for every row with min_count points)
  unsigned long long* key;  // [n] the dst key of src row r, ~0 for a row that takes no part
  int* val;                 // [n] r
  const unsigned long long* skey;  // the pairs sorted
  const int* sval;
  const int *flag, *pos;    // launch_merge_heads' flags and their exclusive scan
  int* heads;               // [n] first sorted position of every run
  const int *rank, *mpos;   // launch_map_lookup's and the scan of its misses: run k's dst row is rank[k] + mpos[k]
  unsigned long long* kept_points;  // the sum of the kept rows' counts (zeroed before the launch)
  int* res;                 // kMapRes words, zeroed: kMapRange (keys), kMapKept / kMapScanVoxels (runs), kMapMaxCount (sums: the longest run)
  MapRows to;               // dst's spare set, after launch_map_scatter
};
hipError_t launch_map_merge_keys(const MapMergeArgs& a, hipStream_t st);       // mx my mz, key, val, kept_points, res[kMapRange]
hipError_t launch_map_merge_runs(const MapMergeArgs& a, hipStream_t st);       // heads, res[kMapKept, kMapScanVoxels]
hipError_t launch_map_merge_fold_sums(const MapMergeArgs& a, hipStream_t st);  // to.{sums, cnt} of the touched rows, res[kMapMaxCount]
hipError_t launch_map_merge_fold_hist(const MapMergeArgs& a, hipStream_t st);  // to.hist of the touched rows

// ---- initial alignment without a pose prior (bootstrap_kernels.hip; driver: bootstrap.cpp) ----
constexpr int kBootMaxK = 16;  // feature neighbours per source keypoint (k_correspondences)
int boot_bounds_blocks(int n);
// the label forms (sicp_bootstrap_semantic): a point whose label is in the ignore list is dropped with the box filter
constexpr int kBootMaxIgnore = 64;
struct BootIgnore {  // a kernel argument: n <= kBootMaxIgnore labels
  int n;
  unsigned v[kBootMaxIgnore];
};
// Both take the label form as arguments: ig == nullptr launches the label-blind kernel (label is not read), otherwise the
// kernel that also drops the points whose label[i] is in *ig.
// per workgroup of 256 points: min xyz, max xyz and count of the box-filtered points -> blk[block * 8 + 0..6]
hipError_t launch_boot_bounds(int n, const float* x, const float* y, const float* z, const unsigned* label, const BootIgnore* ig,
                              double box_max, float* blk, hipStream_t st);
// key[i] = voxel index << 32 | i for a kept point, ~0 otherwise
hipError_t launch_boot_voxel_keys(int n, const float* x, const float* y, const float* z, const unsigned* label, const BootIgnore* ig,
                                  double box_max, float inv_leaf, const int* min_b, int dx, int dxy, unsigned long long* key,
                                  hipStream_t st);
// klabel[k] = the most frequent label among voxel k's points (its range of the sorted keys), ties to the smallest label
hipError_t launch_boot_label_vote(int n_kp, int n_kept, const int* heads, const unsigned long long* key, const unsigned* label,
                                  unsigned* klabel, hipStream_t st);
// sorted voxel keys -> first entry of every voxel (heads[n_out]) and the keypoint count *n_out (temp: prim_scan_int's)
hipError_t launch_boot_voxel_compact(int n_kept, const unsigned long long* key, int* flag, int* pos, int* heads, int* n_out,
                                     void* temp, size_t temp_bytes, hipStream_t st);
hipError_t launch_boot_centroids(int n_kp, int n_kept, const int* heads, const unsigned long long* key, const float* x,
                                 const float* y, const float* z, float* kx, float* ky, float* kz, hipStream_t st);
// Job forms (job_table.hpp; one launch over every cloud or pair of a bootstrap batch).  A workgroup is the unit of the
// launch: 256 items for radius / normals / k-NN, one keypoint for SPFH / FPFH, one hypothesis for the error.
// Per item every kernel runs what the lone launch ran, in the same order: a batch gives every job the bits of a batch of one.
struct BootCloudJob {
  int m, pad_;                  // keypoints
  const float *x, *y, *z;       // keypoints (device)
  // radius lists under construction: the cell grid, its sorted keys / point ids, and the counts (fill 0) or lists (fill 1)
  float inv_cell, r2;
  const unsigned long long* skey;
  const int* sval;
  long long* count;
  const long long* loff;
  unsigned long long* list;
  // the finished lists: normal radius (noff / nidx: normals) and feature radius (off / idx / d2: SPFH, FPFH)
  const long long* noff;
  const int* nidx;
  const long long* off;
  const int* idx;
  const float* d2;
  double* n3;    // [m][3]
  double* spfh;  // [m][33] scratch
  float* fpfh;   // [m][33]
};
struct BootPairJob {
  int n;   // feature k-NN: source keypoints;  error: hypotheses of the pair in this launch
  int nt;  // feature k-NN: target keypoints;  error: squared distances per hypothesis (source keypoints)
  const float *sf, *tf;  // k-NN: features [n][33], [nt][33]
  int* out;              // k-NN: [n][k]
  const float* d2;       // error: [n][nt]
  double* err;           // error: [n]
  // the label forms only (keypoint labels):
  const unsigned *sl, *tl;  // k-NN: of the source / target keypoints, keypoint order;  error: in the order of the search's
                            // rows (sl: the source tree's device order) and of its neighbour indices (tl: the target tree's)
  const int* nbr;           // error: [n][nt] the search's neighbour index of every squared distance (-1: none)
};
// radius neighbourhoods on a uniform grid: cell keys + point ids (to be sorted by key), then count (fill = 0: count[i]) or
// write the unsorted lists of (d^2 bits << 32 | index) at loff[i] (fill = 1); split: sorted lists -> index / d^2 arrays
hipError_t launch_boot_cell_keys(int m, const float* x, const float* y, const float* z, float inv_cell, unsigned long long* key,
                                 int* val, hipStream_t st);
hipError_t launch_boot_radius_jobs(int fill, const BootCloudJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st);
hipError_t launch_boot_split(long long total, const unsigned long long* list, int* idx, float* d2, hipStream_t st);
hipError_t launch_boot_normal_jobs(const BootCloudJob* jobs, const int* blk_end, int nj, int blocks, hipStream_t st);
// SPFH (into spfh) then FPFH; pt_end: prefix of the keypoint counts, points = all keypoints of the launch
hipError_t launch_boot_fpfh_jobs(const BootCloudJob* jobs, const int* pt_end, int nj, int points, hipStream_t st);
// out[n][k]: the k nearest target features of every source feature (-1: none / no feature); same_label: among the target
// keypoints with the source keypoint's label (sl / tl)
hipError_t launch_boot_feature_knn_jobs(const BootPairJob* jobs, const int* blk_end, int nj, int blocks, int k, bool same_label,
                                        hipStream_t st);
// err[h] = sum over the nt squared distances d2[h][.] of (e <= t ? e / t : 1); hyp_end: prefix of the hypothesis counts;
// same_label: a distance counts as e / t only when the neighbour found has the source keypoint's label (sl / tl / nbr)
hipError_t launch_boot_error_jobs(const BootPairJob* jobs, const int* hyp_end, int nj, int hypotheses, double t, bool same_label,
                                  hipStream_t st);

// ---- scan descriptors and the loop-candidate search (place_kernels.hip; driver: place.cpp) ----
// sicp_place_*: a scan -> R x S cell codes (one pass of integer atomics into a zeroed table, a finalise pass), and the exact
// search of query descriptors against the stored ones at every sector shift.  Integers only behind the cell arithmetic of
// include/sicp.h, rules 3 and 4.
constexpr int kPlaceMaxRings = 64, kPlaceMaxSectors = 256;
enum { kPlaceKept = 0, kPlaceBadLabel = 1, kPlaceCells = 2, kPlaceRes = 4 };
struct PlaceDescribeArgs {
  const float *x, *y, *z;   // the scan's finite points (Cloud::rx ...)
  const uint32_t* label;    // nullptr for the height channel
  int n, R, S, C;           // C: num_classes (label channel), 0 for the height channel
  float ox, oy, oz;         // (float)sensor_origin
  double min_range_sq, z_min, inv_z_step;
  const double* tables;     // edge2[R + 1] | cos_half[S / 2] | sin_half[S / 2]
  uint32_t ignore[8];       // bit l: label l takes no part
  int min_cell_points;
  uint32_t* table;          // label: [R*S][C] counts of labels 1..C; height: [R*S][2] count, largest level.  Zeroed before
  uint8_t* desc;            // [R*S]
  unsigned long long* res;  // kPlaceRes words, zeroed before
};
hipError_t launch_place_cells(const PlaceDescribeArgs& a, hipStream_t st);     // table, res[kept, bad label]
hipError_t launch_place_finalise(const PlaceDescribeArgs& a, hipStream_t st);  // desc, res[cells]
struct PlaceSearchArgs {
  const uint8_t* query;     // [n_q][R*S]
  const uint8_t* entries;   // [count][R*S]: the searched range's first entry
  int n_q, count, R, S;
  unsigned long long* key;  // [n_q][count]: (2^30 - floor(match * 2^30 / either)) << 31 | entry index in the range
  unsigned long long* hit;  // [n_q][count]: shift | match << 16 | either << 32 of the entry's best shift
};
hipError_t launch_place_search(const PlaceSearchArgs& a, hipStream_t st);
// rows[q][k] = {entry index in the range, shift, match, either} of the k-th sorted key of query q, k < top
hipError_t launch_place_gather(const unsigned long long* sorted_key, const unsigned long long* hit, int n_q, int count, int top, int4* rows,
                               hipStream_t st);

// ---- the pose graph (graph_kernels.hip; driver: graph.cpp; the edge's algebra: graph_edge.hpp) ----
// sicp_graph_*: linearise every edge, gather per node through the incidence table, preconditioned conjugate gradients on the
// damped normal equations, candidate poses.  No float atomics: every sum has one order (per node its enabled edge records in
// ascending (edge, side), then its enabled prior records in ascending prior id; per-workgroup partial sums of 256 lanes added by
// one workgroup in index order).  A disabled edge is left out of the incidence lists, a disabled prior out of the prior lists,
// and either counts as +0.0 at its place in the cost's sum (ec: the edges in id order, then the priors in id order).  The scalars of the iteration stay in
// GraphScalars on the device: the kernels read the previous step's from memory and return at once when `flag` is set.
constexpr int kGraphRec = 42;        // a (edge, side) contribution: the 6x6 diagonal block, then the gradient
constexpr int kGraphChol = 27;       // a node's preconditioner: the 21 entries of L (row-major lower), then 1 / L_kk
constexpr int kGraphLinLanes = 64;   // lanes of a linearise workgroup (one edge each: the register budget of a whole SIMD)
enum { kGraphRunning = 0, kGraphConverged = 1, kGraphBreakdown = 2 };
struct GraphScalars {
  double rz, pq, alpha, beta, rr, bb;   // conjugate gradients: r.z, p.Ap, the two step scalars, |r|^2, |b|^2
  double cost, cand_cost, gmax;         // 1/2 sum rho at the poses / at the candidates; max |g|
  double pose2, xx, gx, xHx;            // |poses|^2, |delta|^2, g.delta, delta^T H delta
  int cg_iters, flag;                   // kGraph*
};
struct GraphArgs {
  int n_nodes, n_edges, n_priors;
  const double* pose;          // [n_nodes][7]
  const uint8_t* fixed;        // [n_nodes]
  const int *ei, *ej;          // [n_edges]
  const double *z, *omega;     // [n_edges][7], [n_edges][36]
  const uint8_t* een;          // [n_edges] enabled flags; NULL: every edge is enabled
  // priors (graph_prior.hpp): a POSITION prior uses the first 3 of its z and the first 9 of its omega
  const int *pnode, *pkind;    // [n_priors]
  const uint8_t* pen;          // [n_priors] enabled flags
  const double *pz, *pomega;   // [n_priors][7], [n_priors][36]
  int loss;
  double cauchy_a;
  // per edge
  double *C, *B, *r, *s, *w, *ec;   // [2 n_edges][kGraphRec], [n_edges][36], [n_edges][6], [n_edges] x 2, ec [n_edges + n_priors]: 1/2 rho
  // per prior; its 1/2 rho is ec[n_edges + prior]
  double *PC, *pr, *ps, *pw;        // [n_priors][kGraphRec], [n_priors][6], [n_priors] x 2
  // incidence: the slots 2 * edge + side of the enabled edges sorted by node (low 32 bits of inc; the disabled ones follow
  // under the key n_nodes), off[n_nodes + 1]; the enabled priors sorted by node in pinc, poff[n_nodes + 1] (n_priors > 0 only)
  unsigned long long* inc;
  int *deg, *off;
  const int *pinc, *poff;
  // per node
  double *H, *g, *L;           // [n_nodes][36], [n_nodes][6], [n_nodes][kGraphChol]
  double *x, *rr, *zz, *p, *q; // [n_nodes][6]: the step, the residual, M^-1 r, the direction, A p
  double* cand;                // [n_nodes][7]
  double* part;                // [3][part_stride] partial sums
  int part_stride;
  GraphScalars* S;
  double lo, hi, radius, eta;  // D = clip(diag H, lo, hi) / radius
};
enum { kGraphFinStart, kGraphFinPq, kGraphFinRz, kGraphFinCost, kGraphFinCandCost, kGraphFinGmax, kGraphFinCand, kGraphFinModel };
hipError_t launch_graph_keys(const GraphArgs& a, unsigned long long* keys, hipStream_t st);  // keys[2 n_edges], deg (zeroed before)
hipError_t launch_graph_linearise(const GraphArgs& a, const double* pose, bool full, hipStream_t st);  // ec (+ r s w C B when full)
hipError_t launch_graph_prior_linearise(const GraphArgs& a, const double* pose, bool full, hipStream_t st);  // ec (+ pr ps pw PC when full)
hipError_t launch_graph_gather(const GraphArgs& a, hipStream_t st);                          // H, g
hipError_t launch_graph_sum(const GraphArgs& a, int fin, hipStream_t st);                    // ec -> S->cost / cand_cost; g -> S->gmax
hipError_t launch_graph_cg_begin(const GraphArgs& a, hipStream_t st);                        // L, x = 0, r = -g, z, p, S->rz bb rr
hipError_t launch_graph_cg_iteration(const GraphArgs& a, hipStream_t st);                    // one step of x, r, z, p
hipError_t launch_graph_candidates(const GraphArgs& a, hipStream_t st);                      // cand, S->pose2 xx gx xHx
inline int graph_blocks(long long items) { return (int)((items + 255) / 256); }

// ---- blocks of H^-1 (graph_cov_kernels.hip; driver: graph.cpp; the relative pose's Jacobian: graph_cov.hpp) ----
// sicp_graph_marginals / sicp_graph_relative_covariances: H X = J^T for `cols` right-hand sides at once (six per query) by
// conjugate gradients in lock step, on the undamped H of the last linearisation with the block-Jacobi preconditioner.  Every
// vector is [n_nodes][cols][6]: the six lanes of a node and consecutive columns read contiguous memory.  Each column has its own
// scalars and its own flag; a column whose flag is set is frozen (x, r, p are no longer written), and no column's arithmetic
// depends on another's or on how many there are: a query's bytes are the same alone, in any company and at any `cols`.
// Partial sums go per (column, workgroup) -- the SpMM's workgroup is 256 (node, row) lanes, the others' 64 nodes, whatever
// `cols` -- and one workgroup per column adds them in graph_finish_kernel's order.
constexpr int kGraphCovNodes = 64;   // nodes of a workgroup of the begin and update kernels
enum { kGraphCovRunning = 0, kGraphCovConverged = 1, kGraphCovBreakdown = 2, kGraphCovLimit = 3 };
struct GraphCovColumn {
  double rz, pq, alpha, beta, rr, bb;   // as GraphScalars
  int iters, flag;                      // kGraphCov*
};
struct GraphCovArgs {
  int n_nodes, cols;           // cols = 6 * (queries of this pass)
  const double* pose;          // [n_nodes][7]
  const uint8_t* fixed;
  const int *ei, *ej;
  const double* B;             // [n_edges][36]
  const unsigned long long* inc;
  const int* off;
  const uint8_t* held;         // [n_nodes]: the node has an enabled pose prior; NULL: the graph has no priors
  const double* H;             // [n_nodes][36], undamped
  double* L;                   // [n_nodes][kGraphChol]: the factor of H's blocks (identity for a free node without enabled edges
                               // or pose prior)
  const int *qa, *qb;          // [cols / 6]: the query's nodes (qa = -1: a marginal); a fixed end has no block
  double* J;                   // [cols / 6][36]: J_a
  double *x, *r, *z, *p, *q;   // [n_nodes][cols][6]
  double* part;                // [2][cols][part_stride]
  int part_stride;
  GraphCovColumn* S;           // [cols]
  int* bad;                    // set when a diagonal block is not positive definite
  double tolerance;
  int max_iters;
  double* out;                 // [cols / 6][36]
};
inline int graph_cov_node_blocks(long long n_nodes) { return (int)((n_nodes + kGraphCovNodes - 1) / kGraphCovNodes); }
inline int graph_cov_spmm_cols(int cols) { return cols % 24 == 0 ? 24 : cols % 12 == 0 ? 12 : 6; }  // the instantiation a pass runs
hipError_t launch_graph_cov_factor(const GraphCovArgs& a, hipStream_t st);     // L, *bad
hipError_t launch_graph_cov_begin(const GraphCovArgs& a, hipStream_t st);      // J, x = 0, r = b, z, p, S
hipError_t launch_graph_cov_iteration(const GraphCovArgs& a, hipStream_t st);  // one step of every running column
hipError_t launch_graph_cov_extract(const GraphCovArgs& a, hipStream_t st);    // out = sym(J X)

// ---- the sorts and scans of the feature calls (prim_kernels.hip: the only rocPRIM instantiations besides build_tree.hip) ----
// rocPRIM's convention: temp == nullptr asks for the bytes.  Ascending, stable; keys: bits [begin_bit, end_bit).
hipError_t prim_sort_keys(void* temp, size_t& bytes, const unsigned long long* in, unsigned long long* out, long long n, int begin_bit,
                          int end_bit, hipStream_t st);
hipError_t prim_sort_pairs(void* temp, size_t& bytes, const unsigned long long* kin, unsigned long long* kout, const int* vin, int* vout,
                           long long n, int begin_bit, int end_bit, hipStream_t st);
// exclusive sums
hipError_t prim_scan_int(void* temp, size_t& bytes, const int* in, int* out, long long n, hipStream_t st);
hipError_t prim_scan_ll(void* temp, size_t& bytes, const long long* in, long long* out, long long n, hipStream_t st);
// all 64 bits of the keys of every segment [off[s], off[s + 1]) on its own
hipError_t prim_segmented_sort_keys(void* temp, size_t& bytes, const unsigned long long* in, unsigned long long* out, long long n,
                                    int segments, const long long* off, hipStream_t st);

}  // namespace sicp
#endif
