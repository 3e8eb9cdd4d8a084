/*
 * sicp.h -- C ABI of the MI355X-native semantic-ICP registration engine.
 *
 * This is the drop-in boundary for the hot path of kxhit/semantic-icp: the body
 * of align() in the reference's three header-only registration classes.  The
 * reference has no FFI of its own (it is header-only C++ that the drivers
 * instantiate directly), so every entry point below cites the reference
 * member(s) it replaces; the C++ class shims in semantic-icp_amd/host/ keep the
 * reference's class/method names on top of this ABI.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, opaque handle, int status
 *     (0 = ok, negative = error).  No exception crosses the ABI: every entry
 *     point and the stream worker thread run inside a barrier that turns
 *     std::bad_alloc into SICP_ERR_OUT_OF_MEMORY and anything else into
 *     SICP_ERR_INTERNAL (csrc/abi_barrier.hpp).  The library never prints --
 *     unless the developer sets SICP_DEBUG in the environment, which unlocks
 *     the stderr logs of SICP_KNN_STATS / SICP_SOLO_LOG / SICP_STREAM_LOG.
 *   - The caller owns every input/output buffer (host memory unless a name
 *     ends in _device); the handle owns all device memory.
 *   - One handle = one HIP device + one stream.  Handles are independent and
 *     may be driven from different host threads or processes (that is how
 *     scan pairs shard across the 8 GPUs of a node); a single handle is not
 *     thread-safe, like the reference classes.
 *   - Pose exchange format: Sophus storage order qt[7] = [qx qy qz qw tx ty tz]
 *     (reference: gicp_cost_function.h:64-70).  Tangent order [upsilon; omega].
 *   - Clouds are SoA float32 xyz (+ uint32 labels): the layout the kernels read.
 *     Labels are 1..C for SICP_MODE_EM (reference quirk: em_icp.hpp:301 indexes
 *     label-1), arbitrary for SICP_MODE_SEMANTIC, ignored for SICP_MODE_GICP.
 */
#ifndef SICP_H_
#define SICP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SICP_VERSION_MAJOR 0
#define SICP_VERSION_MINOR 6
#define SICP_MAX_K_COV 32  /* largest covariance neighbourhood (ctor argument k) */

/* ---- status codes ------------------------------------------------------- */
enum {
  SICP_OK = 0,
  SICP_ERR_INVALID_ARGUMENT = -1,
  SICP_ERR_NO_DEVICE = -2,       /* no HIP device / HIP runtime failure at create */
  SICP_ERR_HIP = -3,             /* a HIP call failed; see sicp_last_error()       */
  SICP_ERR_NOT_READY = -4,       /* clouds / confusion matrix missing for the mode */
  SICP_ERR_TOO_FEW_POINTS = -5,  /* target has fewer than K points (reference: UB,
                                    em_icp.hpp:62-65)                             */
  SICP_ERR_BAD_LABEL = -6,       /* EM label outside 1..C (reference: UB)          */
  SICP_ERR_OUT_OF_MEMORY = -7,   /* host (std::bad_alloc) or device (hipErrorOutOfMemory, or the
                                    limit of sicp_set_memory_limit) memory exhausted     */
  SICP_ERR_INTERNAL = -8         /* a C++ exception was caught at the ABI boundary; see
                                    sicp_last_error() / sicp_stream_last_error()        */
};

/* ---- which reference class the handle behaves as ------------------------ */
enum {
  SICP_MODE_GICP = 0,     /* semanticicp::GICP<PointT>             gicp.h:15-132        */
  SICP_MODE_EM = 1,       /* EmIterativeClosestPoint<N>            em_icp.h:17-122      */
  SICP_MODE_SEMANTIC = 2  /* SemanticIterativeClosestPoint<P,S>    semantic_icp.h:15-83 */
};

enum { SICP_SOURCE = 0, SICP_TARGET = 1 };

/* sicp_params.profile bits.  Each timed kernel adds one event synchronisation. */
enum {
  SICP_PROFILE_NN = 1,      /* correspondence search (nn_partial kernel)          */
  SICP_PROFILE_COV = 2,     /* covariance self-kNN (nn_partial<20> kernel)        */
  SICP_PROFILE_WEIGHT = 4,  /* EM weight kernel                                   */
  SICP_PROFILE_ACC = 8      /* accumulate + finalize kernels, per LM evaluation   */
};

typedef struct sicp_context* sicp_handle;

/* Tunables.  The reference hard-codes most of these as literals; defaults
 * (sicp_default_params) reproduce them exactly. */
typedef struct sicp_params {
  int32_t mode;            /* SICP_MODE_*                                              */
  int32_t knn;             /* correspondences per source point: 4 (em_icp.hpp:60) or 1  */
  int32_t k_cov;           /* covariance neighbourhood (ctor arg k = 20, em_icp.h:42):
                              any 1..SICP_MAX_K_COV                                      */
  int32_t num_classes;     /* runtime C, replaces template parameter N (em_icp.h:16)    */
  double epsilon;          /* ctor arg epsilon = 1e-3 (em_icp.h:43)                     */
  double gate_sq;          /* 250, strict < (em_icp.hpp:65)                             */
  double cauchy_a;         /* 3.0 (em_icp.hpp:111) / 1.5 (semantic_icp.hpp:96)          */
  int32_t use_sqloss;      /* ComposedLoss(.., SQLoss): 1 EM/GICP, 0 Semantic            */
  int32_t max_outer;       /* 50 (em_icp.hpp:180) / 35 (semantic_icp.hpp:152)            */
  double outer_tol;        /* 1e-5 / 1e-3 on ||log(T_cur^-1 T_est)||^2                   */
  int32_t min_class_pts;   /* 400, strict > (semantic_icp.hpp:51)                        */
  int32_t max_lm_iterations;      /* 400 (em_icp.hpp:169)                                */
  double gradient_tolerance;      /* 1e-11 (em_icp.hpp:163)                              */
  double function_tolerance;      /* 1e-11 (em_icp.hpp:164)                              */
  /* Ceres defaults the reference leaves untouched (Ceres 1.14..2.1 solver.h) */
  double parameter_tolerance;     /* 1e-8  */
  double initial_radius;          /* 1e4   */
  double max_radius;              /* 1e16  */
  double min_radius;              /* 1e-32 */
  double min_relative_decrease;   /* 1e-3  */
  double min_lm_diagonal;         /* 1e-6  */
  double max_lm_diagonal;         /* 1e32  */
  int32_t max_consecutive_invalid_steps; /* 5 */
  int32_t jacobi_scaling;         /* 1 */
  /* Reference quirks, reproduced by default (SURVEY.md 8a "Quirks") */
  int32_t quirk_bool_probability; /* Q1: GICPCostFunction::Probability returns bool
                                     (gicp_cost_function.h:75); 0 = use the double   */
  int32_t quirk_float_products;   /* Q2: float32 products in the covariance moments
                                     (em_icp.hpp:307-314); 0 = double products       */
  /* engine knobs (no reference counterpart) */
  int32_t nn_method;              /* 0 = LDS-tiled brute force, 1 = Hilbert box-tree, the
                                     16 queries of a wave walk it together (default),
                                     2 = box-tree, every query walks alone; all exact,
                                     bit-identical results                              */
  int32_t profile;                /* SICP_PROFILE_* bit mask: bracket those kernels with
                                     HIP events on the handle's stream (sicp_stats)     */
  int32_t lm_on_device;           /* 0 = host loop (one synchronisation per evaluation);
                                     1 (default; 3 is an alias) = trust-region state lives on
                                     the GPU: ticks of [accumulate kernel, LM-step kernel] x
                                     lm_batch as one graph launch, the host polls once per tick;
                                     the ONLY pair still iterating -- sicp_align, or the tail of
                                     a batch / stream -- continues its solve as persistent
                                     launches (its chunks stay in registers, one workgroup per
                                     chunk + one that steps the solver) when they
                                     fit the chip, falling back to the ticks if that grid cannot
                                     become resident;
                                     2 = as 1 without the persistent launches.
                                     Same machine (csrc/lm.hpp), same iterates, same bits.  */
  int32_t lm_batch;               /* evaluations queued per host poll (lm_on_device)    */
  int32_t reuse_features;         /* 0 (default) = recompute normals / histograms on every
                                     align() like em_icp.hpp:28-29 and gicp.hpp:33-34 do;
                                     1 = keep them while the uploaded cloud, k and C are
                                     unchanged (same values: they only depend on the cloud),
                                     what setSourceCloud(cloud, kdtree, covs) gicp.h:48-56
                                     exists for                                          */
  int32_t reserved_;
} sicp_params;

/* Per-align() counters; times in milliseconds.  *_kernel_ms are HIP-event
 * times on the handle's stream and are only filled when params.profile = 1. */
typedef struct sicp_stats {
  int32_t outer_iters;      /* what getOuterIter() returns (em_icp.h:88-91)          */
  int32_t total_lm_iters;
  int32_t total_evals;      /* accumulate passes ("E" of SURVEY.md 8d), all outer    */
  int32_t weights_in_search; /* correspondence searches of this align() that wrote the EM weights themselves
                               (a handle alone, streams, most batches): these have no weight launch of their own,
                               so weight_launches + weights_in_search = searches with weights            */
  int64_t total_corr;       /* sum over outer passes of N_s*K candidate slots        */
  int64_t total_active;     /* slots that passed the distance gate                   */
  double final_cost;
  double t_cov_ms, t_nn_ms, t_weight_ms, t_solve_ms, t_total_ms;  /* host wall clock */
  double cov_kernel_ms;     /* nn_partial<k_cov> (self-kNN) launches                 */
  double nn_kernel_ms;      /* nn_partial<K> (correspondence search) launches        */
  double weight_kernel_ms;  /* EM weight kernel launches                             */
  double acc_kernel_ms;     /* accumulate + finalize pairs                           */
  int32_t cov_launches, nn_launches, weight_launches, acc_launches; /* timed launches */
  /* LM evaluation launches this pair was part of (ticks of lm_batch evaluations, one graph launch
   * each, shared by all pairs of a sicp_align_batch), including the tail of a tick it sat through
   * after its own inner solve had finished: idle slots = lockstep_slots - total_evals */
  int32_t lockstep_slots;
  int32_t graph_builds;     /* hipGraph instantiations during this align (leader handle of a batch) */
} sicp_stats;

/* ---- lifetime ------------------------------------------------------------- */
int sicp_device_count(int* count);
/* replaces the three class constructors (em_icp.h:42-48, gicp.h:34-40,
 * semantic_icp.h:35-39); mode and tunables follow via sicp_set_params */
int sicp_create(int device_id, sicp_handle* out);
/* Ends the caller's use of `h`: everything it queued is waited for and its clouds are let go.  The handle itself is
 * PARKED, not freed: up to 32 per device stay in a pool with their streams, events, pinned mirrors, device buffers and
 * tick graphs (a batch leader or a stream's slot holds tens of MB), and the next sicp_create on that device hands one
 * out again, reset to what a new handle is.  Only sicp_release_pool gives a parked handle's memory back.
 * A second sicp_destroy of a handle that is still parked returns SICP_ERR_INVALID_ARGUMENT and changes nothing.  The
 * check can only work while the handle is parked: once sicp_create has handed it out again it is another caller's live
 * handle, and once sicp_release_pool has freed it the pointer dangles -- as after any free. */
int sicp_destroy(sicp_handle h);
/* Uploaded clouds (device buffers, search structures, pinned staging memory) are recycled through a
 * per-device pool when their last handle lets go of them, and all device buffers are carved from a
 * per-device arena that is not returned to the driver by itself; this frees what the pool of
 * `device_id` currently holds -- the recycled clouds and the handles parked by sicp_destroy, with all they retain --
 * and every arena slab no live buffer sits in (it waits for the device first).  Never required. */
int sicp_release_pool(int device_id);
/* Device memory the library may hold on `device_id`, in bytes (0 = no limit, the default): the arena takes no new
 * slab from the driver beyond it, and whatever then cannot be allocated -- a cloud, a handle's buffers -- fails with
 * SICP_ERR_OUT_OF_MEMORY (a status, like every other failure; the handle / stream stays usable for smaller work).
 * Memory already held is not given back by lowering the limit (sicp_release_pool does that).  For a process that
 * shares its GPU.  sicp_memory_reserved: what the arena holds right now. */
int sicp_set_memory_limit(int device_id, int64_t bytes);
int sicp_memory_reserved(int device_id, int64_t* bytes);
const char* sicp_strerror(int status);
const char* sicp_last_error(sicp_handle h); /* detail of the last SICP_ERR_HIP */
const char* sicp_version(void);

/* ---- configuration --------------------------------------------------------- */
int sicp_default_params(int mode, sicp_params* p);
/* Besides mode, knn, k_cov, epsilon, cauchy_a and nn_method, the trust-region options are checked, because their loop
 * runs inside kernels: SICP_ERR_INVALID_ARGUMENT, the field named in sicp_last_error and the handle's parameters left as
 * they were, unless the nine option doubles and outer_tol are finite, gradient_ / function_ / parameter_tolerance >= 0,
 * 0 <= min_radius <= initial_radius <= max_radius with initial_radius > 0 (denormal radii are legal),
 * 0 <= min_relative_decrease < 1, 0 <= min_lm_diagonal <= max_lm_diagonal, max_lm_iterations >= 0 and
 * max_consecutive_invalid_steps >= 1.  sicp_stream_create applies the same rule to its params. */
int sicp_set_params(sicp_handle h, const sicp_params* p);
int sicp_get_params(sicp_handle h, sicp_params* p);

/* setSourceCloud / setTargetCloud (em_icp.h:50-66, gicp.h:42-70) and
 * setInputSource / setInputTarget (semantic_icp.h:41-49).  Copies the cloud to
 * HBM (SoA).  label may be NULL for SICP_MODE_GICP.  In SICP_MODE_SEMANTIC the
 * points are grouped by label in order of first appearance
 * (pcl_2_semantic.h:24-39); all outputs stay in the caller's point order. */
int sicp_set_cloud(sicp_handle h, int which, int32_t n, const float* x, const float* y,
                   const float* z, const uint32_t* label);
/* The same from an array of points as the reference holds them (pcl::PointCloud<pcl::PointXYZL>::points,
 * em_icp.h:37 / exec/kitti_eval.cc:132: x y z at bytes 0 4 8 of a 32-byte point, the label at 16; a plain
 * float[n][3] has stride 12): `xyz` = address of the first point's x, `label` = address of the first
 * point's uint32 label or NULL; strides in bytes.  One pass over the caller's memory, no intermediate
 * arrays. */
int sicp_set_cloud_strided(sicp_handle h, int which, int32_t n, const void* xyz, int64_t stride_bytes,
                           const void* label, int64_t label_stride_bytes);
/* Non-finite points (NaN / Inf in any coordinate, e.g. the invalid pixels of an organized RGB-D
 * cloud) are accepted and LEFT OUT of the device cloud, as pcl::KdTreeFLANN::setInputCloud
 * (called by setSourceCloud / setTargetCloud, em_icp.h:50-66) leaves them out of its index: they
 * are never found as neighbours and -- a NaN query keeps no candidate -- never matched, so they
 * contribute no residual.  Every per-point output keeps the caller's size and order; for a
 * dropped point: correspondences idx = -1, d2 = NaN, w = 0; normal / covariance NaN, histogram
 * 0, neighbour list -1; fused label 0; sicp_transform_source transforms it like any other point.
 * n_points = what the caller handed over (the size of per-point outputs), n_indexed = the finite
 * points held on the device.  Either output may be NULL. */
int sicp_cloud_size(sicp_handle h, int which, int32_t* n_points, int32_t* n_indexed);
/* same, from buffers already resident on the handle's device */
int sicp_set_cloud_device(sicp_handle h, int which, int32_t n, const float* x_device,
                          const float* y_device, const float* z_device,
                          const uint32_t* label_device);
/* setSourceCloud(cloud, kdtree, covs) / setTargetCloud(cloud, kdtree, covs) (gicp.h:48-56,
 * 64-70, em_icp.h:50-66 via getTargetKdTree()/getTargetCovariances(), used by
 * exec/kitti_eval.cc:207-226 to hand one scan's search tree and covariances from one
 * registration to the next): slot `which` of `h` refers to the SAME device-resident cloud
 * (points, search structure, normals, histograms) as slot `from_which` of `from`; nothing is
 * copied or rebuilt.  Both handles must be on the same device.  Handles that share a cloud may
 * run in one sicp_align_batch, or one after the other; two host threads must not ALIGN handles
 * that share a cloud at the same time.  One thing is safe across threads, because a sequence
 * driver needs it: while one thread registers handles (sicp_align / sicp_align_batch), another
 * may upload clouds into OTHER handles and sicp_share_cloud from a handle of the running call --
 * a shared cloud is never written by an align, a handle that gets a new cloud lets go of the
 * shared one instead of overwriting it, and the "upload still in flight" flag is atomic. */
int sicp_share_cloud(sicp_handle h, int which, sicp_handle from, int from_which);
/* setConfusionMatrix (em_icp.h:68-71); cm is C*C row-major, cm[r*C+s] */
int sicp_set_confusion(sicp_handle h, int32_t C, const double* cm_rowmajor);

/* ---- the hot path ------------------------------------------------------------ */
/* align(final, init) + getFinalTransFormation() + getOuterIter()
 * (em_icp.hpp:25-200, gicp.hpp:29-175, semantic_icp.hpp:28-166).
 * stats may be NULL. */
int sicp_align(sicp_handle h, const double init_qt[7], double out_qt[7],
               int32_t* outer_iters, sicp_stats* stats);
/* n independent align() calls -- one handle per scan pair, all on one device, equal in the
 * fields that decide what a launch does: mode, knn, k_cov, use_sqloss, nn_method, lm_on_device,
 * lm_batch and profile (anything else -- the trust-region options, outer_tol, max_outer, gate_sq,
 * epsilon, cauchy_a, num_classes and its matrix, min_class_pts, the quirks, reuse_features -- is
 * each pair's own) -- batched continuously: every launch of the inner solve evaluates the
 * pairs that are inside a solve (up to 256; with more, the others wait with their search done),
 * the searches of the pairs between two solves run between the launches (what
 * exec/kitti_eval.cc:124-249 does pair after pair).  Per pair the result is bit-identical to
 * sicp_align on that handle.  init_qt, out_qt: n*7; outer_iters (nullable): n; stats
 * (nullable): n.  No reference counterpart. */
int sicp_align_batch(sicp_handle* handles, int32_t n, const double* init_qt, double* out_qt,
                     int32_t* outer_iters, sicp_stats* stats);

/* ---- registration streams: an OPEN sequence of scan pairs --------------------------------------
 * The unit the reference iterates over is one align() per loop trip (exec/kitti_eval.cc:124-249:
 * ~4.5K stride-3 pairs of one odometry sequence, every scan the source of one registration and the
 * target of the next).  A stream is the continuous batching of sicp_align_batch without the closed
 * batch: registrations are submitted as their scans arrive and come out as they converge, up to
 * max_in_flight of them share the GPU, and a pair that needs 500 LM evaluations does not hold back the
 * batch it happened to be submitted with.  Per pair the result is bit-identical to sicp_align.
 *
 *   sicp_stream_create(device, params, max_in_flight, &s)   mode, K, tolerances ... of every registration
 *   sicp_stream_set_confusion(s, C, cm)                      SICP_MODE_EM
 *   id = sicp_stream_add_cloud(s, n, x, y, z, label)         setSourceCloud / setTargetCloud
 *        (em_icp.h:50-66): copies the cloud into pinned memory and queues upload + search-tree
 *        build on the stream's own HIP stream, beside the running registrations; returns at once.
 *        A cloud may take part in any number of registrations: it is uploaded and indexed once
 *        and its normals / histograms are computed once (what setSourceCloud(cloud, kdtree, covs),
 *        gicp.h:48-56, exists for).
 *   ticket = sicp_stream_submit(s, source_id, target_id, init_qt)   align(final, init); blocks
 *        while max_in_flight registrations are already waiting (back-pressure)
 *   sicp_stream_release_cloud(s, id)                         the caller is done with it; it is
 *        recycled when its last registration has finished
 *   sicp_stream_poll(s, wait, max, results, &n)              finished registrations, in order of
 *        completion: wait = 0 returns what is there, 1 waits for at least one result (or for the
 *        stream to run dry), 2 waits until everything submitted so far has finished
 *
 * A library-owned worker thread advances the registrations; submit / add_cloud / poll may be called
 * from any thread(s).  Requires the default engine (nn_method 1, lm_on_device 1, profile 0).
 * No reference counterpart. */
typedef struct sicp_stream_ctx* sicp_stream;
typedef struct sicp_stream_result {
  int64_t ticket;       /* what sicp_stream_submit returned */
  int32_t status;       /* SICP_OK, or why this registration could not run */
  int32_t outer_iters;  /* getOuterIter() */
  double qt[7];         /* getFinalTransFormation() */
  sicp_stats stats;     /* as from sicp_align, except total_active (0: not counted in a stream) */
} sicp_stream_result;
int sicp_stream_create(int device_id, const sicp_params* params, int32_t max_in_flight, sicp_stream* out);
int sicp_stream_destroy(sicp_stream s);  /* registrations still in flight are abandoned */
int sicp_stream_set_confusion(sicp_stream s, int32_t C, const double* cm_rowmajor);
int sicp_stream_add_cloud(sicp_stream s, int32_t n, const float* x, const float* y, const float* z,
                          const uint32_t* label, int64_t* cloud_id);
/* sicp_stream_add_cloud from an array of points (see sicp_set_cloud_strided) */
int sicp_stream_add_cloud_strided(sicp_stream s, int32_t n, const void* xyz, int64_t stride_bytes,
                                  const void* label, int64_t label_stride_bytes, int64_t* cloud_id);
int sicp_stream_release_cloud(sicp_stream s, int64_t cloud_id);
int sicp_stream_submit(sicp_stream s, int64_t source_id, int64_t target_id, const double init_qt[7],
                       int64_t* ticket);
/* sicp_stream_submit with options (flags = 0: the same):
 *   SICP_SUBMIT_FUSED_LABELS   SICP_MODE_EM: getFusedLabels(out, final pose) (em_icp.hpp:202-268, what
 *       exec/scenenet_eval.cc:193-198 calls right after align) is computed when the registration retires -- one more
 *       K = 4 search and one label kernel, queued beside the running registrations -- and kept until
 *       sicp_stream_take_labels(ticket) fetches it (once; n = the source cloud's point count, caller order).  The
 *       registration's result is only handed out by sicp_stream_poll when its labels are there.  Taking them is
 *       the caller's side of the contract: a label set (4 bytes per source point) stays in host memory until it is taken or
 *       the stream is destroyed -- a caller may take them long after the poll that returned the registration.
 *   SICP_SUBMIT_FRESH_FEATURES the normals / label histograms of BOTH clouds are recomputed for this registration,
 *       like every align() of the reference does (em_icp.hpp:28-29, gicp.hpp:33-34), instead of being kept with the
 *       cloud (a stream's default: what setSourceCloud(cloud, kdtree, covs) exists for).  Same values either way.
 *   SICP_SUBMIT_POSE_COVARIANCE (any mode; may be combined with the other two) the sums of sicp_pose_covariance at the
 *       final pose are computed when the registration retires -- one more search at that pose, one accumulate sweep and
 *       the covariance kernels, shared by all flagged registrations that retire in the same turn and queued beside the
 *       running ones -- and kept (about 0.6 KB) until sicp_stream_take_pose_covariance(ticket) fetches them.  The
 *       registration's result is only handed out by sicp_stream_poll when they are there; its pose, outer_iters and
 *       counters are those of the same registration without the flag.
 * The value 8, not 4: bit 4 has always been refused as an unknown flag and stays refused, as do bits 16 and above. */
enum { SICP_SUBMIT_FUSED_LABELS = 1, SICP_SUBMIT_FRESH_FEATURES = 2, SICP_SUBMIT_POSE_COVARIANCE = 8 };
int sicp_stream_submit_ex(sicp_stream s, int64_t source_id, int64_t target_id, const double init_qt[7],
                          uint32_t flags, int64_t* ticket);
int sicp_stream_take_labels(sicp_stream s, int64_t ticket, int32_t n, uint32_t* out_labels);
int sicp_stream_poll(sicp_stream s, int32_t wait, int32_t max_results, sicp_stream_result* results,
                     int32_t* n_results);
/* counters since creation: registrations submitted / finished, and -- over the finished ones -- their
 * own LM evaluations and the evaluation launches they sat through (busy fraction = the ratio).  Any
 * output may be NULL. */
int sicp_stream_counters(sicp_stream s, int64_t* submitted, int64_t* completed, int64_t* busy_evals,
                         int64_t* slot_evals);
const char* sicp_stream_last_error(sicp_stream s);

/* Caller-supplied per-point covariances, where the reference reads them instead of computing them:
 * SemanticIterativeClosestPoint::align takes whatever sits in the public `labeledCovariances` of its two clouds
 * (impl/semantic_icp.hpp:73,77; semantic_point_cloud.h:36-42: addSemanticCloud(..., computeKd, computeCov = false) leaves
 * them to the caller), and GICP::setSourceCloud(cloud, tree, covs) / setTargetCloud(cloud, tree, covs) (gicp.h:50-55, 65-70)
 * accept arbitrary vectors (GICP::align and EmIterativeClosestPoint::align then overwrite them, impl/gicp.hpp:33-34,
 * impl/em_icp.hpp:28-29 -- which is what this engine does too unless reuse_features is set).
 * cov9: n_points x 9 row-major 3x3 matrices in the caller's point order.
 *   - every matrix of the form the reference's own routine produces, C = I - (1 - epsilon) n n^T (a unit normal n; epsilon =
 *     params.epsilon; to 1e-8): the engine keeps the normals and registers with its product kernels, batches and streams included;
 *   - otherwise, every matrix symmetric and finite (SICP_MODE_GICP / SICP_MODE_SEMANTIC): kept as they are, and the cloud's
 *     registrations evaluate gicp_cost_function.h:27-73 on the full 3x3 matrices (its closed form for symmetric covariances),
 *     with the trust-region loop on the host: correct to the same tolerances, ONE PAIR AT A TIME (sicp_align, sicp_solve,
 *     sicp_accumulate; sicp_align_batch of more than one pair and streams answer SICP_ERR_INVALID_ARGUMENT) and far from the
 *     product path's speed -- the path of an exotic input, e.g. exec/test_gradient.cc:32-50's fixture;
 *   - anything else (a non-symmetric or non-finite matrix; a general matrix in SICP_MODE_EM, whose align() recomputes
 *     covariances and label histograms together) is REFUSED: SICP_ERR_INVALID_ARGUMENT, sicp_last_error names the first
 *     offending point, nothing is changed -- never a silent replacement.
 * Accepted covariances count as the cloud's current features for SICP_MODE_SEMANTIC, and for SICP_MODE_GICP with
 * reuse_features = 1 (without it align() recomputes them, as impl/gicp.hpp:33-34 does).  Entries of non-finite points (which
 * never reach the device) are ignored.  sicp_covariances hands back what is there. */
int sicp_set_covariances(sicp_handle h, int which, const double* cov9);

/* the final_cloud output of align (em_icp.hpp:192-198): source transformed by
 * float(matrix(qt)); ox/oy/oz are host buffers of n_source floats */
int sicp_transform_source(sicp_handle h, const double qt[7], float* ox, float* oy, float* oz);

/* getFusedLabels (em_icp.hpp:202-268): out_labels[n_source] */
int sicp_fused_labels(sicp_handle h, const double qt[7], uint32_t* out_labels);

/* ---- initial alignment without a pose prior ------------------------------------------------------
 * The reference's Bootstrap (exec/bootstrap.h): box filter -> VoxelGrid -> NormalEstimation -> FPFHEstimation on the
 * keypoints of both clouds -> SampleConsensusInitialAlignment.  Registers the handle's current source onto its current
 * target from no initial guess; the result is a coarse pose for sicp_align's init_qt.  Works in every mode, ignores
 * labels (sicp_bootstrap_semantic below uses them), uses the finite points the handle holds.  Orders, precisions and the deviations from PCL: INTEGRATION.md. */
typedef struct sicp_bootstrap_params {
  double box_max;              /* keep a point when x < box_max && y < box_max && z < box_max: 35 (bootstrap.h:24-28) */
  double leaf_size;            /* VoxelGrid leaf: 0.4 (bootstrap.h:29-33)                                              */
  double normal_radius;        /* NormalEstimation radius: 3 (bootstrap.h:105)                                         */
  double feature_radius;       /* FPFHEstimation radius: 3 (bootstrap.h:112)                                           */
  double min_sample_distance;  /* 0.4 (bootstrap.h:57)                                                                 */
  double max_corr_distance;    /* TruncatedError threshold: 0.8 (bootstrap.h:58)                                       */
  int32_t max_iterations;      /* hypotheses: 500 (bootstrap.h:59)                                                     */
  int32_t nr_samples;          /* points per hypothesis: 3 (PCL default), 3..8                                         */
  int32_t k_correspondences;   /* feature neighbours one is drawn from: 10 (PCL default), 1..16                        */
  int32_t reserved_;
  uint64_t seed;               /* splitmix64 state of the sampling: 1                                                  */
} sicp_bootstrap_params;
typedef struct sicp_bootstrap_info {
  int32_t n_source_keypoints, n_target_keypoints;  /* voxel centroids of the box-filtered clouds              */
  int32_t max_neighbours;      /* largest radius neighbourhood of either cloud (the point itself included)    */
  int32_t best_iteration;      /* hypothesis that won (0-based)                                               */
  double best_error;           /* its summed truncated error                                                  */
  double t_keypoints_ms, t_features_ms, t_match_ms, t_score_ms, t_total_ms;  /* host wall clock per stage    */
} sicp_bootstrap_info;
int sicp_default_bootstrap_params(sicp_bootstrap_params* p);
/* out_qt[7]: the coarse pose source -> target; info may be NULL.  SICP_ERR_TOO_FEW_POINTS when the source has fewer
 * than nr_samples keypoints with features or the target none; SICP_ERR_INVALID_ARGUMENT for a bad parameter or a voxel
 * grid whose cell count overflows int32 (PCL silently returns the input there).  Nothing on the handle changes. */
int sicp_bootstrap(sicp_handle h, const sicp_bootstrap_params* p, double out_qt[7], sicp_bootstrap_info* info);
/* sicp_bootstrap for n pairs at once: pair i = handle hs[i]'s current source onto its current target, with the same
 * params for every pair.  Per pair bit-identical to sicp_bootstrap(hs[i], p, ...): pose, info counts, best_iteration
 * and best_error (the t_*_ms fields hold the batch's stage times, the same in every info).  status[n] (nullable)
 * gets each pair's own code; the call returns SICP_OK when every pair succeeded, else the first failing pair's code.
 * A pair that fails (SICP_ERR_NOT_READY: a handle without both clouds; SICP_ERR_TOO_FEW_POINTS; SICP_ERR_INVALID_ARGUMENT:
 * a voxel grid that overflows int32) does not stop the others; its out_qt row and info are not written, and the message
 * (sicp_last_error of its handle, and of hs[0] for the first failing pair) names the pair's index.  A failure of the call
 * itself (HIP, memory) is every unfinished pair's status.  out_qt n*7; infos nullable.  Handles may be in any mode, may
 * repeat, and may share clouds (sicp_share_cloud): a cloud's keypoints and features are computed once per call.  n has no
 * upper bound (the work runs in groups of bounded scratch).  Refused before any work, with SICP_ERR_INVALID_ARGUMENT and
 * nothing written: n < 1, a NULL array or handle, handles on different devices, bad params.  Nothing on any handle
 * changes. */
int sicp_bootstrap_batch(sicp_handle* hs, int32_t n, const sicp_bootstrap_params* p, double* out_qt, int32_t* status,
                         sicp_bootstrap_info* infos);
/* ---- label-aware initial alignment ------------------------------------------------
 * sicp_bootstrap with the clouds' labels (an extension: the reference has no such stage).  Labels are any uint32 values,
 * compared for equality only; the mode, num_classes and the confusion matrix play no part.  Both clouds must carry labels.
 *   filter   a point is kept when it is finite, passes the box filter and its label is not in `ignore` (moving classes:
 *            cars, people); the voxel grid is sicp_bootstrap's over the kept points.
 *   labels   a keypoint gets the most frequent label of its voxel's kept points, ties to the smallest label (the rule of
 *            sicp_merge_clouds).
 *   match    match_same_label: a source keypoint's feature neighbours are the k_correspondences nearest among the target
 *            keypoints with a feature AND its label (fewer: the row ends in -1); a source keypoint can be sampled when it
 *            has a feature and at least one such neighbour, and its target is drawn among the neighbours it has.
 *   score    score_same_label: a source keypoint whose nearest target keypoint lies within max_corr_distance but carries
 *            another label scores 1, as an outlier does.
 * With both flags 0 and n_ignore 0, and with both flags 1 on clouds of a single label, the result is sicp_bootstrap's bit
 * for bit.  Orders and precisions: INTEGRATION.md ("Bootstrap"). */
#define SICP_BOOTSTRAP_MAX_IGNORE 64
typedef struct sicp_bootstrap_label_params {
  int32_t match_same_label;  /* 1 (default): a source keypoint's feature neighbours are drawn only from target keypoints of its label */
  int32_t score_same_label;  /* 1 (default): a source keypoint whose nearest target keypoint has another label scores 1 (an outlier) */
  int32_t n_ignore;          /* 0 (default) .. SICP_BOOTSTRAP_MAX_IGNORE */
  int32_t reserved_;
  uint32_t ignore[SICP_BOOTSTRAP_MAX_IGNORE]; /* points with one of these labels are dropped with the box filter, in both clouds */
} sicp_bootstrap_label_params;
int sicp_default_bootstrap_label_params(sicp_bootstrap_label_params* lp);
/* As sicp_bootstrap (statuses, info, nothing on the handle changes).  SICP_ERR_TOO_FEW_POINTS when fewer than nr_samples
 * source keypoints can be sampled or the target has no keypoint with a feature.  Refused with SICP_ERR_INVALID_ARGUMENT,
 * nothing written and the reason in sicp_last_error: a NULL lp, n_ignore outside 0..64, a flag that is neither 0 nor 1,
 * a cloud without labels. */
int sicp_bootstrap_semantic(sicp_handle h, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp,
                            double out_qt[7], sicp_bootstrap_info* info);
/* As sicp_bootstrap_batch, with the same p and lp for every pair; per pair bit-identical to sicp_bootstrap_semantic.  A
 * pair with a cloud without labels fails alone (SICP_ERR_INVALID_ARGUMENT in its status); a NULL or bad lp refuses the call. */
int sicp_bootstrap_semantic_batch(sicp_handle* hs, int32_t n, const sicp_bootstrap_params* p,
                                  const sicp_bootstrap_label_params* lp, double* out_qt, int32_t* status,
                                  sicp_bootstrap_info* infos);
/* ---- how well a registration's pose is determined ------------------------------
 * The 6x6 covariance of the pose at qt (Censi's estimate with the solver's Gauss-Newton matrix), in the tangent space of
 * the right perturbation T * exp(delta), delta = [upsilon; omega] (units m^2, m rad, rad^2).  The slots are those
 * sicp_correspondences(qt) finds (gate, EM weights, SEMANTIC label segments and min_class_pts included); with them, the
 * weights, both clouds' covariances and R held fixed, per slot i with gradient share g_i = rho'(r^2) r J:
 *   B_i^p = d g_i / d p_i,  B_i^q = d g_i / d q_i   (6x3; kappa = rho' + 2 s rho'' in closed form)
 *   G_j = sum of B^p over source point j's slots,  G_k = sum of B^q over every slot whose target is point k
 *   S_src = sum_j G_j G_j^T,  S_tgt = sum_k G_k G_k^T,  H = the Gauss-Newton sums of sicp_accumulate at qt
 *   covariance    = H^-1 (sigma_source^2 S_src + sigma_target^2 S_tgt) H^-1   (isotropic point noise sigma^2 I)
 *   covariance_gn = H^-1                                                     (what ceres::Covariance gives for the pose)
 * For the left form (perturbation exp(delta) * T) use Ad_T Sigma Ad_T^T.  Not modelled: how the point covariances depend
 * on neighbouring points, changes in the data association, the exact Hessian. */
typedef struct sicp_pose_covariance_result {
  double hessian[21];        /* = sicp_accumulate out28[0:21] at qt after sicp_correspondences(qt): same order, same bits */
  double gradient[6];        /* = out28[21:27] */
  double cost;               /* = out28[27] */
  double cross_source[21];   /* S_src, upper triangle in hessian's order */
  double cross_target[21];   /* S_tgt, likewise */
  double covariance[36];     /* row-major; NaN unless positive_definite */
  double covariance_gn[36];  /* H^-1, row-major; NaN unless positive_definite */
  int64_t active;            /* slots that passed the gate */
  int32_t positive_definite; /* the Cholesky factorisation of H succeeded */
  int32_t reserved_;
} sicp_pose_covariance_result;
/* The handle's correspondences end up as after sicp_correspondences(qt).  H that is not positive definite (zero active
 * slots included) gives positive_definite = 0, NaN covariances and SICP_OK.  Refused with SICP_ERR_INVALID_ARGUMENT and
 * nothing written: a NULL handle, qt or out; a sigma that is negative or not finite; a cloud that holds caller covariances
 * of general form (sicp_set_covariances; the reason in sicp_last_error).  Missing clouds or confusion matrix:
 * SICP_ERR_NOT_READY, as sicp_align.  Bit-reproducible: no float atomics anywhere in the sums. */
int sicp_pose_covariance(sicp_handle h, const double qt[7], double sigma_source, double sigma_target,
                         sicp_pose_covariance_result* out);
/* sicp_pose_covariance for n pairs: pair i = handle hs[i] at qt[7 i .. 7 i + 7), out[i].  The pairs run in groups that
 * share every launch -- one job flush for the searches, the batched accumulate kernel, the covariance kernels over a job
 * table with one sort, one read-back and one wait per group; a group holds a handle once (a handle may repeat in the
 * call) and is bounded by its scratch -- and a pair keeps the summation order of its lone call, so every row is
 * bit-identical to it.  Handles may be in different modes.  status[n]
 * (nullable) gets each pair's own code; a failing pair does not stop the others and its row is not written; the call
 * returns SICP_OK when every pair succeeded, else the first failing pair's code.  Refused before any work, with
 * SICP_ERR_INVALID_ARGUMENT and nothing written: n < 1, a NULL array or handle, a bad sigma, handles on different devices.
 * Streams: SICP_SUBMIT_POSE_COVARIANCE and sicp_stream_take_pose_covariance. */
int sicp_pose_covariance_batch(sicp_handle* hs, int32_t n, const double* qt, double sigma_source, double sigma_target,
                               sicp_pose_covariance_result* out, int32_t* status);
/* The pose covariance of a registration submitted with SICP_SUBMIT_POSE_COVARIANCE, once sicp_stream_poll has handed the
 * registration out: *out is what sicp_pose_covariance(h, final pose, sigma_source, sigma_target) gives on a handle that
 * holds the two clouds, bit for bit (the stream keeps the sums; the 6x6 algebra runs here, with these sigmas -- which is
 * why they are no submit arguments).  H that is not positive definite: positive_definite = 0, NaN matrices, SICP_OK.  A
 * successful call takes the entry: it works once per ticket.  SICP_ERR_NOT_READY: the ticket was not flagged, is not
 * finished, or has been taken.  SICP_ERR_INVALID_ARGUMENT, nothing written and the entry kept (a later correct call
 * succeeds): a NULL stream or out, a sigma that is negative or not finite. */
int sicp_stream_take_pose_covariance(sicp_stream s, int64_t ticket, double sigma_source, double sigma_target,
                                     sicp_pose_covariance_result* out);

/* ---- how well the clouds fit at a pose -----------------------------------------
 * The question after align(): overlap, inlier RMSE and label agreement of the handle's source onto its target at qt -- what
 * PCL calls getFitnessScore, Open3D evaluate_registration, and the reference ROCMetrics::evaluate (exec/roc_metrics.h:21-41:
 * the nearest target of every transformed source point, kept when d^2 < 25, and the two labels).  The queries are the finite
 * source points transformed exactly as sicp_correspondences transforms them; the candidates are the WHOLE target cloud; per
 * query the result is the one nearest neighbour under the search's own order (float32 d^2, ties to the lower caller index).
 * The same in every mode: params.knn, gate_sq, min_class_pts and the mode's label segments play no part (on a
 * SICP_MODE_SEMANTIC handle, whose target holds one search tree per label, the trees' winners are merged by (d^2, caller
 * index): the result does not depend on the layout). */
typedef struct sicp_evaluate_result {
  int64_t n_source;      /* queries = finite source points the handle holds */
  int64_t inliers;       /* queries whose nearest target has d2 < (float)max_dist_sq, strict (roc_metrics.h:34; the gate's own rule) */
  int64_t label_agree;   /* inliers with equal labels; 0 when either cloud was set without labels */
  int64_t label_outside; /* inliers left out of the table because a label is outside 1..C; 0 when no table was asked for */
  double  sum_d2;        /* sum of the inliers' float32 d2, accumulated in double in a fixed order */
  double  fitness;       /* inliers / n_source; 0 when n_source = 0 */
  double  inlier_rmse;   /* sqrt(sum_d2 / inliers); NaN when inliers = 0 */
  double  reserved_;
} sicp_evaluate_result;
/* confusion (nullable, num_classes^2 counts, row-major): confusion[(ls - 1) * C + (lt - 1)] = inliers with source label ls and
 * target label lt, the tabulated output of ROCMetrics::evaluate; num_classes is read only with it.  nn_idx / nn_d2 (nullable,
 * n_points of the source each, caller order): the nearest target's caller index and d^2; a query without an inlier gets -1
 * and keeps its d^2, a non-finite source point (sicp_cloud_size) gets -1 and NaN.
 * Needs both clouds and nothing else: no confusion matrix, no features (no self-search, no covariances -- clouds with caller
 * covariances of any form are fine).  Nothing on the handle changes: its correspondences, statistics and solver state are
 * those from before the call (the searches write to scratch of their own).  SICP_ERR_NOT_READY: a cloud is missing (or, on a
 * SICP_MODE_SEMANTIC handle, has no labels to lay its trees out by); SICP_ERR_TOO_FEW_POINTS: the target holds no finite
 * point; n_source = 0: SICP_OK, zeros and a NaN inlier_rmse.  Refused with SICP_ERR_INVALID_ARGUMENT before any device call,
 * nothing written: a NULL handle, qt or out; max_dist_sq NaN or <= 0 (+inf is allowed: every query is an inlier); confusion
 * with num_classes outside 1..255 or with a cloud that has no labels.  Bit-reproducible: integer counts, and sum_d2 from
 * partial sums over fixed chunks of 256 queries added in index order -- no float atomics. */
int sicp_evaluate(sicp_handle h, const double qt[7], double max_dist_sq, int32_t num_classes, int64_t* confusion,
                  int32_t* nn_idx, float* nn_d2, sicp_evaluate_result* out);
/* sicp_evaluate for n pairs: pair i = handle hs[i] at qt[7 i .. 7 i + 7), out[i], confusion + i C^2 (nullable; no per-point
 * outputs).  The pairs run in groups that share every launch -- one job flush for all searches, one evaluation launch, one
 * read-back and one wait per group; a group holds a handle once (a handle may repeat in the call) and is bounded by its
 * scratch -- and every row, tables included, is bit-identical to the pair's lone call.  Handles may be in different modes and
 * may share clouds.  status[n] (nullable) gets each pair's own code; a failing pair does not stop the others and its row and
 * table are not written; the call returns SICP_OK when every pair succeeded, else the first failing pair's code.  Refused
 * before any work, with SICP_ERR_INVALID_ARGUMENT and nothing written: n < 1, a NULL array or handle, a bad max_dist_sq, a
 * table with num_classes outside 1..255, handles on different devices. */
int sicp_evaluate_batch(sicp_handle* hs, int32_t n, const double* qt, double max_dist_sq, int32_t num_classes,
                        int64_t* confusion, sicp_evaluate_result* out, int32_t* status);

/* ---- registered scans into one cloud --------------------------------------------
 * The step after align() in scan-to-local-map odometry: several clouds, each at its pose, cropped about the vehicle and
 * reduced on a voxel grid to the next target, without leaving the device.  Part i is slot part_which[i] of handle parts[i];
 * handles may be in any mode (and modes may be mixed), may repeat and may share clouds; dst may be one of the parts (the
 * rolling map: map = merge(map, scan)).
 *  1. The points are the finite points each cloud holds (sicp_cloud_size's n_indexed) in caller order, the parts in the order
 *     given; a point's global index is its position in that concatenation.  The result does not depend on a cloud's device
 *     layout (a SICP_MODE_SEMANTIC handle groups it by label).
 *  2. Transform, exactly as sicp_correspondences transforms sources: the matrix of qt as the engine forms it (no
 *     normalisation), ((m0 x + m1 y) + m2 z) + m3 in double without contraction, one rounding to float.  qt = NULL: identities,
 *     through the same arithmetic.
 *  3. Crop, when crop_range > 0: c = (float)crop_center, d = p - c in float, d2 = (dx dx + dy dy) + dz dz in float (each
 *     operation rounded), kept when (double)d2 <= crop_range * crop_range.  With the identity, centre 0 and leaf_size 0 this is
 *     the reference drivers' filterRange(cloud, range) (exec/filter_range.h), value for value.
 *  4. Voxel grid, when leaf_size > 0: v = floor(p * (1.0f / (float)leaf_size)) per axis in float -- an absolute grid anchored
 *     at the origin, so a merge is stable from call to call; the voxel membership is that of sicp_bootstrap's grid.  One
 *     output point per occupied voxel in ascending (vz, vy, vx): the double sum of the voxel's points in ascending global index,
 *     divided by their number, rounded once to float; count[j] = that number; label[j] = the most frequent label of the voxel,
 *     ties to the smallest label value (labels are arbitrary uint32).  |v| >= 2^20 on any axis: SICP_ERR_INVALID_ARGUMENT (the
 *     text names the leaf size).
 *  5. leaf_size = 0: the result is the kept points themselves in global index order, their own labels, count = 1.
 *  6. Labels: every part's cloud has them -> the result has them; none has -> it has none (label untouched, has_label = 0); a
 *     mixture is refused. */
typedef struct sicp_merge_params {
  double leaf_size;       /* voxel edge; 0 = no voxel grid.  default 0.2 */
  double crop_center[3];  /* default 0 0 0 */
  double crop_range;      /* 0 = no crop (default); +inf allowed (keeps everything finite) */
} sicp_merge_params;
typedef struct sicp_merge_info {
  int64_t n_in;              /* finite points of all parts (a cloud used twice counts twice) */
  int64_t n_kept;            /* after the crop */
  int32_t n_out;             /* points of the result */
  int32_t max_voxel_points;  /* 1 when leaf_size = 0 and n_out > 0; 0 when n_out = 0 */
  int32_t has_label, reserved_;
  double t_total_ms;         /* host wall clock */
} sicp_merge_info;
int sicp_default_merge_params(sicp_merge_params* p);
/* Outputs: info (nullable) is written on success and on the capacity refusal; an output array (each nullable, capacity
 * elements) is written when it is non-NULL and capacity >= n_out; a non-NULL array with a smaller capacity gives
 * SICP_ERR_INVALID_ARGUMENT and nothing else happens (call once without arrays, or size them by the sum of n_indexed).
 * dst (nullable): slot dst_which of dst becomes the result exactly as if the caller had passed the output arrays to
 * sicp_set_cloud -- everything downstream, sicp_align included, is bit-identical to that; the whole result is computed before
 * the slot lets go of its old cloud, and other handles sharing the old cloud keep it (sicp_share_cloud's rule).  n_out = 0
 * with a dst: SICP_ERR_TOO_FEW_POINTS, dst unchanged.
 * Refused before any work, with SICP_ERR_INVALID_ARGUMENT and nothing written: n_parts < 1; a NULL array or handle; a `which`
 * outside SICP_SOURCE / SICP_TARGET; handles (dst included) on different devices; leaf_size negative or not finite;
 * crop_range negative or NaN; a centre or pose that is not finite; labelled and unlabelled parts together; more than 2^31 - 1
 * points in all.  SICP_ERR_NOT_READY: a part's slot holds no cloud (or, on a SICP_MODE_SEMANTIC handle, a cloud that was never
 * uploaded because it has no labels).  No part's cloud, correspondences, features or statistics change, unless it is dst's
 * slot; parts already on the device are not uploaded again.  Bit-reproducible: a stable sort and fixed-order sums, no float
 * atomics.  Streams: merge on handles and pass the arrays to sicp_stream_add_cloud.  For a map that rolls on from scan to
 * scan use a sicp_map (below): a merged cloud that goes back in as a part counts every point of it as one observation. */
int sicp_merge_clouds(sicp_handle* parts, const int32_t* part_which, int32_t n_parts, const double* qt /* n_parts*7, NULL = identities */,
                      const sicp_merge_params* p, sicp_handle dst /* nullable */, int dst_which,
                      int32_t capacity, float* x, float* y, float* z, uint32_t* label, uint32_t* count /* all nullable */,
                      sicp_merge_info* info /* nullable */);

/* ---- objects of a labelled cloud -------------------------------------------------
 * Label-aware Euclidean clustering of the cloud in a handle's slot (what PCL users know as pcl::EuclideanClusterExtraction /
 * pcl::LabeledEuclideanClusterExtraction): the connected components of the graph below, numbered, with one table row --
 * label, count, first index, centroid, box -- per cluster.  The handle may be in any mode.
 *  1. Vertices.  The finite points the slot's cloud holds (sicp_cloud_size's n_indexed); a point whose label equals one of
 *     ignore[0 .. n_ignore) is not a vertex.  The result does not depend on the cloud's device layout (a SICP_MODE_SEMANTIC
 *     handle groups it by label): the same cloud gives the same bytes on a handle of any mode, in either slot.
 *  2. Edges.  p and q are joined iff d2 < t2, strict (sicp_evaluate's rule), and (same_label = 0 or their labels are equal):
 *     d = p - q in float, d2 = (dx dx + dy dy) + dz dz in float, every operation rounded on its own, no contraction (the crop
 *     arithmetic of sicp_merge_clouds, step 3); t2 = (float)tolerance * (float)tolerance in float.  d2 is symmetric in p and
 *     q: the graph is undirected.
 *  3. Clusters.  The connected components whose size lies in [min_points, max_points] (max_points = 0: no upper bound),
 *     numbered 0, 1, ... in ascending order of their smallest caller index, which is first_index[c].  cluster_id[i] is that
 *     number; -1 for a non-finite point, an ignored label, and a member of a component outside the bounds.
 *  4. Per cluster.  count[c]: its points.  label[c]: the most frequent label of its points, ties to the smallest value (the
 *     merge's rule; with same_label = 1 the one label they share).  centroid[3 c ..]: per axis the float64 sum of the members'
 *     float coordinates in ascending caller index, one add per point, divided by the count in double (the merge's order).
 *     bbox_min / bbox_max[3 c ..]: the members' float extremes.
 *  5. Labels.  A cloud set without labels is accepted only with same_label = 0 and n_ignore = 0, and label[] is then written
 *     as 0; otherwise it is SICP_ERR_INVALID_ARGUMENT.  On a SICP_MODE_SEMANTIC handle a cloud that was never uploaded for want
 *     of labels gives SICP_ERR_NOT_READY, as it does in sicp_merge_clouds.
 *  6. Capacity (the merge's rule).  The table arrays hold `capacity` rows (centroid, bbox_min, bbox_max: 3 values per row); each
 *     is nullable.  A non-NULL table array with capacity < n_clusters: SICP_ERR_INVALID_ARGUMENT with info written and nothing
 *     else (call once without arrays to size them).  cluster_id (nullable) has no capacity: it is n_points long, caller order.
 *  7. Nothing on the handle changes: cloud, tree, features, correspondences, statistics and solver state stay, and a later
 *     sicp_align returns the bytes it returns on a handle that never made the call.  Needs the cloud and nothing else; a cloud
 *     not yet on the device is prepared as a part of sicp_merge_clouds is.
 *  8. n_kept = 0 (no finite point, or every label ignored): SICP_OK, no clusters, cluster_id all -1.  The slot holds no cloud:
 *     SICP_ERR_NOT_READY.
 *  9. Refused before any device work, with SICP_ERR_INVALID_ARGUMENT, nothing written and the reason in sicp_last_error: a NULL
 *     handle or params; a `which` outside SICP_SOURCE / SICP_TARGET; a tolerance that is not finite or <= 0; min_points < 1;
 *     max_points negative, or positive and below min_points; same_label not 0 or 1; n_ignore outside 0 .. SICP_CLUSTER_MAX_IGNORE;
 *     capacity < 0.  Refused after the first kernel, in the same way: a point whose cell of the internal search grid (edge: a
 *     hair above the tolerance) has a coordinate of 2^20 - 1 or more in magnitude -- the text names the tolerance.
 * 10. Bit-reproducible: a function of the points, labels and parameters only, the same bytes for every launch shape and from
 *     run to run -- integer atomics decide a partition that does not depend on their order, every float sum runs in a fixed
 *     order, no float atomics.  Permuting the input permutes cluster_id and renumbers the clusters; the partition, counts,
 *     labels and boxes stay, and centroids may differ in their last bits (the order of the adds changes). */
#define SICP_CLUSTER_MAX_IGNORE 64
typedef struct sicp_cluster_params {
  double tolerance;     /* > 0, finite.  default 0.5 */
  int32_t min_points;   /* >= 1.  default 10 */
  int32_t max_points;   /* 0 = no limit (default); otherwise >= min_points */
  int32_t same_label;   /* 1 (default): only points of equal label are joined; 0: labels play no part in joining */
  int32_t n_ignore;     /* 0 .. SICP_CLUSTER_MAX_IGNORE.  default 0 */
  uint32_t ignore[SICP_CLUSTER_MAX_IGNORE];
} sicp_cluster_params;
typedef struct sicp_cluster_info {
  int64_t n_points;            /* what the caller handed over (the size of cluster_id) */
  int64_t n_kept;              /* vertices: finite points whose label is not ignored */
  int64_t n_components;        /* connected components of all sizes */
  int64_t n_clustered;         /* points with cluster_id >= 0 */
  int32_t n_clusters;          /* components with min_points <= size <= max_points */
  int32_t max_cluster_points;  /* 0 when n_clusters = 0 */
  double t_total_ms;           /* host wall clock */
} sicp_cluster_info;
int sicp_default_cluster_params(sicp_cluster_params* p);
int sicp_cluster(sicp_handle h, int which, const sicp_cluster_params* p, int32_t* cluster_id /* n_points, nullable */,
                 int32_t capacity, uint32_t* label, int32_t* count, int32_t* first_index, double* centroid /* 3 per cluster */,
                 float* bbox_min, float* bbox_max /* 3 per cluster each; all nullable */, sicp_cluster_info* info /* nullable */);

/* ---- filtering a cloud -----------------------------------------------------------
 * Removes points from the cloud in a handle's slot: the statistical outlier test (pcl::StatisticalOutlierRemoval, Open3D's
 * remove_statistical_outlier), the radius outlier test (pcl::RadiusOutlierRemoval, remove_radius_outlier), a caller's mask and
 * label lists, in one call; the kept points can become a slot's cloud without leaving the device's side of the library.  The
 * handle may be in any mode.
 *  1. Classes.  A point is REMOVED when it is not finite, when mask is given and mask[i] == 0, or when its label is one of
 *     drop[0 .. n_drop); otherwise it is PROTECTED when its label is one of protect[0 .. n_protect); otherwise it is TESTED.  A
 *     label in both lists is refused.  A cloud set without labels is accepted only with both lists empty (rule 5 of
 *     sicp_cluster).
 *  2. Neighbours are the finite points of the cloud, whatever their class (PCL's filters with indices: the searcher sees the
 *     whole input, the indices are judged).
 *  3. Statistical test (mean_k > 0).  For a tested point i take the mean_k + 1 smallest float32 squared distances from p_i to
 *     the finite points, p_i included -- d2 = (dx dx + dy dy) + dz dz in float, every operation rounded on its own (rule 2 of
 *     sicp_cluster) -- in ascending order, and leave the first out.  m_i = (sum of (double)sqrtf(d2_j)) / (double)mean_k: the
 *     float roots correctly rounded, the terms added to a double in ascending order.  Only values enter: ties need no order.
 *     S1 = sum m_i and S2 = sum m_i m_i over the tested points are sums over the perfect binary tree on the caller's indices
 *     0 .. 2^ceil(log2 n_points) - 1: absent entries are +0.0, and level by level s[j] = s[2 j] + s[2 j + 1].  mean = S1 /
 *     n_tested; var = max(0, (S2 - S1 S1 / n_tested) / (n_tested - 1)); threshold = mean + std_mul sqrt(var) -- double
 *     operations, each rounded on its own, none contracted.  The point passes when m_i <= threshold.  Fewer than mean_k + 1
 *     finite points, or fewer than 2 tested points: SICP_ERR_TOO_FEW_POINTS.
 *  4. Radius test (radius > 0).  c_i = the number of finite j != i with d2 < r2, strict, r2 = (float)radius * (float)radius in
 *     float (the edge rule of sicp_cluster).  The point passes when c_i >= min_neighbors.  neighbors[i] = min(c_i,
 *     min_neighbors): counting stops at the answer.  A point whose cell of the internal search grid (edge: a hair above the
 *     radius) has a coordinate of 2^20 - 1 or more in magnitude: SICP_ERR_INVALID_ARGUMENT, the text names the radius (rule 9 of
 *     sicp_cluster).
 *  5. Both tests judge the same set: a tested point is kept when it passes every test that is on.  With both off the call is
 *     a pure selection by mask and labels.
 *  6. Outputs, all nullable, n_points long, caller order.  keep[i]: 1 for kept and protected points, else 0.  mean_dist[i]:
 *     m_i; NaN for a point that is not tested, and for every point when the statistical test is off.  neighbors[i]: as in 4;
 *     -1 for a point that is not tested, and for every point when the radius test is off.
 *  7. info: the counts -- n_fail_stat and n_fail_radius each on its own, a point may be in both -- and mean, stddev =
 *     sqrt(var), threshold (NaN when the statistical test is off).
 *  8. dst (nullable; needs the same device; may be h with dst_which = which: the cloud is filtered in place).  The kept points in
 *     ascending caller index, with their labels, become the cloud of dst's slot, exactly as sicp_set_cloud of those arrays
 *     would set it.  An empty result with dst: SICP_ERR_TOO_FEW_POINTS and dst keeps its cloud (the merge's rule).
 *  9. Every refusal leaves the output arrays, info and dst as they were.  Without dst, or with another handle as dst, nothing h
 *     holds for sicp_align changes -- correspondences, features, statistics, timers -- and a later sicp_align returns the bytes it
 *     returns on a handle that never made the call.  The slot holds no cloud: SICP_ERR_NOT_READY.  Refused before any device
 *     work with SICP_ERR_INVALID_ARGUMENT: a NULL handle or params; a `which` (or, with dst, a dst_which) outside SICP_SOURCE /
 *     SICP_TARGET; mean_k outside 0 .. 31; std_mul or radius negative or not finite; min_neighbors < 1 with the radius test on;
 *     n_drop or n_protect outside 0 .. SICP_FILTER_MAX_LABELS; a label in both lists; lists with a cloud without labels; dst on
 *     another device.
 * 10. Bit-reproducible: a function of the points, labels, mask and parameters only -- the same bytes on a handle of any mode (a
 *     SICP_MODE_SEMANTIC handle searches the cloud label by label and merges the lists by value), in either slot, before or
 *     after a sicp_align has laid the cloud out, for every launch shape.  No float atomics. */
#define SICP_FILTER_MAX_LABELS 16
typedef struct sicp_filter_params {
  int32_t mean_k;         /* 0 = statistical test off; 1 .. 31.  default 20 */
  int32_t min_neighbors;  /* other points needed inside radius; >= 1 when the radius test is on.  default 2 */
  double std_mul;         /* threshold = mean + std_mul * stddev; finite, >= 0.  default 2.0 */
  double radius;          /* 0 = radius test off (default); finite, >= 0 */
  int32_t n_drop;         /* 0 .. SICP_FILTER_MAX_LABELS.  default 0 */
  int32_t n_protect;      /* 0 .. SICP_FILTER_MAX_LABELS.  default 0 */
  uint32_t drop[SICP_FILTER_MAX_LABELS];     /* labels removed outright */
  uint32_t protect[SICP_FILTER_MAX_LABELS];  /* labels kept without being tested */
} sicp_filter_params;
typedef struct sicp_filter_info {
  int64_t n_points;       /* what the caller handed over (the size of keep, mean_dist, neighbors) */
  int64_t n_finite;
  int64_t n_tested;
  int64_t n_protected;
  int64_t n_kept;         /* protected points and tested points that passed */
  int64_t n_fail_stat;    /* tested points with m_i > threshold */
  int64_t n_fail_radius;  /* tested points with c_i < min_neighbors */
  double mean, stddev, threshold;  /* NaN when the statistical test is off */
  double t_total_ms;      /* host wall clock */
} sicp_filter_info;
int sicp_default_filter_params(sicp_filter_params* p);
int sicp_filter(sicp_handle h, int which, const sicp_filter_params* p, const uint8_t* mask /* n_points, nullable */,
                sicp_handle dst /* nullable */, int dst_which, uint8_t* keep /* n_points, nullable */,
                double* mean_dist /* n_points, nullable */, int32_t* neighbors /* n_points, nullable */,
                sicp_filter_info* info /* nullable */);

/* ---- deskewing a scan ---------------------------------------------------------------
 * A spinning lidar takes the points of one revolution over about 0.1 s while the sensor moves; every other entry point of this
 * header treats a scan as one rigid snapshot.  sicp_deskew moves every point of the cloud in a handle's slot to one common
 * instant, from a time stamp per point and a trajectory of pose knots (the first step of LOAM, KISS-ICP, CT-ICP); the result
 * can become a slot's cloud without the caller touching the points.  The handle may be in any mode.
 *  1. Trajectory.  Knot k says the sensor had pose knot_qt[7 k .. 7 k + 6] = [qx qy qz qw tx ty tz] (sensor -> some fixed frame) at
 *     knot_time[k].  Times are finite and strictly ascending, 2 <= n_knots <= SICP_DESKEW_MAX_KNOTS; poses are finite with
 *     | |q| - 1 | <= 1e-6 (the pose graph's rule) and are used normalised.  Point i was measured at times[i]; its output is the
 *     same physical point in the sensor frame of ref_qt (NULL: the last knot's pose): p' = ref^-1 T(times[i]) p.
 *  2. Relative knots, on the host.  K_k = ref^-1 T_k is formed once per call in double (quaternions scaled by 1 / |q|, the
 *     inverse and the product of the engine's SE(3)); then, k ascending from 1, the quaternion of K_k is negated where its dot
 *     product with that of K_(k-1) -- as stored -- is negative, so consecutive knots lie in one hemisphere.  knots_out returns
 *     exactly the table the kernel reads (the scheme of sicp_place_tables: the host's libm and composition order are not part of
 *     the bit-exact rule).
 *  3. Per point, on the device, in double; only + - * /, each rounded on its own, none contracted, no sin, cos or sqrt.  With
 *     t = times[i], kt = knot_time and K the table of rule 2:
 *       a = the largest index with kt[a] <= t, limited to 0 .. n_knots - 2;
 *       u = (t - kt[a]) / (kt[a+1] - kt[a]);  t < kt[0]: u = 0 (a = 0), counted in n_clamped_lo;  t > kt[n_knots-1]: u = 1
 *       (a = n_knots - 2), counted in n_clamped_hi;  w = 1 - u;
 *       c[j] = (w * K[a][j]) + (u * K[a+1][j]) for the seven numbers; (qx qy qz qw) = c[0..3] is not normalised;
 *       xx = qx qx, yy = qy qy, zz = qz qz, ww = qw qw;  s = ((xx + yy) + zz) + ww;  k = 2 / s;
 *       xy = qx qy, xz = qx qz, yz = qy qz, wx = qw qx, wy = qw qy, wz = qw qz;
 *       row 0 = [1 - k (yy + zz),  k (xy - wz),  k (xz + wy),  c[4]]
 *       row 1 = [k (xy + wz),  1 - k (xx + zz),  k (yz - wx),  c[5]]
 *       row 2 = [k (xz - wy),  k (yz + wx),  1 - k (xx + yy),  c[6]]
 *       p'[r] = (float)(((m0 (double)x + m1 (double)y) + m2 (double)z) + m3) of row r: the row rule of sicp_merge_clouds, one
 *       rounding to float.
 *     Why knots and not an exponential per point: device sin and cos are not the host libm's to the bit.  The price: between two
 *     knots whose rotations differ by an angle Theta the blend is off the geodesic by at most (sqrt(3) / 432) Theta^3 ~
 *     0.00401 Theta^3 rad (to leading order: times 1 + Theta^2 / 80), and the blended translation is off a screw motion's arc by
 *     the arc's sagitta at most, (L / 2) tan(Theta / 4) ~ L Theta / 8, L the chord length of the interval.  A car at 30 m/s turning at 1 rad/s over a 0.1 s scan with 33 knots: about 1e-10 rad and 4e-5 m.
 *     Choose n_knots by these two bounds.  (The hemisphere rule keeps s >= 1/2.)
 *  4. Classes of points.  A point with a coordinate that is not finite keeps its three floats bit for bit and is counted in
 *     neither n_finite nor n_moved.  A finite point whose time is not finite becomes three quiet NaNs (0x7fc00000) -- it leaves
 *     the index instead of staying skewed -- and is counted in n_bad_time.  Every other finite point is moved and counted in
 *     n_moved; the two clamp counts are among the moved points.  Labels are never touched.
 *  5. Outputs.  ox / oy / oz (nullable, n_points each) in caller order.  With dst (nullable; needs the same device; may be h
 *     with dst_which = which: the cloud is deskewed in place) all n_points output points with the cloud's labels, or without
 *     labels when the cloud has none, become the cloud of dst's slot exactly as sicp_set_cloud of those arrays would set it.  No
 *     moved point and dst: SICP_ERR_TOO_FEW_POINTS, nothing is written and dst keeps its cloud.
 *  6. Refused before any device work with SICP_ERR_INVALID_ARGUMENT, the outputs, info, knots_out and dst left as they were: a
 *     NULL handle, times, knot_time or knot_qt; a `which` (or, with dst, a dst_which) outside SICP_SOURCE / SICP_TARGET; n_knots
 *     out of range; knot times that are not finite or not strictly ascending; a knot pose or ref_qt that is not finite or not
 *     unit within 1e-6; dst on another device.  The slot holds no cloud: SICP_ERR_NOT_READY.  Without dst, or with another handle
 *     as dst, nothing h holds for sicp_align changes (rule 9 of sicp_filter).
 *  7. Bit-reproducible: a function of the points, times and knot table only -- the same bytes on a handle of any mode, in either
 *     slot, before or after a sicp_align has laid the cloud out, for every launch shape.  No float atomics; the four counters are
 *     integers from wave ballots and integer atomics.
 *  8. sicp_deskew_twist_knots (host only, no device): the constant-velocity model of KISS-ICP.  delta_qt is the sensor's motion
 *     over [t0, t1], T(t0)^-1 T(t1); knot k is exp(s_k log(delta)) at time t0 + s_k (t1 - t0), s_k = k / (n_knots - 1), with the
 *     engine's SE(3) exp and log (Sophus' formulas) -- held to a tolerance, not to the bit.  With these knots and ref_qt NULL the
 *     scan is expressed in the sensor frame at t1.  SICP_ERR_INVALID_ARGUMENT: a NULL pointer, a pose that is not finite or not
 *     unit within 1e-6, times that are not finite, t1 <= t0, n_knots out of range. */
#define SICP_DESKEW_MAX_KNOTS 1024
typedef struct sicp_deskew_info {
  int64_t n_points;       /* what the caller handed over (the size of times, ox, oy, oz) */
  int64_t n_finite;
  int64_t n_moved;        /* finite points with a finite time */
  int64_t n_bad_time;     /* finite points with a time that is not finite: written as NaN */
  int64_t n_clamped_lo;   /* moved points with a time below the first knot's */
  int64_t n_clamped_hi;   /* moved points with a time above the last knot's */
  double t_total_ms;      /* host wall clock */
} sicp_deskew_info;
int sicp_deskew(sicp_handle h, int which, const double* times /* n_points */, int32_t n_knots, const double* knot_time /* n_knots */,
                const double* knot_qt /* n_knots*7 */, const double ref_qt[7] /* NULL = the last knot's pose */,
                sicp_handle dst /* nullable */, int dst_which, float* ox, float* oy, float* oz /* n_points each, nullable */,
                double* knots_out /* n_knots*7, nullable */, sicp_deskew_info* info /* nullable */);
int sicp_deskew_twist_knots(const double delta_qt[7], double t0, double t1, int32_t n_knots, double* knot_time /* n_knots */,
                            double* knot_qt /* n_knots*7 */);

/* ---- range image and labels from it ---------------------------------------------------
 * The labels of a lidar scan come from a network that reads a range image (RangeNet++, SalsaNext, the SemanticKITTI tools).
 * sicp_range_image is the step before the network: the spherical projection of the cloud in a handle's slot, about
 * sensor_origin in the cloud's own frame, into height x width pixels.  sicp_range_labels is the step after it: the per-pixel
 * classes carried back onto every point by a vote among the nearest pixels of a window, the points that lost their pixel to a
 * nearer one included; the relabelled cloud can become a slot's cloud without leaving the library.  The image is also what depth
 * clustering, visibility tests and organised down-sampling work on.  The handle may be in any mode.
 *  Tables, on the host, once per call, in double with libm; sicp_range_tables returns exactly what the kernels read (the scheme
 *  of sicp_place_tables: the host's libm is not part of the bit-exact rule).  With W = width, H = height:
 *     cos_half[j], sin_half[j] = cos, sin of 2 pi j / W for j < W / 2;
 *     row_edge[r] = tan(a_r) |tan(a_r)| for r = 0 .. H, strictly descending: the signed squared tangent of the elevation a_r of
 *     the edge between rows r - 1 and r.  Without a beam table a_r = fov_up + (fov_down - fov_up) (r / H) (a_H = fov_down).  With
 *     beam_elevation[H] (radians, strictly descending, row 0 the top beam) the inner edges are the midpoints (b[r-1] + b[r]) / 2,
 *     a_0 = b[0] + (b[0] - b[1]) / 2 and a_H = b[H-1] - (b[H-2] - b[H-1]) / 2; for H = 1 the edges are fov_up and fov_down.
 *     A table entry that is not finite, or edges that do not strictly descend, are refused.
 *  The projection (fp contraction off, every operation rounded on its own; restated in numpy by tests/range_ref.py):
 *  1. Offset.  dx, dy, dz = the point minus sensor_origin in float (NULL: 0 0 0), as sicp_place_describe forms them.
 *  2. Range.  r2 = (dx dx + dy dy) + dz dz in float.  The point is KEPT iff (double)r2 >= min_range^2 and (double)r2 <
 *     max_range^2, the bounds squared on the host in double.
 *  3. Doubles.  X, Y, Z = (double)dx, dy, dz;  D = X X + Y Y (both products exact, one rounded sum);  Zs = Z |Z| (exact).
 *  4. Column.  The half plane of sicp_place_describe: lower = !(dy > 0 || (dy == 0 && dx > 0)), (xp, yp) = lower ? (-X, -Y) :
 *     (X, Y).  The sector inside it by one fixed bisection:
 *       lo = 0, hi = W / 2;  while (hi - lo > 1) { mid = (lo + hi) >> 1;  if (cos_half[mid] yp - sin_half[mid] xp >= 0.0) lo = mid;
 *       else hi = mid; }
 *     each product and the difference rounded on their own.  s = lo (+ W / 2 when lower); c = clockwise ? W - 1 - s : s;
 *     col = (c + col_shift) mod W.  The bisection, not monotonicity of the rounded predicate, is the definition.  Sector s holds
 *     the azimuths atan2(dy, dx) in [2 pi s / W, 2 pi (s + 1) / W) counted from +x through +y; clockwise = 1 with col_shift =
 *     W / 2 is the RangeNet++ column floor(0.5 (1 - yaw / pi) W) for every point away from a sector edge.
 *  5. Row.  The point is inside the field of view iff !(Zs > row_edge[0] D) and Zs >= row_edge[H] D, one rounded product each.
 *     Its row by the same kind of bisection over the inner edges:
 *       lo = 0, hi = H;  while (hi - lo > 1) { mid = (lo + hi) >> 1;  if (Zs < row_edge[mid] D) lo = mid; else hi = mid; }
 *     row = lo: a point exactly on an inner edge belongs to the row above it, both outer edges are inside.  A kept point
 *     outside the field of view is counted in n_outside_fov and has pixel -1.  A point on the sensor's vertical axis has D = 0
 *     and needs no special case: the comparisons put it outside (above or below), or, at the origin itself, inside.
 *  6. Winner.  A pixel's winner is its kept, in-view point with the smallest 64-bit key (bits(r2) << 32) | index, the index
 *     ascending with the caller's: the nearest point, equal ranges to the smaller caller index.  One unsigned 64-bit atomic
 *     minimum per point: an integer atomic, so the bytes depend neither on the launch shape nor on the other points' order.
 *  7. Outputs, every one nullable.  Per pixel, H W long, row-major: index (the winner's caller index, -1: empty), range_sq
 *     (r2, 0: empty; no root is taken on the device), x, y, z (the winner's coordinates as the caller gave them, 0: empty), label
 *     (the winner's label; 0 when empty or when the cloud has no labels), count (the kept, in-view points that fell into the
 *     pixel).  Per point, n_points long, caller order: pixel = row W + col or -1; visible = 1 iff the point won its pixel.  A
 *     point that is not finite has pixel -1, visible 0 and is counted in neither n_finite nor anything after it (rule 4 of
 *     sicp_deskew).  info: n_kept (rule 2), n_out_of_range = n_finite - n_kept, n_outside_fov, n_pixels_hit.
 *  The vote (sicp_range_labels): the call projects as above; pixel_label[H W] is the network's class per pixel, 0 = no class.
 *  Every kept, in-view point i with pixel (r, c) then:
 *  8. Candidates.  The occupied pixels of the window x window block centred on (r, c); columns wrap modulo W, rows outside
 *     0 .. H - 1 are absent; visited in ascending (window row, window column).
 *  9. Distance.  d2 = (ex ex + ey ey) + ez ez in float, e = the point minus the pixel's winner in float.  A candidate takes
 *     part iff (double)d2 < max_dist_sq, strictly (the comparison of sicp_evaluate).  This true 3-D distance deliberately
 *     replaces RangeNet++'s range difference under a Gaussian window weight: it needs no root and no exponential, and two
 *     points of equal range in neighbouring pixels can be metres apart only in range-image terms, never in d2.
 * 10. Neighbours.  The k participants with the smallest (bits(d2), visiting order).
 * 11. Vote.  Each neighbour whose pixel_label is not 0 gives one vote to that class; the class with the most votes wins, ties
 *     to the smallest label (the rule of sicp_merge_clouds).  out_label[i] = the winner, votes[i] = its vote count.
 * 12. No vote.  A point without any vote -- no neighbour of a class, not kept, outside the view -- keeps its own label (0 when
 *     the cloud has none) with votes = 0; a point that is not finite has out_label 0 (sicp_set_cloud dropped it with its
 *     label).  info: n_voted = the points with votes > 0, n_unvoted = n_points - n_voted.
 * 13. dst (nullable; needs the same device; may be h with dst_which = which: the cloud is relabelled in place).  All n_points
 *     points with out_label become the cloud of dst's slot exactly as sicp_set_cloud of those arrays would set it; a cloud that
 *     had no labels becomes a labelled one.  Everything is on the host before the slot lets go of its old cloud.  No finite
 *     point and dst: SICP_ERR_TOO_FEW_POINTS, dst keeps its cloud.
 * 14. Refused before any device work with SICP_ERR_INVALID_ARGUMENT, the outputs, info and dst left as they were, the reason in
 *     sicp_last_error: a NULL handle or params; a `which` (or, with dst, a dst_which) outside SICP_SOURCE / SICP_TARGET; width odd
 *     or outside 16 .. SICP_RANGE_MAX_WIDTH; height outside 1 .. SICP_RANGE_MAX_HEIGHT; fov_up <= fov_down, or either not
 *     strictly inside +-pi/2; min_range negative or not finite, max_range not finite or <= min_range; clockwise not 0 or 1;
 *     col_shift outside 0 .. W - 1; window even or outside 1 .. SICP_RANGE_MAX_WINDOW; k outside 1 .. SICP_RANGE_MAX_K;
 *     max_dist_sq negative or NaN; a beam table that is not finite or not strictly descending, or whose edges are not; a
 *     sensor_origin that is not finite; a NULL pixel_label (the vote); dst on another device.  The slot holds no cloud:
 *     SICP_ERR_NOT_READY.  Without dst, or with another handle as dst, nothing h holds for sicp_align changes (rule 9 of
 *     sicp_filter).  sicp_range_tables (host only, no handle) returns the status alone.
 * 15. Bit-reproducible: a function of the points, labels, parameters and tables only -- the same bytes on a handle of any mode,
 *     in either slot, before or after a sicp_align has laid the cloud out, for every launch shape.  No float atomics. */
#define SICP_RANGE_MAX_WIDTH 4096
#define SICP_RANGE_MAX_HEIGHT 256
#define SICP_RANGE_MAX_WINDOW 7
#define SICP_RANGE_MAX_K 16
typedef struct sicp_range_params {
  int32_t width;       /* W: even, 16 .. SICP_RANGE_MAX_WIDTH.  default 2048 */
  int32_t height;      /* H: 1 .. SICP_RANGE_MAX_HEIGHT.  default 64 */
  double fov_up;       /* radians, strictly inside +-pi/2, > fov_down.  default +3 degrees */
  double fov_down;     /* default -25 degrees */
  double min_range;    /* metres, finite, >= 0.  default 0.5 */
  double max_range;    /* finite, > min_range.  default 120 */
  int32_t clockwise;   /* 0: columns ascend with the azimuth; 1 (default): they descend */
  int32_t col_shift;   /* 0 .. W - 1.  default W / 2 = 1024 (with clockwise: the RangeNet++ column) */
  int32_t window;      /* the vote: S odd, 1 .. SICP_RANGE_MAX_WINDOW.  default 5 */
  int32_t k;           /* the vote: 1 .. SICP_RANGE_MAX_K.  default 5 */
  double max_dist_sq;  /* the vote: >= 0 (infinity allowed).  default 1.0 */
} sicp_range_params;
typedef struct sicp_range_info {
  int64_t n_points;        /* what the caller handed over (the size of pixel, visible, out_label, votes) */
  int64_t n_finite;
  int64_t n_kept;          /* finite points inside [min_range, max_range) */
  int64_t n_out_of_range;  /* n_finite - n_kept */
  int64_t n_outside_fov;   /* kept points outside the field of view */
  int64_t n_pixels_hit;    /* pixels with a winner */
  int64_t n_voted;         /* sicp_range_labels: points with votes > 0; sicp_range_image: 0 */
  int64_t n_unvoted;       /* sicp_range_labels: n_points - n_voted; sicp_range_image: 0 */
  double t_total_ms;       /* host wall clock */
} sicp_range_info;
int sicp_default_range_params(sicp_range_params* p);
int sicp_range_tables(const sicp_range_params* p, const double* beam_elevation /* height, nullable */,
                      double* cos_half /* width/2 */, double* sin_half /* width/2 */, double* row_edge /* height+1; all nullable */);
int sicp_range_image(sicp_handle h, int which, const sicp_range_params* p, const double* beam_elevation /* height, nullable */,
                     const float sensor_origin[3] /* NULL = 0 0 0 */, int32_t* index, float* range_sq, float* x, float* y, float* z,
                     uint32_t* label, uint32_t* count /* height*width each, nullable */, int32_t* pixel, uint8_t* visible
                     /* n_points each, nullable */, sicp_range_info* info /* nullable */);
int sicp_range_labels(sicp_handle h, int which, const sicp_range_params* p, const double* beam_elevation /* height, nullable */,
                      const float sensor_origin[3] /* NULL = 0 0 0 */, const uint32_t* pixel_label /* height*width */,
                      sicp_handle dst /* nullable */, int dst_which, uint32_t* out_label, uint8_t* votes
                      /* n_points each, nullable */, sicp_range_info* info /* nullable */);

/* ---- camera: depth frames and image labels -------------------------------------------
 * The camera's side of what the range image does for a lidar.  sicp_camera_unproject turns a depth frame (and a label image)
 * into a slot's cloud -- the organised 640 x 480 clouds of RGB-D datasets, invalid pixels included.  sicp_camera_image projects
 * the cloud in a handle's slot through a calibrated pinhole camera into height x width pixels, each won by its nearest point.
 * sicp_camera_labels carries an image network's per-pixel classes onto the points the camera sees: a lidar point behind a
 * parked car projects into the car's pixels, so a point keeps its own label when a nearer surface covers its window.  The
 * handle may be in any mode.
 *  Calibration: OpenCV's convention -- the centre of pixel (row r, column c) is at (u, v) = (c, r); fx fy cx cy in pixels;
 *  k1 k2 p1 p2 k3 the Brown-Conrady coefficients in OpenCV's order.  camera_qt[7] = [qx qy qz qw tx ty tz] is the camera's pose
 *  in the cloud's frame (camera -> cloud; x right, y down, z forward); NULL: the identity, through the same arithmetic.
 *  Matrices, on the host, once per call, in double; sicp_camera_matrices returns exactly what the kernels read (the scheme of
 *  sicp_range_tables).  cam_to_cloud[12] = the 3 x 4 matrix of camera_qt as the engine forms a pose matrix (rule 2 of
 *  sicp_merge_clouds: no normalisation), rows of (R | t).  cloud_to_cam[12] = (R^T | t') with t'_i = -((R_0i t_0 + R_1i t_1) +
 *  R_2i t_2): the inverse for a unit quaternion.
 *  The projection, shared by sicp_camera_image and sicp_camera_labels, per finite point f of the cloud in the caller's order (fp
 *  contraction off, everything in double, every operation rounded on its own; restated in numpy by tests/camera_ref.py):
 *  1. Camera frame.  Xc, Yc, Zc = ((m0 x + m1 y) + m2 z) + m3 per row of cloud_to_cam, x y z widened from float: rule 2 of
 *     sicp_merge_clouds without the final rounding.
 *  2. Depth gate.  The point is KEPT iff Zc >= min_depth && Zc < max_depth.
 *  3. Normalised coordinates.  xn = Xc / Zc, yn = Yc / Zc;  a = xn xn, b = yn yn, c = xn yn;  r2 = a + b.  A kept point with
 *     !(r2 <= max_tan_sq) is outside the view: far off the axis the distortion polynomial folds back into the image.
 *  4. Distortion.  rad = 1 + r2 (k1 + r2 (k2 + r2 k3)) by Horner;  xd = xn rad + ((2 p1) c + p2 (r2 + 2 a));
 *     yd = yn rad + (p1 (r2 + 2 b) + (2 p2) c).
 *  5. Pixel.  u = fx xd + cx, v = fy yd + cy;  cf = floor(u + 0.5), rf = floor(v + 0.5).  The point is inside the image iff
 *     cf >= 0 && cf <= W - 1 && rf >= 0 && rf <= H - 1, compared as doubles (a NaN is outside);  pixel = rf W + cf.
 *  6. Winner.  A pixel's winner is its kept, in-image point with the smallest 64-bit key (bits((float)Zc) << 32) | f: the
 *     nearest point, equal float depths to the smaller caller index.  One unsigned 64-bit atomic minimum per point.
 *  Outputs of sicp_camera_image, every one nullable.  Per pixel, H W long, row-major: index (the winner's caller index, -1:
 *  empty), depth (the winner's (float)Zc, 0: empty), x, y, z (the winner as the caller gave it, 0: empty), label (the winner's;
 *  0 when empty or when the cloud has no labels), count (the kept, in-image points of the pixel).  Per point, n_points long,
 *  caller order: pixel (rf W + cf or -1), u, v ((float)u, (float)v; NaN unless the point is kept and inside the view of rule 3),
 *  visible (1 iff the point won its pixel).  A point that is not finite has -1 / NaN / 0 and is counted in nothing after
 *  n_finite.  info: n_kept (rule 2), n_outside (kept, no pixel), n_pixels_hit.
 *  sicp_camera_labels: the call projects as above; pixel_label[H W] is the network's class per pixel, 0 = no class.  Every kept,
 *  in-image point with zf = (float)Zc and pixel (r, c) then:
 *  7. Front depth.  zmin = the smallest winner depth over the occupied pixels of the window x window block centred on (r, c),
 *     truncated at the image's border (no wrap).  The point's own pixel always has a winner.
 *  8. Occlusion.  The point is occluded iff (double)zf - (double)zmin > occlusion_abs + occlusion_rel (double)zmin, strictly.
 *  9. Label.  Not occluded and pixel_label[pixel] != 0: out_label = pixel_label[pixel], state = 1.  Occluded: state = 2.  Visible
 *     with class 0: state = 3.  No pixel, for any reason: state = 0.  In states 0, 2 and 3 the point keeps its own label (0 when
 *     the cloud has none).  A point that is not finite has out_label 0 and state 0 (rule 12 of sicp_range_labels).  info:
 *     n_labelled, n_occluded, n_unclassed = the points of states 1, 2, 3.
 * 10. dst: exactly rule 13 of sicp_range_labels, in place included; a cloud without labels becomes a labelled one.  Because a
 *     point the camera does not see keeps its label, a rig of N cameras is N calls with dst = h.
 *  sicp_camera_unproject: exactly one of depth_u16 / depth_f32 [H W]; label (nullable) uint32 [H W].  h gives the device, the
 *  stream and the scratch; it needs no cloud, and dst may be h.  Per pixel (r, c):
 * 11. Depth.  Z = (double)d16 * depth_scale, or (double)df.  The pixel is valid iff Z is finite and Z >= min_depth &&
 *     Z < max_depth (a uint16 of 0 is invalid).
 * 12. Ray.  xd = ((double)c - cx) / fx, yd = ((double)r - cy) / fy;  x = xd, y = yd;  then exactly undistort_iterations times,
 *     with rule 4's rad, tx = (2 p1) c + p2 (r2 + 2 a) and ty = p1 (r2 + 2 b) + (2 p2) c formed from the current x, y:
 *     x = (xd - tx) / rad, y = (yd - ty) / rad.  The fixed count is the definition (OpenCV's undistortPoints runs 5; 20 brings
 *     wide lenses below 1e-3 px); with zero coefficients every pass is exact.
 * 13. Point.  Pc = (x Z, y Z, Z); then cam_to_cloud as rule 2 of sicp_merge_clouds applies a pose, one rounding to float per
 *     coordinate.  An invalid pixel gives NaN NaN NaN; valid[p] = 1 / 0; info: n_valid.
 * 14. dst (nullable; the same device).  The H W points with `label` become the cloud of dst's slot exactly as sicp_set_cloud of
 *     those arrays would set it: n_points = H W as in an organised cloud, the NaN pixels left out of the index; without `label`
 *     the cloud has none.  No valid pixel and dst: SICP_ERR_TOO_FEW_POINTS, dst keeps its cloud.
 * 15. Refused before any device work with SICP_ERR_INVALID_ARGUMENT, the outputs, info and dst left as they were, the reason in
 *     sicp_last_error: a NULL handle or params; a `which` (or, with dst, a dst_which) outside SICP_SOURCE / SICP_TARGET; width or
 *     height outside 8 .. SICP_CAMERA_MAX_WIDTH / _HEIGHT; fx fy cx cy or a coefficient not finite, fx or fy <= 0; min_depth
 *     <= 0 or NaN, max_depth not finite or <= min_depth; max_tan_sq or depth_scale <= 0 or NaN; undistort_iterations outside
 *     0 .. 64; window even or outside 1 .. SICP_CAMERA_MAX_WINDOW; occlusion_abs or occlusion_rel negative or NaN; a camera_qt
 *     that is not finite or whose quaternion is zero; a NULL pixel_label; both or neither depth pointer; dst on another device.
 *     The slot holds no cloud: SICP_ERR_NOT_READY.  Without dst, or with another handle as dst, nothing h holds for sicp_align
 *     changes.  sicp_camera_matrices (host only, no handle) returns the status alone.  SICP_ERR_OUT_OF_MEMORY (the arena
 *     refused, sicp_set_memory_limit applies) is a status: refused for the call's scratch, the outputs, info and dst are left as
 *     they were; refused for dst's own device buffers, the outputs and info are left as they were and dst's slot is what
 *     sicp_set_cloud of the same arrays leaves under the same limit.  The handles stay usable.
 * 16. Bit-reproducible: a function of the points, labels, images, parameters and matrices only -- the same bytes on a handle of
 *     any mode, in either slot, before or after a sicp_align, for every launch shape.  No float atomics. */
#define SICP_CAMERA_MAX_WIDTH 4096
#define SICP_CAMERA_MAX_HEIGHT 4096
#define SICP_CAMERA_MAX_WINDOW 15
typedef struct sicp_camera_params {
  int32_t width;                 /* W: 8 .. SICP_CAMERA_MAX_WIDTH.  default 640 */
  int32_t height;                /* H: 8 .. SICP_CAMERA_MAX_HEIGHT.  default 480 */
  double fx, fy, cx, cy;         /* finite, fx fy > 0.  default 525 525 319.5 239.5 */
  double k1, k2, p1, p2, k3;     /* Brown-Conrady, finite.  default 0 */
  double min_depth;              /* > 0.  default 0.3 */
  double max_depth;              /* finite, > min_depth.  default 100 */
  double max_tan_sq;             /* > 0: the largest xn^2 + yn^2 the distortion is trusted at.  default 4.0 */
  double depth_scale;            /* > 0: metres per uint16 unit.  default 0.001 */
  int32_t undistort_iterations;  /* 0 .. 64.  default 20 */
  int32_t window;                /* odd, 1 .. SICP_CAMERA_MAX_WINDOW.  default 5 */
  double occlusion_abs;          /* >= 0, metres.  default 0.3 */
  double occlusion_rel;          /* >= 0, per metre of front depth.  default 0.02 */
} sicp_camera_params;
typedef struct sicp_camera_info {
  int64_t n_points;      /* what the caller handed over; sicp_camera_unproject: H W */
  int64_t n_finite;
  int64_t n_kept;        /* finite points inside [min_depth, max_depth) */
  int64_t n_outside;     /* kept points without a pixel */
  int64_t n_pixels_hit;  /* pixels with a winner */
  int64_t n_labelled;    /* sicp_camera_labels: state 1 */
  int64_t n_occluded;    /* state 2 */
  int64_t n_unclassed;   /* state 3 */
  int64_t n_valid;       /* sicp_camera_unproject: valid pixels */
  double t_total_ms;     /* host wall clock */
} sicp_camera_info;
int sicp_default_camera_params(sicp_camera_params* p);
int sicp_camera_matrices(const double camera_qt[7] /* NULL = identity */, double cam_to_cloud[12], double cloud_to_cam[12] /* nullable */);
int sicp_camera_image(sicp_handle h, int which, const sicp_camera_params* p, const double camera_qt[7] /* NULL = identity */,
                      int32_t* index, float* depth, float* x, float* y, float* z, uint32_t* label, uint32_t* count
                      /* height*width each, nullable */, int32_t* pixel, float* u, float* v, uint8_t* visible
                      /* n_points each, nullable */, sicp_camera_info* info /* nullable */);
int sicp_camera_labels(sicp_handle h, int which, const sicp_camera_params* p, const double camera_qt[7] /* NULL = identity */,
                       const uint32_t* pixel_label /* height*width */, sicp_handle dst /* nullable */, int dst_which,
                       uint32_t* out_label, uint8_t* state /* n_points each, nullable */, sicp_camera_info* info /* nullable */);
int sicp_camera_unproject(sicp_handle h, const sicp_camera_params* p, const double camera_qt[7] /* NULL = identity */,
                          const uint16_t* depth_u16, const float* depth_f32 /* height*width, exactly one */,
                          const uint32_t* label /* height*width, nullable */, sicp_handle dst /* nullable */, int dst_which,
                          float* x, float* y, float* z, uint8_t* valid /* height*width each, nullable */,
                          sicp_camera_info* info /* nullable */);

/* ---- planes of a cloud -------------------------------------------------------------
 * RANSAC plane extraction of the cloud in a handle's slot (pcl::SACSegmentation with SACMODEL_PLANE or, with an axis,
 * SACMODEL_PERPENDICULAR_PLANE; Open3D's segment_plane): up to max_planes planes, one per round, each from a fixed number of
 * three-point hypotheses scored over every remaining candidate.  plane_id -> a mask -> sicp_filter(mask, dst) -> sicp_cluster
 * is "remove the ground, then cluster".  The handle may be in any mode.  All arithmetic below is float64 on the points'
 * float coordinates widened exactly; every operation is rounded on its own, none contracted; (a b + c d) + e f is evaluated
 * in that order.
 *  1. Candidates.  A point is a candidate when it is finite, mask is NULL or mask[i] != 0, and its label is not one of
 *     ignore[0 .. n_ignore).  A cloud set without labels is accepted only with n_ignore = 0 (rule 1 of sicp_filter).  Round
 *     r = 0, 1, ... works on the candidates no earlier round has taken, in ascending caller index: cand[0 .. m_r).  The result
 *     does not depend on the handle's mode, slot or device layout.
 *  2. Hypotheses.  One SplitMix64 stream seeded with `seed`: draw number k (from 0) is the output z of the state
 *     seed + (k + 1) * 0x9E3779B97F4A7C15 (mod 2^64), z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) *
 *     0x94D049BB133111EB, z ^ z >> 31.  Draw 3 (r H + h) + s gives sample s of hypothesis h of round r as the index
 *     min(floor((double)m_r * u), m_r - 1) into cand, u = (double)(z >> 11) * 2^-53.  With a, b, c the three points:
 *     e1 = b - a, e2 = c - a, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), nn = (nx nx + ny ny) + nz nz.
 *     The hypothesis is invalid when two of its sample indices coincide or nn > 0 is false; with an axis also when
 *     na na >= ((min_cos min_cos) nn) aa is false, na = (nx ax + ny ay) + nz az, aa = (ax ax + ay ay) + az az.  No sqrt, no
 *     division, no trigonometry.
 *  3. Score.  Candidate p is an inlier of (a, n) iff e e <= (t t) nn, d = p - a, e = (nx dx + ny dy) + nz dz,
 *     t = distance_threshold.  A hypothesis' score is its inlier count over cand; the winner is the valid hypothesis with the
 *     largest score, ties to the smallest h.  The call ends, with SICP_OK and the planes found so far, when m_r < 3 (the round is
 *     not scored), when no hypothesis is valid or the winner's score is < min_inliers (the round is scored: it counts in
 *     `rounds` and its invalid hypotheses in n_invalid_hypotheses), or after max_planes planes.
 *  4. refine = 0.  The plane's members are the winner's inliers.  coeff = (u, D): u = n / sqrt(nn) component by component,
 *     D = -((ux ax + uy ay) + uz az), then oriented: with an axis all four are negated when s = (ux axis_x + uy axis_y) +
 *     uz axis_z < 0; without an axis, or when s == 0, when the first non-zero of (D, uz, uy, ux) is negative.
 *  5. refine = 1.  Over the winner's inliers: S = the sums of x, y, z; g = S / (double)count; Q = the sums of the six products
 *     dx dx, dy dx, dy dy, dz dx, dz dy, dz dz of d = p - g.  Every sum here and below is the sum over the perfect binary tree on
 *     the caller's indices (rule 3 of sicp_filter: absent entries are +0.0), and +0.0 is added to the result once (a zero sum
 *     is +0.0).  Q, undivided, goes through the cyclic Jacobi of the covariance estimation (sweeps over (0,1), (0,2), (1,2), at
 *     most 30, stopped when off <= 1e-300 or off <= 1e-34 dia, off and dia the sums of the squared off-diagonal and diagonal
 *     entries); the normal u is the eigenvector column of smallest |eigenvalue|, at ties the last such column.  D = -((ux gx +
 *     uy gy) + uz gz); coeff = (u, D) oriented as in 4.  Then the members are re-selected once among the round's candidates by
 *     rule 3's test with a = g, n = u, nn = (ux ux + uy uy) + uz uz (what PCL does after optimizeCoefficients).
 *  6. Outputs.  plane_id[i] (nullable, n_points long, caller order): the round that took the point, -1 otherwise.  Per plane:
 *     coeff (4), count = the final members, hyp_index = the winner's h, hyp_count = its score, centroid (3) = the tree sums of
 *     the final members' x, y, z / (double)count, rms = sqrt(max(0, E / nn) / (double)count), E = the tree sum of e e over the
 *     final members with a, n, nn the model that selected them (the winner with refine = 0, else (g, u)).  The table arrays are
 *     nullable and hold `capacity` rows; capacity follows rule 6 of sicp_cluster (a non-NULL table array with capacity < n_planes:
 *     SICP_ERR_INVALID_ARGUMENT with info written and nothing else).  n_planes <= max_planes: capacity = max_planes always suffices.
 *  7. Fewer than 3 candidates: SICP_ERR_TOO_FEW_POINTS.  The slot holds no cloud: SICP_ERR_NOT_READY.  Refused before any device
 *     work with SICP_ERR_INVALID_ARGUMENT (rule 9 of sicp_filter): a NULL handle or params; a `which` outside SICP_SOURCE /
 *     SICP_TARGET; distance_threshold not finite or <= 0; an axis component that is not finite; an axis with min_cos outside
 *     (0, 1]; min_cos != 0 without an axis; num_hypotheses outside 1 .. SICP_PLANE_MAX_HYPOTHESES; max_planes outside 1 ..
 *     SICP_PLANE_MAX_PLANES; min_inliers < 3; refine not 0 or 1; n_ignore outside 0 .. SICP_PLANE_MAX_IGNORE; ignore with a cloud
 *     without labels; capacity < 0.  Every refusal leaves the outputs and info as they were.  Nothing on the handle changes: a
 *     later sicp_align returns the bytes it returns on a handle that never made the call.
 *  8. Bit-reproducible: a function of the points, labels, mask and parameters only -- the same bytes from run to run, on a handle
 *     of any mode, in either slot, before or after a sicp_align has laid the cloud out, for every launch shape.  Integer counts,
 *     sums of fixed order, no float atomics. */
#define SICP_PLANE_MAX_HYPOTHESES 4096
#define SICP_PLANE_MAX_PLANES 16
#define SICP_PLANE_MAX_IGNORE 16
typedef struct sicp_plane_params {
  double distance_threshold;  /* t > 0, finite.  default 0.2 */
  double axis[3];             /* all 0 (default): no constraint; otherwise finite, not all 0 */
  double min_cos;             /* with axis: in (0, 1]; |cos| of the largest angle between normal and axis.  default 0 */
  uint64_t seed;              /* default 1 */
  int32_t num_hypotheses;     /* H in 1 .. SICP_PLANE_MAX_HYPOTHESES.  default 1024 */
  int32_t max_planes;         /* 1 .. SICP_PLANE_MAX_PLANES.  default 1 */
  int32_t min_inliers;        /* >= 3.  default 100 */
  int32_t refine;             /* 1 (default): least-squares refit and re-selection; 0: the winning hypothesis as it is */
  int32_t n_ignore;           /* 0 .. SICP_PLANE_MAX_IGNORE.  default 0 */
  uint32_t ignore[SICP_PLANE_MAX_IGNORE];
} sicp_plane_params;
typedef struct sicp_plane_info {
  int64_t n_points;              /* what the caller handed over (the size of plane_id) */
  int64_t n_finite;
  int64_t n_candidates;          /* rule 1 */
  int64_t n_assigned;            /* points with plane_id >= 0 */
  int32_t n_planes;
  int32_t rounds;                /* rounds scored: n_planes, or one more when the last one found no plane */
  int64_t n_invalid_hypotheses;  /* over the rounds scored */
  double t_total_ms;             /* host wall clock */
} sicp_plane_info;
int sicp_default_plane_params(sicp_plane_params* p);
int sicp_segment_planes(sicp_handle h, int which, const sicp_plane_params* p, const uint8_t* mask /* n_points, nullable */,
                        int32_t* plane_id /* n_points, nullable */, int32_t capacity, double* coeff /* 4 per plane */,
                        int32_t* count, int32_t* hyp_index, int32_t* hyp_count, double* centroid /* 3 per plane */,
                        double* rms /* all nullable */, sicp_plane_info* info /* nullable */);

/* ---- ground of a cloud -------------------------------------------------------------
 * Piecewise-planar ground of the cloud in a handle's slot on a polar grid around the sensor (Zermas et al. 2017, "ground plane
 * fitting"; Patchwork, Patchwork++): R rings x S sectors of cells, one small plane per cell, fitted from the cell's lowest
 * points upward, and for every point its height above the local ground.  A ramp, a crowned road or a kerb that leave the one
 * plane of sicp_segment_planes(axis = up) stay ground here.  z is up; the sensor looks along its own axes (no pose).  The handle
 * may be in any mode; nothing on it changes unless dst is given.  All arithmetic below is float64 on the points' float
 * coordinates widened exactly; every operation is rounded on its own, none contracted; (a b + c d) + e f is evaluated in that
 * order; no atan2 and no sqrt but the Jacobi's.
 *  1. Frame and candidates.  d = p - sensor_origin per axis (NULL: 0 0 0).  r2 = dx dx + dy dy.  A point is `inside` when it
 *     is finite and edge2[0] <= r2 < edge2[R].  An inside point is a candidate when mask is NULL or mask[i] != 0, its label is
 *     not one of ignore[0 .. n_ignore) (rule 1 of sicp_segment_planes: a cloud without labels only with n_ignore = 0), and
 *     dz >= -(sensor_height + max_below), the bound formed once (a sum, a negation).  An inside point that fails only this last
 *     test -- a multipath return under the road -- is counted in info.n_below.
 *  2. Cell.  Tables formed once on the host in double with libm (sicp_ground_tables hands back what the kernel reads):
 *     edge[i] = ring_edge[i] when the caller gives a table of R + 1 entries, else min_range + (double)i * ((max_range -
 *     min_range) / (double)R), i = 0..R; edge2[i] = edge[i] * edge[i]; cos_half[j] = cos(a), sin_half[j] = sin(a), a = (double)j *
 *     (6.283185307179586 / (double)S), j = 0..S/2-1 (rule 2 of sicp_place_*).  ring = the number of i in 1..R-1 with r2 >=
 *     edge2[i].  sector by rule 3 of sicp_place_* on the doubles dx, dy: lower = !(dy > 0 || (dy == 0 && dx > 0)); (x', y') =
 *     lower ? (-dx, -dy) : (dx, dy); sector = the number of j in 1..S/2-1 with cos_half[j]*y' - sin_half[j]*x' >= 0, plus S/2
 *     when lower.  cell = ring * S + sector.  R in 1..64, S even in 4..256.
 *  3. Order inside a cell.  The candidates, taken in ascending caller index, go through one stable sort by the key
 *     (cell << 32) | ordered_bits(z): z the float32 as stored (not dz), ordered_bits(b) = b ^ 0x80000000 for a clear sign bit
 *     and ~b otherwise, so -0.0 comes before +0.0.  A cell's members are one segment m_0 .. m_(m-1): lowest z first, ties by
 *     caller index.
 *  4. Seeds.  L = min(n_lpr, m); lpr = (((+0.0 + dz(m_0)) + dz(m_1)) + ...) / (double)L over the first L members; the seed
 *     set is the members with dz < lpr + th_seeds (the sum formed once).
 *  5. Fit, n_iter times, the first on the seed set.  A sum over a set is formed so: lane l of 64 adds, from +0.0, the terms of
 *     the members m_j of the set with j mod 64 == l, in ascending j; then T_0[l] = the lane's sum, T_(k+1)[l] = T_k[l] +
 *     T_k[l xor 2^k] for k = 0..5, and the sum is T_6[0] (pairs at distance 1, 2, 4, .. 32: the tree of sicp_map_extract_fused's
 *     confidence).  A set with count < min_points ends the cell with status TOO_FEW.  S = the sums of dx, dy, dz; g = S /
 *     (double)count; Q = the sums of the six products ex ex, ey ex, ey ey, ez ex, ez ey, ez ez of e = d - g.  Q, undivided, goes
 *     through the cyclic Jacobi of rule 5 of sicp_segment_planes; u is the eigenvector column of smallest |eigenvalue| (at ties
 *     the last such column), lambda_min that column's diagonal entry as the Jacobi left it; u is negated, all three components,
 *     when uz < 0.  The next set is ALL members of the cell with (ux ex + uy ey) + uz ez < th_dist, e = d - g: signed, points
 *     under the plane are ground.  The set selected by the last fit is the cell's ground; the model reported is the last fit:
 *     u, g, lambda_min and n_fit = the count of the set it was fitted to.
 *  6. Cell tests on the last fit, in this order: `uz >= min_cos` false: NOT_UPRIGHT; ring < elevation_rings and gz >=
 *     -sensor_height + max_elevation (the bound formed once): TOO_HIGH (a hood, a roof, a loading ramp beside the sensor);
 *     max_thickness > 0 and lambda_min > (max_thickness max_thickness) (double)n_fit: TOO_THICK; otherwise GROUND.  A cell
 *     without candidates is EMPTY.  Only GROUND cells have ground points and a model.
 *  7. Height, for every inside point, candidate or not: with the model of its own cell if that is GROUND, otherwise of the
 *     first GROUND cell of the same sector at ring - 1, ring - 2, .. 0: height = (ux ex + uy ey) + uz ez, e = d - g.  No such
 *     cell, or a point that is not inside: NaN.
 *  8. Outputs (sicp_ground_out; every array nullable).  Per point, caller order: ground (1: a ground point), cell (the cell
 *     of an inside point, candidate or not; -1 otherwise), height.  Per cell, R*S rows: status, n_members (candidates), n_ground,
 *     n_fit, normal = u, centroid = g + sensor_origin, lambda_min, lpr; a row that is not GROUND has n_ground = n_fit = 0 and NaN
 *     in normal, centroid and lambda_min; lpr is NaN only in an EMPTY row.  Capacity follows rule 6 of sicp_segment_planes with
 *     R*S for n_planes (a non-NULL cell array with capacity < R*S: SICP_ERR_INVALID_ARGUMENT with info written and nothing
 *     else, dst included).  select: 0 nothing, 1 the finite points that are not ground (non-candidates and points outside the
 *     rings among them), 2 the ground points; with dst they become dst's slot dst_which exactly as sicp_set_cloud of them, in
 *     caller order and with their labels, would make it (the route of sicp_filter(mask, dst)); dst may be h itself.  An empty
 *     selection: SICP_ERR_TOO_FEW_POINTS, dst keeps its cloud, outputs and info untouched.
 *  9. No candidate at all: SICP_OK, every cell EMPTY.  The slot holds no cloud: SICP_ERR_NOT_READY.  Refused before any device
 *     work with SICP_ERR_INVALID_ARGUMENT, outputs and info left as they were: a NULL handle or params; a `which` (or, with
 *     dst, dst_which) outside SICP_SOURCE / SICP_TARGET; a sensor_origin component or a double of params that is not finite;
 *     min_range < 0; max_range <= min_range; a ring_edge table with a non-finite entry, ring_edge[0] < 0 or ring_edge[i + 1] <=
 *     ring_edge[i]; n_rings outside 1..64; n_sectors outside 4..256 or odd; n_lpr outside 1..64; n_iter outside 1..8;
 *     min_points < 3; min_cos outside (0, 1]; th_dist or th_seeds not > 0; max_thickness < 0; elevation_rings outside
 *     0..n_rings; n_ignore outside 0..SICP_GROUND_MAX_IGNORE; ignore with a cloud without labels; select outside 0..2;
 *     select != 0 without dst (dst with select = 0 is left alone); dst on another device; capacity < 0.  An out-of-memory answer
 *     (sicp_set_memory_limit applies to the call's scratch) leaves both handles as they were.
 * 10. Bit-reproducible: a function of the points, labels, mask, origin and parameters only, on a handle of any mode, in either
 *     slot, before or after a sicp_align has laid the cloud out, for every launch shape: one wave owns a cell, integer counts,
 *     sums of fixed order, no float atomics.
 * The defaults are Patchwork's published KITTI values where it has them; nobody has tuned them on this engine. */
#define SICP_GROUND_MAX_RINGS 64
#define SICP_GROUND_MAX_SECTORS 256
#define SICP_GROUND_MAX_IGNORE 16
#define SICP_GROUND_EMPTY 0
#define SICP_GROUND_GROUND 1
#define SICP_GROUND_TOO_FEW 2
#define SICP_GROUND_NOT_UPRIGHT 3
#define SICP_GROUND_TOO_HIGH 4
#define SICP_GROUND_TOO_THICK 5
typedef struct sicp_ground_params {
  double min_range;        /* >= 0.  default 2.7 */
  double max_range;        /* > min_range.  default 80 */
  double sensor_height;    /* of the sensor above the road.  default 1.73 */
  double max_below;        /* candidates reach this far under the road.  default 1.0 */
  double th_seeds;         /* > 0.  default 0.5 */
  double th_dist;          /* > 0.  default 0.2 */
  double min_cos;          /* in (0, 1].  default 0.707 */
  double max_elevation;    /* default 0.5 */
  double max_thickness;    /* >= 0; 0 (default): the test is off */
  int32_t n_rings;         /* R in 1 .. SICP_GROUND_MAX_RINGS.  default 16 */
  int32_t n_sectors;       /* S even in 4 .. SICP_GROUND_MAX_SECTORS.  default 32 */
  int32_t n_lpr;           /* 1 .. 64.  default 20 */
  int32_t n_iter;          /* 1 .. 8.  default 3 */
  int32_t min_points;      /* >= 3.  default 10 */
  int32_t elevation_rings; /* 0 .. R.  default 4 */
  int32_t select;          /* what goes to dst: 0 (default) nothing, 1 the non-ground points, 2 the ground points */
  int32_t n_ignore;        /* 0 .. SICP_GROUND_MAX_IGNORE.  default 0 */
  uint32_t ignore[SICP_GROUND_MAX_IGNORE];
} sicp_ground_params;
typedef struct sicp_ground_out {
  uint8_t* ground;         /* n_points */
  int32_t* cell;           /* n_points */
  double* height;          /* n_points */
  int32_t capacity;        /* rows the cell arrays below hold */
  int32_t pad_;
  uint8_t* status;
  int32_t* n_members;
  int32_t* n_ground;
  int32_t* n_fit;
  double* normal;          /* 3 per cell */
  double* centroid;        /* 3 per cell */
  double* lambda_min;
  double* lpr;
} sicp_ground_out;
typedef struct sicp_ground_info {
  int64_t n_points;        /* what the caller handed over */
  int64_t n_finite;
  int64_t n_candidates;    /* rule 1 */
  int64_t n_below;         /* rule 1 */
  int64_t n_ground;
  int64_t n_selected;      /* points handed to dst; 0 with select = 0 */
  int32_t n_cells;         /* R*S */
  int32_t cells[6];        /* cells per status, indexed by SICP_GROUND_EMPTY .. SICP_GROUND_TOO_THICK */
  int32_t pad_;
  double t_total_ms;       /* host wall clock */
} sicp_ground_info;
int sicp_default_ground_params(sicp_ground_params* p);
/* rule 2's tables as the kernel reads them: cos_half, sin_half [S/2], edge2 [R+1], all nullable; host only */
int sicp_ground_tables(const sicp_ground_params* p, const double* ring_edge /* R+1, nullable */, double* cos_half, double* sin_half,
                       double* edge2);
int sicp_segment_ground(sicp_handle h, int which, const sicp_ground_params* p, const uint8_t* mask /* n_points, nullable */,
                        const double sensor_origin[3] /* nullable */, const double* ring_edge /* R+1, nullable */,
                        sicp_handle dst /* nullable */, int dst_which, const sicp_ground_out* out /* nullable */,
                        sicp_ground_info* info /* nullable */);

/* ---- a persistent voxel map ---------------------------------------------------
 * The map of scan-to-map odometry as an object that lives on the device between calls: per occupied voxel of the absolute
 * grid of the merge above (v = floor(p * (1.0f / (float)leaf_size)), |v| < 2^20) its 63-bit key (three biased 21-bit
 * coordinates, z highest), the float64 sums of its points, their number, and -- with num_classes > 0 -- a histogram of their
 * labels 0..num_classes.  Integrating scans 1..n and extracting with the defaults gives the merge of parts 1..n under the same
 * poses, leaf, centre and range bit for bit in x, y, z, count and label (every label <= num_classes), n_out and
 * max_voxel_points included: a voxel's sums continue from the stored value with the new points in ascending point index, one
 * add per point, which is the merge's own order.  Every call is synchronous; a map lives on one device and serves one thread at
 * a time; a handle on another device is refused.  No float atomics: two maps built by the same calls are byte-identical. */
typedef struct sicp_map_ctx* sicp_map;
typedef struct sicp_map_params {
  double leaf_size;     /* voxel edge, finite and > 0.  default 0.2 */
  int32_t num_classes;  /* 0..255; 0 (default): the map keeps no labels and the clouds' labels are ignored */
  int32_t reserved_;
} sicp_map_params;
int sicp_default_map_params(sicp_map_params* p);
int sicp_map_create(int device_id, const sicp_map_params* p, sicp_map* out);
int sicp_map_destroy(sicp_map m);
int sicp_map_clear(sicp_map m);  /* no voxels; the buffers stay */
int sicp_map_size(sicp_map m, int64_t* n_voxels, int64_t* n_points /* either nullable */);
const char* sicp_map_last_error(sicp_map m);

typedef struct sicp_map_integrate_info {
  int64_t n_in;            /* finite points of the slot */
  int64_t n_kept;          /* after the crop: the points added */
  int32_t n_scan_voxels;   /* voxels the scan touches */
  int32_t n_new_voxels;    /* ... of which the map did not hold */
  int64_t n_voxels;        /* the map's voxels after the call */
  double t_total_ms;       /* host wall clock */
} sicp_map_integrate_info;
/* Adds the finite points of slot `which` of h, in caller order whatever the handle's mode and device layout, transformed by qt
 * and cropped about crop_center with crop_range exactly as steps 2 and 3 of sicp_merge_clouds say (the kernels share the
 * arithmetic), to their voxels.  The handle is not modified -- cloud, features, correspondences and statistics stay, as with a
 * merge part; a cloud that is not yet on the device is prepared as a merge part is.  The work is a sort of the SCAN's keys plus
 * linear passes over the map; the map is never sorted.
 * SICP_ERR_INVALID_ARGUMENT: a NULL map or handle; `which` outside the two slots; a pose or centre that is not finite; a range
 * that is negative or NaN; a handle on another device; a cloud without labels into a map with num_classes > 0; a kept point
 * whose voxel coordinate reaches 2^20 (the text names the leaf size); more than 2^31 - 1 voxels or 2^32 - 1 points in all.
 * SICP_ERR_BAD_LABEL: a kept point's label above num_classes.  SICP_ERR_NOT_READY: the slot holds no cloud.
 * SICP_ERR_OUT_OF_MEMORY: the arena refused (sicp_set_memory_limit applies).  After each of these the map is exactly what it
 * was -- every extract output has the same bytes -- and stays usable, and info is not written.  A scan without a finite or kept
 * point: SICP_OK, nothing changes. */
int sicp_map_integrate(sicp_map m, sicp_handle h, int which, const double qt[7] /* NULL = identity */,
                       const double crop_center[3] /* NULL = 0 0 0 */, double crop_range /* 0 = none */,
                       sicp_map_integrate_info* info /* nullable */);
/* Keeps the voxels whose centroid -- (float)(s / count) per axis -- passes step 3's crop test about center with range (> 0;
 * +inf keeps everything); the survivors' state is unchanged bit for bit.  n_removed (nullable): voxels dropped. */
int sicp_map_prune(sicp_map m, const double center[3], double range, int64_t* n_removed);

/* ---- free-space carving: remove map voxels a new scan sees through ----------------
 * Every ray of a scan, from the sensor to its return, shows that the voxels it passes through are empty.  A map voxel that
 * enough rays of ONE scan pass through, and in which no return of that scan lands, is removed: the car that stood in scan 3
 * and drove off.  The intended order in a loop is align -> carve(scan, pose) -> integrate(scan, pose).  The rules:
 *  1. Points and origin.  The points are the finite points the slot holds, in caller order, whatever the handle's mode and
 *     device layout; each is transformed by qt exactly as sicp_map_integrate does, giving float p.  The origin o is
 *     (float)sensor_origin put through the same arithmetic, as a point of the scan would be.  Both are keyed with the grid's float
 *     arithmetic, v = floor(p * inv_leaf) with inv_leaf = 1.0f / (float)leaf_size: vo, vp.  An origin with |v| >= 2^20 on an axis
 *     is refused; a point with such a voxel takes no part (it is not an error).
 *  2. Hits.  Every point with a valid key marks its voxel's row as hit, if the map holds that voxel.  The range test plays no
 *     part here.
 *  3. Rays.  A point casts a ray when its key is valid and either max_range = 0 or step 3's crop test of sicp_merge_clouds
 *     holds for p about the centre o with the range max_range (all in float, as there).
 *  4. The walk runs in double, every operation rounded on its own, no contraction.  Per axis a: u = (double)o_a * (double)
 *     inv_leaf and w = (double)p_a * (double)inv_leaf (both products are exact); rem_a = |vp_a - vo_a| and step_a the sign of
 *     vp_a - vo_a.  For an axis with rem_a > 0: du = w - u, tmax_a = ((double)(vo_a + (step_a > 0 ? 1 : 0)) - u) / du and
 *     tdelta_a = (double)step_a / du.  The ray visits v_0 = vo and then takes exactly n = rem_x + rem_y + rem_z steps; a step
 *     picks, among the axes with rem_a > 0, the one with the smallest tmax_a (ties: x before y before z) and sets v_a +=
 *     step_a, rem_a -= 1, tmax_a = tmax_a + tdelta_a.  So v_n = vp by construction, whatever the rounding: the trip count is an
 *     integer known before the loop and nothing loops on a floating-point condition.  The carve candidates of the ray are v_i for
 *     0 <= i < n - end_margin (none when n <= end_margin; the return's own voxel v_n is never one).
 *  5. Miss counts.  miss[row] += 1 for every candidate the map holds.  A ray visits a voxel at most once; the counts are
 *     integers, so the result does not depend on the order of the updates.
 *  6. Removal.  A row is removed when miss >= min_rays, it is not hit, and its fullest histogram bin -- sicp_map_extract's label:
 *     ties to the smallest label, bin 0 can win -- is not in protect.  The survivors keep their state bit for bit and stay in
 *     ascending key; the map's point count follows, as in sicp_map_prune.
 *  7. Outputs.  miss (nullable, capacity elements): one count per row of the map BEFORE the call in ascending key, the order of
 *     sicp_map_extract with its defaults; written when non-NULL and capacity >= that row count.  A smaller capacity gives
 *     SICP_ERR_INVALID_ARGUMENT with info written (n_removed: the rows that would have gone) and nothing else happens.  info
 *     (nullable) is written on success and on that one refusal.
 *  8. Contracts: those of sicp_map_integrate.  The call computes into the spare set and swaps last, so every refusal leaves
 *     every extract byte as it was.  SICP_ERR_INVALID_ARGUMENT: a NULL map, handle or params; `which` outside the two slots; a
 *     pose or origin that is not finite; an origin beyond the key's range; max_range negative or NaN (+inf: every ray);
 *     min_rays < 1; end_margin < 0; dry_run neither 0 nor 1; n_protect outside 0..SICP_MAP_MAX_PROTECT, or > 0 on a map with
 *     num_classes = 0; a protected label above num_classes; a handle on another device.  SICP_ERR_NOT_READY: the slot holds no
 *     cloud.  An empty map, or a scan without rays: SICP_OK, nothing changes.  The handle is not modified; the cloud's labels are
 *     not read.  No float atomics: two maps driven alike are byte-identical, whatever the launch shape.
 * Cost: one lookup among the map's keys per candidate, a ray's candidates one after the other.  max_range is what bounds a
 * ray's length, n <= 3 * max_range / leaf_size + 3; with max_range = 0 a stray far return walks all the way (up to 3 * 2^21
 * steps), so a loop that feeds raw scans should set it.
 * The counts do not persist: a voxel must be seen through min_rays times by one scan.  The default min_rays = 3 is a choice; it
 * has not been tuned on real data. */
#define SICP_MAP_MAX_PROTECT 64
typedef struct sicp_map_carve_params {
  double  max_range;      /* 0 (default) = every ray; else only rays whose return passes step 3's crop test about the origin */
  int32_t min_rays;       /* a voxel goes when at least this many rays of THIS scan pass through it.  default 3, >= 1 */
  int32_t end_margin;     /* voxels before the return's voxel that a ray spares.  default 1, >= 0 */
  int32_t dry_run;        /* 1: count, remove nothing.  default 0 */
  int32_t n_protect;      /* 0 (default) .. SICP_MAP_MAX_PROTECT */
  uint32_t protect[SICP_MAP_MAX_PROTECT]; /* a voxel whose fullest histogram bin (extract's label rule) is one of these is never removed */
} sicp_map_carve_params;
typedef struct sicp_map_carve_info {
  int64_t n_in;           /* finite points of the slot */
  int64_t n_rays;         /* points that cast a ray */
  int64_t n_steps;        /* carve candidates visited by all rays (map or not) */
  int64_t n_voxels;       /* the map's voxels after the call */
  int32_t n_touched;      /* map rows with miss > 0 */
  int32_t n_hit;          /* map rows that hold a return of this scan */
  int32_t n_removed;      /* rows removed (dry_run: rows that would be) */
  int32_t n_spared_hit, n_spared_label;  /* rows with miss >= min_rays kept by the hit rule / by protect (hit first) */
  int32_t reserved_;
  double t_total_ms;      /* host wall clock */
} sicp_map_carve_info;
int sicp_default_map_carve_params(sicp_map_carve_params* p);
int sicp_map_carve(sicp_map m, sicp_handle h, int which, const double qt[7] /* NULL = identity */,
                   const double sensor_origin[3] /* in the scan's own frame; NULL = 0 0 0 */,
                   const sicp_map_carve_params* p, int32_t capacity, uint32_t* miss /* nullable */,
                   sicp_map_carve_info* info /* nullable */);

/* ---- ray casting: what a sensor at a pose sees of the map -------------------------
 * The map read along lines of sight (OctoMap's castRay, Open3D's VoxelBlockGrid.ray_cast).  The caller gives END POINTS, not
 * directions: ray i is the segment from the sensor origin to (ex, ey, ez)[i], both in the sensor's frame, which is exactly a
 * carve ray of a virtual return -- so a virtual scan pattern and "the scan's own points" are the same call.  It answers, per
 * ray, the first opaque voxel on the way, and can make the distinct voxels hit the cloud of a handle's slot: a target without
 * what is occluded, a rendered scan for sicp_place_query; with `ignore` the rays pass the voxels of moving classes; with the
 * scan's own points as ends, step < length says that the map holds something in front of that return.  The rules:
 *  1. Origin and ends.  Carve rule 1 word for word: each end and (float)sensor_origin go through the transform of
 *     sicp_map_integrate, giving float p and o; both are keyed with the grid's float arithmetic: vp, vo.  An origin with
 *     |v| >= 2^20 on an axis is refused.  An end that is not finite, or whose voxel is beyond the key's range, casts no ray (it
 *     is not an error).
 *  2. Which ends cast.  Carve rule 3: a valid key and either max_range = 0 or step 3's crop test of sicp_merge_clouds for p about
 *     the centre o with the range max_range.
 *  3. The walk.  Carve rule 4 unchanged: v_0 = vo, then exactly n = rem_x + rem_y + rem_z steps, so v_n = vp.
 *  4. Opaque.  A map row is opaque when count >= min_count and, when n_ignore > 0, its fullest histogram bin -- sicp_map_extract's
 *     label: ties to the smallest label, bin 0 can win -- is not in ignore.
 *  5. Hit.  The hit is the smallest i in start_margin .. n whose voxel v_i the map holds as an opaque row.  The end's own voxel
 *     v_n is tested.
 *  6. A ray with a hit.  row[i]: the row's index in ascending key, the order of sicp_map_extract with default params -- it
 *     indexes the arrays of sicp_map_extract and sicp_map_extract_fused, so a fused label or a histogram per ray is one gather
 *     away.  step[i]: the hit's index in the walk.  length[i]: n.  x, y, z: the centroid as extract rounds it, (float)(s /
 *     count).  label: the fullest bin; 0 on a map with num_classes = 0.  count: the voxel's count.  range_sq: with dx =
 *     (double)x - (double)o_x and likewise dy, dz, the value (dx dx + dy dy) + dz dz, every operation rounded once, no
 *     contraction; the caller takes the root, the library takes none.
 *  7. Without a hit.  A ray that ran to its end gets row = -1, step = -1, length = n, zeros in the other arrays and range_sq =
 *     -1.0.  An end that cast no ray gets the same with length = -1.
 *  8. n_steps is the sum over the rays cast of the voxels tested: step - start_margin + 1 for a ray with a hit,
 *     max(n + 1 - start_margin, 0) for one without.
 *  9. dst (nullable).  The n_visible distinct rows hit, in ascending key, become slot dst_which of dst: their x, y, z and -- when
 *     the map has classes -- label, exactly as sicp_set_cloud of those arrays would make it (the path of sicp_map_extract).
 *     The result is complete before the slot lets go of its old cloud.
 * 10. n_visible = 0 with a dst gives SICP_ERR_TOO_FEW_POINTS; info is written, dst and every array are untouched.
 * 11. Contracts.  The map is never modified; dst is the only handle touched; the call is synchronous, on the map's stream.
 *     SICP_ERR_INVALID_ARGUMENT with nothing written: a NULL map, params or end array; n < 0; a pose or origin that is not
 *     finite; an origin beyond the key's range; max_range negative or NaN (+inf: every ray); min_count < 1; start_margin < 0;
 *     n_ignore outside 0..SICP_MAP_RAYCAST_MAX_IGNORE, or > 0 on a map with num_classes = 0; an ignored label above
 *     num_classes; with a dst, a dst_which outside the two slots or a dst on another device.  SICP_ERR_OUT_OF_MEMORY: the arena
 *     refused (sicp_set_memory_limit applies); nothing is written.  n = 0, or an empty map, without dst: SICP_OK, the results are
 *     "no hit", and on an empty map n_steps is still counted.  Every output array is nullable and n long.  No float atomics:
 *     every per-ray output is a plain store by the lane that owns the ray, the visible marks are plain stores of 1, the counts
 *     integer atomics -- the bytes depend neither on the launch shape nor on which other rays are in the call.
 * Cost: as carve's, one lookup among the map's keys per voxel walked, but a walk ends at its hit.  max_range, or the ends
 * themselves, bound a ray's length.
 * Not built: an origin per ray; a batch or stream form; the fused label inside the call (gather extract_fused's by row); a hit
 * position on the voxel's face (the answer is the voxel's centroid). */
#define SICP_MAP_RAYCAST_MAX_IGNORE 64
typedef struct sicp_map_raycast_params {
  double  max_range;     /* 0 (default) = every ray; else only rays whose end passes the crop test about the origin (carve rule 3) */
  int32_t min_count;     /* a voxel with fewer points is transparent.  default 1, >= 1 */
  int32_t start_margin;  /* the first start_margin voxels of a walk are not tested.  default 1 (the sensor's own voxel), >= 0 */
  int32_t n_ignore;      /* 0 (default) .. SICP_MAP_RAYCAST_MAX_IGNORE */
  int32_t reserved_;
  uint32_t ignore[SICP_MAP_RAYCAST_MAX_IGNORE]; /* a voxel whose fullest histogram bin (extract's label rule) is one of these is transparent */
} sicp_map_raycast_params;
typedef struct sicp_map_raycast_info {
  int64_t n_in, n_rays, n_steps, n_hits, n_voxels;  /* rays given / cast / voxels tested by all rays / rays with a hit / map rows */
  int32_t n_visible, reserved_;                     /* distinct rows hit */
  double t_total_ms;                                /* host wall clock */
} sicp_map_raycast_info;
int sicp_default_map_raycast_params(sicp_map_raycast_params* p);
int sicp_map_raycast(sicp_map m, const double qt[7] /* NULL = identity */, const double sensor_origin[3] /* NULL = 0 0 0 */,
                     int32_t n, const float* ex, const float* ey, const float* ez,   /* ray i ends at (ex,ey,ez)[i], sensor frame */
                     const sicp_map_raycast_params* p, sicp_handle dst /* nullable */, int dst_which,
                     int32_t* row, int32_t* step, int32_t* length, float* x, float* y, float* z, uint32_t* label,
                     uint32_t* count, double* range_sq,                              /* n each, every one nullable */
                     sicp_map_raycast_info* info /* nullable */);

/* ---- elevation: the map as a semantic 2.5-D height grid ---------------------------
 * What a planner reads (grid_map, elevation_mapping, OctoMap's projected map, multi-level surface maps): per ground cell of a
 * window the height of the surface one can stand on, what it is, what hangs over it, how much it steps to its neighbours and
 * whether it is free -- and, for the points of a handle's slot, their height above that MAPPED ground, which is there where a
 * single scan sees no ground at all.  The map is read and never modified.  Every floating-point operation is rounded on its
 * own, no contraction.  leaf and inv_leaf = 1.0f / (float)leaf_size are the map's; B = cell_voxels; fdiv(a, B) is the
 * mathematical floor of a / B (not C's division for a negative a).  The host forms once: lo = floorf((float)z_min * inv_leaf)
 * and hi = floorf((float)z_max * inv_leaf), both clamped to the key's range -(2^20 - 1) .. 2^20 - 1 (so -inf and +inf give its
 * ends), and vref = floorf((float)ref_z * inv_leaf) clamped to -2^20 .. 2^20.  The rules:
 *  1. Window.  center (x, y; finite) is keyed with the grid's float arithmetic, vc = floorf((float)center * inv_leaf) per axis;
 *     a centre with |vc| >= 2^20 is refused.  x0 = fdiv(vc_x, B) - width / 2 and y0 = fdiv(vc_y, B) - height / 2 (integer
 *     halves).  Cell (i, j), output index c = j * width + i, holds the voxel columns with fdiv(vx, B) = x0 + i and fdiv(vy, B) =
 *     y0 + j.  info returns x0, y0 and cell_size = B * leaf_size.
 *  2. Rows that count.  A map row counts when count >= min_count; when n_ignore > 0, its fullest histogram bin --
 *     sicp_map_extract's label: ties to the smallest label, bin 0 can win -- is not in ignore (sicp_map_raycast's rule 4);
 *     lo <= vz <= hi; and its column lies in the window.
 *  3. Levels and runs.  A cell's levels are the distinct vz of its counting rows, ascending: l_0 < l_1 < ...  Level l_k starts a
 *     new run when k = 0 or l_k - l_(k-1) > clearance_voxels.  A cell without a level is EMPTY.
 *  4. The chosen run.  use_ref_z = 0: the first run.  use_ref_z = 1: the last run whose bottom level is <= vref; when there is
 *     none, the first run (a level of a multi-level place: a bridge deck over a road).
 *  5. Per SURFACE cell, the chosen run having top level t and bottom level b.  The mean at a level: S = 0.0, N = 0, then over
 *     the cell's counting rows at that level in ascending map row (= ascending key) S = S + sz[row], N += count[row]; the mean
 *     is (float)(S / (double)N) -- for B = 1 sicp_map_extract's z of that voxel, byte for byte.  elevation: the mean at t.
 *     bottom: the mean at b.  ceiling: the mean at the bottom level of the run that follows the chosen one, +inf when there is
 *     none.  count: N at t.  label: the fullest bin of the level-t rows' histograms added bin by bin (ties to the smallest
 *     label, bin 0 can win); 0 on a map without classes.  level_top = t, level_bottom = b; n_levels: the levels of the run;
 *     state = 1.  An EMPTY cell: state = 0; elevation, bottom and ceiling the quiet NaN 0x7fc00000; zeros elsewhere.
 *  6. Neighbourhood.  neighbors of a SURFACE cell: the SURFACE cells among the up to 8 adjacent cells inside the window.  step:
 *     the maximum over those of fabsf(e_n - e_c), one float subtraction each (the maximum is exact: the order does not matter);
 *     0.0f when there are none.  An EMPTY cell: step that NaN, neighbors 0.
 *  7. Class; the first test that holds decides:
 *       SICP_ELEVATION_UNKNOWN 0        the cell is EMPTY
 *       SICP_ELEVATION_BLOCKED_LABEL 2  n_blocked > 0 and the label is in blocked, or n_drivable > 0 and it is not in drivable
 *       SICP_ELEVATION_OBSTACLE 3       level_top - level_bottom > max_extent_voxels (a wall, a trunk, a parked car not ignored)
 *       SICP_ELEVATION_LOW_CLEARANCE 4  min_clearance > 0, ceiling finite, (double)(ceiling - elevation) < min_clearance (the
 *                                       difference in float)
 *       SICP_ELEVATION_STEP 5           (double)step > max_step
 *       SICP_ELEVATION_SPARSE 6         neighbors < min_neighbors
 *       SICP_ELEVATION_FREE 1           none of the above
 *     info.n_class[8]: the cells per class, counted on the device with integer atomics, so valid without any array.
 *  8. Points (h non-NULL).  Every one of the slot's n_points in caller order, whatever the handle's mode and device layout: a
 *     point that is not finite gets point_cell = -1 and point_height = that NaN; a finite one goes through
 *     sicp_map_integrate's transform and the grid's key arithmetic, without a crop; beyond the key's range or outside the window
 *     it gets -1 and NaN; in an EMPTY cell c and NaN; otherwise c and pz - elevation[c], one float subtraction.  The handle is
 *     not modified; a cloud that is not yet on the device is prepared as a merge part is.
 *  9. Contracts.  Every output array is nullable; the cell arrays are width * height long, the point arrays n_points.  The call
 *     is synchronous, on the map's stream.  No float atomics: every cell's bytes are plain stores by the lane that owns the
 *     cell and do not depend on the launch shape; those of state, elevation, bottom, ceiling, label, count and the levels do
 *     not depend on the window the cell is seen through.  An empty map: SICP_OK, every cell EMPTY.
 *     SICP_ERR_INVALID_ARGUMENT with nothing written (info included): a NULL map, params or centre; width or height outside
 *     1..2048; cell_voxels outside 1..8; min_count < 1; n_ignore, n_blocked or n_drivable outside
 *     0..SICP_MAP_ELEVATION_MAX_LABELS, or > 0 on a map with num_classes = 0; a listed label above num_classes; z_min or z_max
 *     NaN, or z_min > z_max; clearance_voxels < 1; use_ref_z neither 0 nor 1, or 1 with a ref_z that is not finite;
 *     max_extent_voxels < 0; min_clearance or max_step negative or NaN; min_neighbors outside 0..8; a centre that is not finite
 *     or beyond the key's range; a pose that is not finite; with a handle, `which` outside the two slots or a handle on another
 *     device; point outputs without a handle.  SICP_ERR_NOT_READY: the slot holds no cloud.  SICP_ERR_OUT_OF_MEMORY: the arena
 *     refused (sicp_set_memory_limit applies); nothing is written.  sicp_map_last_error names the cause.
 * Cost: one sort of the map's rows by (cell, level) -- the rows outside the window sort behind -- and linear passes; a cell's
 * column is walked by one lane, so a facade at cell_voxels = 8 costs its lane a few hundred rows.
 * Memory: device scratch of about 45 bytes a cell and 28 a map row for the call's duration (the arena keeps it for later
 * calls), and a pinned read-back buffer sized by the arrays asked for -- up to 39 bytes a cell, 160 MB at 2048 x 2048 -- which
 * stays with the map for the next call up to 64 MB and is given back at the call's end above that.
 * Not built: a dst cloud of the surface cells; slope or roughness (they need roots and quotients); fused (confusion-matrix)
 * labels per cell; a persistent grid updated per scan; batch and stream forms; the C++ class shims. */
#define SICP_MAP_ELEVATION_MAX_LABELS 64
enum {
  SICP_ELEVATION_UNKNOWN = 0, SICP_ELEVATION_FREE = 1, SICP_ELEVATION_BLOCKED_LABEL = 2, SICP_ELEVATION_OBSTACLE = 3,
  SICP_ELEVATION_LOW_CLEARANCE = 4, SICP_ELEVATION_STEP = 5, SICP_ELEVATION_SPARSE = 6
};
typedef struct sicp_map_elevation_params {
  double  z_min, z_max;        /* rows outside are not seen.  default -inf, +inf; not NaN, z_min <= z_max */
  double  ref_z;               /* read with use_ref_z = 1; finite then.  default 0 */
  double  min_clearance;       /* >= 0; 0 (default) = the LOW_CLEARANCE test is off */
  double  max_step;            /* >= 0; +inf (default) = the STEP test is off */
  int32_t width, height;       /* cells, 1..2048 each; no default: the caller sets them */
  int32_t cell_voxels;         /* a cell is B x B voxel columns.  1..8, default 1 */
  int32_t min_count;           /* a voxel with fewer points is not seen.  default 1, >= 1 */
  int32_t clearance_voxels;    /* the free height that separates one surface from the one above it.  default 10, >= 1 */
  int32_t use_ref_z;           /* 0 (default): the lowest surface; 1: rule 4's run at ref_z */
  int32_t max_extent_voxels;   /* a run taller than this is an OBSTACLE.  default 2, >= 0 */
  int32_t min_neighbors;       /* 0 (default, off) .. 8 */
  int32_t n_ignore, n_blocked, n_drivable;  /* 0 (default) .. SICP_MAP_ELEVATION_MAX_LABELS each */
  int32_t reserved_;
  uint32_t ignore[SICP_MAP_ELEVATION_MAX_LABELS];   /* a voxel whose fullest histogram bin is one of these does not exist here */
  uint32_t blocked[SICP_MAP_ELEVATION_MAX_LABELS];  /* a surface with one of these labels is BLOCKED_LABEL */
  uint32_t drivable[SICP_MAP_ELEVATION_MAX_LABELS]; /* when given, a surface with any other label is BLOCKED_LABEL */
} sicp_map_elevation_params;
typedef struct sicp_map_elevation_out {
  uint8_t* state;              /* width * height each, c = j * width + i */
  float* elevation;
  float* bottom;
  float* ceiling;
  uint32_t* label;
  uint32_t* count;
  int32_t* level_top;
  int32_t* level_bottom;
  int32_t* n_levels;
  float* step;
  uint8_t* neighbors;
  uint8_t* cell_class;
  int32_t* point_cell;         /* n_points each; they need a handle */
  float* point_height;
} sicp_map_elevation_out;
typedef struct sicp_map_elevation_info {
  int64_t n_voxels;            /* map rows */
  int64_t n_points;            /* what the slot's caller handed over; 0 without a handle */
  int32_t x0, y0;              /* rule 1: the cell coordinates of output cell (0, 0) */
  int32_t width, height;
  int32_t n_class[8];          /* cells per class, indexed by SICP_ELEVATION_UNKNOWN .. SICP_ELEVATION_SPARSE (7: unused, 0) */
  double cell_size;            /* cell_voxels * leaf_size */
  double t_total_ms;           /* host wall clock */
} sicp_map_elevation_info;
int sicp_default_map_elevation_params(sicp_map_elevation_params* p);
int sicp_map_elevation(sicp_map m, const double center[2], const sicp_map_elevation_params* p,
                       const sicp_map_elevation_out* out /* nullable */, sicp_handle h /* nullable */, int which,
                       const double qt[7] /* NULL = identity */, sicp_map_elevation_info* info /* nullable */);

/* ---- distance: a truncated Euclidean distance field of the map ------------------------
 * What Voxblox, FIESTA and nvblox keep for a planner: per voxel of a dense window, how far the nearest occupied voxel is and
 * which map row that is -- for collision checks of a body with height, for obstacle inflation of a 2-D grid (planar mode), for
 * "which points of this scan are far from everything the map holds" (the points of a handle's slot), and, through `only`, for
 * "how far is this place from the nearest voxel of class X".  The map is read and never modified.  leaf and inv_leaf = 1.0f /
 * (float)leaf_size are the map's; everything after the keying is integer arithmetic, in units of one voxel.  The rules:
 *  1. Window.  center[3] (finite) is keyed with the grid's float arithmetic, vc = floorf((float)center * inv_leaf) per axis; a
 *     centre with |vc| >= 2^20 is refused.  nx, ny in 1..1024, nz in 1..256, nx * ny * nz <= 2^24.  x0 = vc_x - nx / 2, y0 =
 *     vc_y - ny / 2, z0 = vc_z - nz / 2 (integer halves).  Cell (i, j, k), output index c = (k * ny + j) * nx + i, is the voxel
 *     (x0 + i, y0 + j, z0 + k).  Voxels beyond the key's range are simply never occupied.  info returns x0, y0, z0.
 *  2. Obstacles.  A map row counts when count >= min_count; when n_ignore > 0, its fullest histogram bin -- sicp_map_extract's
 *     label: ties to the smallest label, bin 0 can win -- is not in ignore; when n_only > 0, that label is in only; and its
 *     voxel lies in the window.  An obstacle outside the window does not exist for the call.
 *  3. Planar mode (planar = 1; nz must be 1).  An obstacle is a column (vx, vy) of the window that holds a counting row with
 *     lo <= vz <= hi, where lo = floorf((float)z_min * inv_leaf) and hi = floorf((float)z_max * inv_leaf), both clamped to the
 *     key's range -(2^20 - 1) .. 2^20 - 1 as sicp_map_elevation's are.  The column's row is the smallest such row.  Distances
 *     are taken in the plane, center[2] is ignored apart from being finite, and z0 = 0.  This is obstacle inflation for a body
 *     that occupies a height band.  With planar = 0, z_min and z_max are checked and otherwise not read.
 *  4. The field.  R = max_dist_voxels, 1..64.  For cell c, D = the minimum over the obstacles o of di^2 + dj^2 + dk^2
 *     (integers; dk = 0 in planar mode).  D <= R^2: dist_sq[c] = D, nearest[c] = the smallest map row among the obstacles at
 *     exactly D -- a row is its index in sicp_map_get_state's order, ascending key -- and label[c] = that row's fullest bin (0
 *     on a map without classes).  Otherwise dist_sq[c] = -1, nearest[c] = -1, label[c] = 0.  The truncation is a ball, not a
 *     cube: with R = 5 an obstacle at offset (3, 4, 0) is found, one at (5, 1, 0) is not.  The metric distance is leaf_size *
 *     sqrt(dist_sq); the call takes no root.
 *  5. Points (h non-NULL).  Every one of the slot's n_points in caller order, whatever the handle's mode and device layout.  A
 *     point that is not finite gets point_cell = -1, point_dist_sq = -1, point_nearest = -1 and point_range_sq the quiet NaN
 *     0x7fc00000.  A finite one goes through sicp_map_integrate's transform and the grid's key arithmetic, v = floorf(p *
 *     inv_leaf) per axis in float, without a crop; with a |v| >= 2^20 or outside the window it gets the same values; inside,
 *     point_cell = c, point_dist_sq = dist_sq[c], point_nearest = nearest[c].  In planar mode only x and y decide (z is not
 *     looked at).  point_range_sq (3-D mode only): with nearest[c] >= 0 the float squared distance from the moved point to that
 *     row's centroid (float)(s / count) -- d = p - centroid, (dx dx + dy dy) + dz dz, each operation rounded on its own --
 *     otherwise that NaN.  The handle is not modified; a cloud that is not yet on the device is prepared as a merge part is.
 *  6. Contracts.  Every output array is nullable; the cell arrays are nx * ny * nz long, the point arrays n_points.  The call is
 *     synchronous, on the map's stream.  Integer arithmetic and plain stores, plus one integer atomicMin per row when seeding
 *     in planar mode: the bytes do not depend on the launch shape.  A cell at least R cells from every face of the window has
 *     bytes that do not depend on the window (nearest: between calls on equal map state).  An empty map: SICP_OK, every cell
 *     -1.  info: n_voxels, n_points, n_points_inside (points with point_cell >= 0), x0, y0, z0, nx, ny, nz, n_obstacles
 *     (obstacle cells of the window), n_reached (cells with dist_sq >= 0), max_dist_sq (the largest reached value, -1 when
 *     there is none), voxel_size = leaf_size and t_total_ms; the counts come from the device with integer atomics, so they
 *     are valid without any array.
 *     SICP_ERR_INVALID_ARGUMENT with nothing written (info included): a NULL map, params or centre; nx or ny outside 1..1024,
 *     nz outside 1..256, or nx * ny * nz above 2^24; max_dist_voxels outside 1..64; min_count < 1; planar neither 0 nor 1, or
 *     1 with nz != 1; z_min or z_max NaN, or z_min > z_max; n_ignore or n_only outside 0..SICP_MAP_DISTANCE_MAX_LABELS, or > 0
 *     on a map with num_classes = 0; a listed label above num_classes; a centre that is not finite or beyond the key's range; a
 *     pose that is not finite; with a handle, `which` outside the two slots or a handle on another device; point outputs
 *     without a handle; point_range_sq with planar = 1.  SICP_ERR_NOT_READY: the slot holds no cloud.
 *     SICP_ERR_OUT_OF_MEMORY: the arena refused (sicp_set_memory_limit applies); nothing is written.  sicp_map_last_error
 *     names the cause.
 * Cost: one lane per map row to seed, then one windowed-minimum sweep per axis longer than one cell -- 2 R + 1 integer
 * min-adds and 16 bytes of traffic a cell each -- and one pass that unpacks.  The field is the lexicographic minimum of
 * (d^2, row), which is separable: see DESIGN.md 3.20.
 * Memory: device scratch of 28 bytes a cell (two 8-byte key buffers and the three outputs; 0.47 GB at 2^24 cells), 4 a map
 * row and 16 a point for the call's duration (the arena keeps it for later calls), and a pinned read-back buffer of 4 bytes a
 * cell and a point per array asked for -- up to 12 bytes a cell, 201 MB at 2^24 cells -- which stays with the map for the next
 * call up to 64 MB and is given back at the call's end above that.
 * Not built: a field kept on the device between calls or updated per scan; a signed field (distance inside obstacles);
 * gradients; batch and stream forms; the C++ class shims. */
#define SICP_MAP_DISTANCE_MAX_LABELS 64
typedef struct sicp_map_distance_params {
  double  z_min, z_max;        /* planar mode: the height band.  default -inf, +inf; not NaN, z_min <= z_max */
  int32_t nx, ny, nz;          /* cells: 1..1024, 1..1024, 1..256, product <= 2^24; no default: the caller sets them */
  int32_t max_dist_voxels;     /* R: the field is truncated at this many voxels.  1..64, default 10 */
  int32_t min_count;           /* a voxel with fewer points is not seen.  default 1, >= 1 */
  int32_t planar;              /* 0 (default): the 3-D field; 1: rule 3's field in the plane, nz = 1 */
  int32_t n_ignore, n_only;    /* 0 (default) .. SICP_MAP_DISTANCE_MAX_LABELS each */
  uint32_t ignore[SICP_MAP_DISTANCE_MAX_LABELS];  /* a voxel whose fullest histogram bin is one of these does not exist here */
  uint32_t only[SICP_MAP_DISTANCE_MAX_LABELS];    /* when given, a voxel with any other label does not exist here */
} sicp_map_distance_params;
typedef struct sicp_map_distance_out {
  int32_t* dist_sq;            /* nx * ny * nz each, c = (k * ny + j) * nx + i */
  int32_t* nearest;
  uint32_t* label;
  int32_t* point_cell;         /* n_points each; they need a handle */
  int32_t* point_dist_sq;
  int32_t* point_nearest;
  float* point_range_sq;       /* 3-D mode only */
} sicp_map_distance_out;
typedef struct sicp_map_distance_info {
  int64_t n_voxels;            /* map rows */
  int64_t n_points;            /* what the slot's caller handed over; 0 without a handle */
  int64_t n_points_inside;     /* points with point_cell >= 0 */
  int32_t x0, y0, z0;          /* rule 1: the voxel of output cell (0, 0, 0) */
  int32_t nx, ny, nz;
  int32_t n_obstacles;         /* obstacle cells of the window */
  int32_t n_reached;           /* cells with dist_sq >= 0 */
  int32_t max_dist_sq;         /* the largest dist_sq; -1 when no cell is reached */
  int32_t reserved_;
  double voxel_size;           /* leaf_size: the metric distance is voxel_size * sqrt(dist_sq) */
  double t_total_ms;           /* host wall clock */
} sicp_map_distance_info;
int sicp_default_map_distance_params(sicp_map_distance_params* p);
int sicp_map_distance(sicp_map m, const double center[3], const sicp_map_distance_params* p,
                      const sicp_map_distance_out* out /* nullable */, sicp_handle h /* nullable */, int which,
                      const double qt[7] /* NULL = identity */, sicp_map_distance_info* info /* nullable */);

typedef struct sicp_map_extract_params {
  int32_t min_count;      /* voxels with fewer points are left out.  default 1 */
  int32_t reserved_;
  double crop_center[3];  /* default 0 0 0 */
  double crop_range;      /* 0 = no crop (default); else prune's test on the centroid */
} sicp_map_extract_params;
typedef struct sicp_map_extract_info {
  int64_t n_voxels;          /* of the map */
  int32_t n_out;             /* voxels selected */
  int32_t max_voxel_points;  /* largest count among them; 0 when n_out = 0 */
  int32_t has_label, reserved_;
  double t_total_ms;
} sicp_map_extract_info;
int sicp_default_map_extract_params(sicp_map_extract_params* p);
/* One point per selected voxel in ascending key, i.e. ascending (vz, vy, vx): the centroid rounded once to float, count[j] the
 * voxel's count, label[j] its fullest histogram bin (ties to the smallest label; untouched when num_classes = 0), hist
 * (capacity * (num_classes + 1), refused when num_classes = 0) the row itself.  The map is not modified.  Capacity, dst and info
 * follow sicp_merge_clouds: info (nullable) is written on success and on the capacity refusal; every array is nullable; a
 * non-NULL array with capacity < n_out gives SICP_ERR_INVALID_ARGUMENT and nothing else happens; slot dst_which of dst
 * (nullable) becomes the result exactly as sicp_set_cloud of the arrays would make it, and the result is complete before the
 * slot lets go of its old cloud; n_out = 0 with a dst gives SICP_ERR_TOO_FEW_POINTS and dst is unchanged. */
int sicp_map_extract(sicp_map m, const sicp_map_extract_params* p, sicp_handle dst /* nullable */, int dst_which, int32_t capacity,
                     float* x, float* y, float* z, uint32_t* label, uint32_t* count, uint32_t* hist,
                     sicp_map_extract_info* info /* nullable */);

/* ---- the map's labels through the confusion matrix ------------------------------
 * sicp_map_extract's label is a majority vote.  With a confusion matrix the map gives the maximum a-posteriori class of a
 * voxel under a uniform prior, and its posterior probability: for a histogram row h[0..C] and L[r][s] = log cm[r*C + s],
 *     score_s = 0.0;  for r = 1..C ascending, where h[r] > 0:  score_s = score_s + (double)h[r] * L[r-1][s-1]
 * (product and sum rounded once each, no contraction; the order is the specification).  Bin 0, "unlabelled", never
 * contributes.  No evidence: no term was added, or the largest score is -inf (every class is ruled out by a zero entry).
 * Otherwise the fused label is the smallest s whose score is the largest, and
 *     confidence = 1 / sum_s exp(score_s - max)
 * in double, summed in this fixed tree: the scoring lanes' own classes (lane j of the map's 64, or of the power of two >= C
 * when C < 64, owns s = j+1, j+1+64, ...) in ascending s, then pairs of lanes at distance 1, 2, 4, ...  No float atomics: two
 * runs give the same bytes.
 *
 * sicp_map_set_confusion: cm[r*C + s] as sicp_set_confusion has it (observed label r+1, class s+1).  May be called at any
 * time and replaces the previous matrix.  Zero entries are allowed (log 0 = -inf).  SICP_ERR_INVALID_ARGUMENT, the map and any
 * earlier matrix unchanged: a NULL pointer; a map with num_classes = 0; C != num_classes; an entry that is negative or not
 * finite (sicp_map_last_error names it).  The logarithms are taken on the host (double, libm) and only they go to the device,
 * into an arena buffer (sicp_set_memory_limit applies). */
int sicp_map_set_confusion(sicp_map m, int32_t C, const double* cm_rowmajor);
/* sicp_map_extract with the fused label in label[j] and its confidence in confidence[j] (0 and 0.0 for a voxel without
 * evidence): the same selection and order under the same p, the same x, y, z, count and info, the same capacity, dst (the slot
 * becomes what sicp_set_cloud of these arrays makes it) and n_out = 0 rules, the same refusals.  SICP_ERR_NOT_READY: no matrix
 * has been set.  SICP_ERR_INVALID_ARGUMENT: num_classes = 0.  The map is not modified. */
int sicp_map_extract_fused(sicp_map m, const sicp_map_extract_params* p, sicp_handle dst /* nullable */, int dst_which,
                           int32_t capacity, float* x, float* y, float* z, uint32_t* label, uint32_t* count,
                           double* confidence, sicp_map_extract_info* info /* arrays and info nullable */);
/* getFusedLabels against the map: a label and a confidence for every one of the slot's n_points (sicp_cloud_size), in caller
 * order whatever the handle's mode and layout.  A point that is not finite gets label 0 and confidence 0 (sicp_fused_labels'
 * rule).  A finite point is transformed by qt and keyed exactly as sicp_map_integrate does, without a crop; a coordinate beyond
 * the key's range means "not in the map", it is not an error.  Evidence: the row of the point's voxel when the map holds it
 * with count >= min_count; then, added last, the one term L[own-1][s-1] when include_own_label is 1, the cloud has labels and
 * the point's label is in 1..C (the reference multiplies source and target distributions; this is the analogue).  With
 * evidence: the fused label and confidence as above.  Without: the point's own label (0 when the cloud has none) and
 * confidence 0.  SICP_ERR_BAD_LABEL, nothing written: include_own_label is set and a finite point's label is above
 * num_classes.  SICP_ERR_INVALID_ARGUMENT, nothing written: a NULL map, handle or out_labels; `which` outside the two slots;
 * a flag that is neither 0 nor 1; min_count < 1; a pose that is not finite; a handle on another device; num_classes = 0.
 * SICP_ERR_NOT_READY: no matrix has been set, or the slot holds no cloud.  Neither the handle nor the map changes. */
int sicp_map_fused_labels(sicp_map m, sicp_handle h, int which, const double qt[7] /* NULL = identity */,
                          int32_t include_own_label, int32_t min_count, uint32_t* out_labels,
                          double* out_confidence /* nullable */);

/* ---- fusing maps: a submap into a global map at its pose ---------------------------
 * After a loop closure the trajectory moves and the map has to follow.  A map does not record which scan gave what, so the
 * answer is submaps: a few dozen scans integrated into a small map in the submap's own frame, the submap a node of the pose
 * graph, and after sicp_graph_optimize every submap added into the global map at its corrected pose -- with its counts, the
 * weight of its centroids and its histograms intact, which sicp_map_extract into a handle followed by sicp_map_integrate
 * loses (that route counts every voxel as one observation).  sicp_map_merge adds src's rows into dst:
 *  1. Rows.  src's, in ascending key; row r has the sums s, the count c and the histogram h.  A row with c < min_count takes no
 *     part.
 *  2. Moved sums.  M is the matrix of qt exactly as sicp_map_integrate forms it.  Per axis a, in double, every operation
 *     rounded on its own, no contraction: t_a = ((M[a][0] sx + M[a][1] sy) + M[a][2] sz) + M[a][3] (double)c -- step 2's order
 *     of sicp_merge_clouds with the translation scaled by the count and no rounding to float.  Under the identity t == s bit for
 *     bit (a sum of -0.0, which no integrate produces, becomes +0.0).
 *  3. Where it lands.  p_a = (float)(t_a / (double)c).  When crop_range > 0, p takes step 3's crop test of sicp_merge_clouds
 *     about crop_center, in dst's frame.  Then p is keyed on DST's grid, v = floor(p * (1.0f / (float)dst.leaf_size)): the two
 *     maps may differ in leaf size.  |v| >= 2^20 on any axis refuses the call as sicp_map_integrate does (the text names dst's
 *     leaf size).  Keying the centroid of the moved SUMS, not the moved float centroid, keeps what every integrate-only map
 *     has: a row's (float)(s / count) lies in the row's own voxel.
 *  4. Fold.  A dst voxel's sums continue from their stored value (0.0 for a voxel dst did not hold) with the contributions in
 *     ascending src row, one add per axis and contributing row; count += c; every histogram bin += h[bin].  The order of the
 *     float adds is the specification; there are no float atomics, so two maps driven alike are byte-identical.  A row moves
 *     whole: its mass is never spread over several voxels.
 *  5. Labels.  dst.num_classes == 0: src's histograms are ignored.  Otherwise src.num_classes must equal dst.num_classes.
 *  6. Limits.  More than 2^31 - 1 voxels or 2^32 - 1 points in dst refuse the call (the second bounds every voxel's count);
 *     both are checked before a row is written.
 *  7. Contracts: sicp_map_integrate's.  The call computes into dst's spare set and swaps last: after every refusal dst holds the
 *     bytes it held and stays usable, and info is not written.  src is never modified.  SICP_ERR_INVALID_ARGUMENT, with the
 *     reason in sicp_map_last_error(dst): a NULL map; src == dst; maps on different devices; a pose or centre that is not
 *     finite; crop_range negative or NaN; min_count < 1; a class mismatch; rules 3 and 6.  SICP_ERR_OUT_OF_MEMORY: the arena
 *     refused.  An empty src, or no kept row: SICP_OK, nothing changes, info is written.  The call is synchronous and runs on
 *     dst's stream; a map serves one thread at a time, and a merge occupies BOTH maps: no other call may run on src or on dst
 *     until it returns.
 * The work is one sort of src's rows plus linear passes over both maps; dst is never sorted. */
typedef struct sicp_map_merge_params {
  int32_t min_count;      /* src rows with fewer points take no part.  default 1, >= 1 */
  int32_t reserved_;
  double crop_center[3];  /* default 0 0 0, in dst's frame */
  double crop_range;      /* 0 = no crop (default); +inf allowed */
} sicp_map_merge_params;
typedef struct sicp_map_merge_info {
  int64_t n_src_rows;      /* src's voxels */
  int64_t n_kept_rows;     /* after min_count and the crop */
  int64_t n_kept_points;   /* the sum of their counts: what dst's point count rises by */
  int32_t n_touched;       /* dst voxels that receive something */
  int32_t n_new_voxels;    /* ... of which dst did not hold */
  int32_t max_run;         /* most src rows landing in one dst voxel; 0 when nothing was kept */
  int32_t reserved_;
  int64_t n_voxels;        /* dst's voxels after the call */
  double t_total_ms;       /* host wall clock */
} sicp_map_merge_info;
int sicp_default_map_merge_params(sicp_map_merge_params* p);
int sicp_map_merge(sicp_map dst, sicp_map src, const double qt[7] /* src frame -> dst frame; NULL = identity */,
                   const sicp_map_merge_params* p /* NULL = defaults */, sicp_map_merge_info* info /* nullable */);

/* ---- the map's exact contents: save, reload, inspect ---------------------------------
 * sicp_map_get_state: the rows in ascending key -- sicp_map_extract's default order, so the `row` outputs of sicp_map_carve and
 * sicp_map_raycast index them -- as they are stored: key[r], sums[3 r ..] = sx sy sz, count[r], hist[(num_classes + 1) r ..].
 * n_rows (nullable) is always written.  An array (each nullable, `capacity` rows) is written when it is non-NULL and
 * capacity >= n_rows; a non-NULL array with a smaller capacity gives SICP_ERR_INVALID_ARGUMENT and nothing else happens (the
 * merge's capacity rule: call once without arrays to size them).  hist on a map with num_classes = 0 is refused.  The map is
 * not modified.
 * sicp_map_set_state: the map's contents become exactly these n rows; n = 0 clears the map.  Every row is checked before the
 * map changes (the spare set, one swap).  SICP_ERR_INVALID_ARGUMENT with the offending row's index in sicp_map_last_error
 * and the map unchanged: keys that do not ascend strictly; a key no point can have (the top bit set, or one of the three 21-bit
 * fields 0); a count of 0; a sum that is not finite; with classes, a histogram row that does not add up to its count (integrate
 * and merge keep that equality); more than 2^31 - 1 rows or 2^32 - 1 points; a NULL key, sums or count with n > 0; hist NULL
 * with num_classes > 0 or non-NULL with num_classes = 0.  leaf_size and num_classes are creation parameters and the caller's to
 * store beside the arrays.  A map filled by set_state(get_state()) gives the same bytes from every later call as the original. */
int sicp_map_get_state(sicp_map m, int64_t capacity, uint64_t* key, double* sums /* 3 per row: sx sy sz */, uint32_t* count,
                       uint32_t* hist /* (num_classes+1) per row */, int64_t* n_rows /* every pointer nullable */);
int sicp_map_set_state(sicp_map m, int64_t n, const uint64_t* key, const double* sums, const uint32_t* count,
                       const uint32_t* hist /* required iff num_classes > 0 */);

/* ---- a database of scan descriptors: which earlier scan is this one? ---------------
 * The step of loop closing that comes before sicp_evaluate (accept the pose) and sicp_pose_covariance (weigh the edge): every
 * keyframe's scan becomes a polar descriptor of R rings x S sectors about the sensor, one uint8 code per cell -- the cell's
 * dominant label (SICP_PLACE_LABEL) or its highest height level (SICP_PLACE_HEIGHT) -- and the database of them lives on the
 * device.  A query compares a new scan's descriptor with every entry at every one of the S sector shifts, exactly and in
 * integers, and returns the best entries with the yaw between the scans.  Contracts as for sicp_map: every call is
 * synchronous; a database lives on one device and serves one thread at a time; a handle on another device is refused; every
 * refusal leaves the database byte for byte what it was; buffers come from the arena (sicp_set_memory_limit applies); it has
 * its own last-error string.  No device floating point beyond rule 3's three operations and rule 4's height level, no float
 * atomics: every launch shape gives the same bytes, and two databases driven alike are byte-identical.  The rules:
 *  1. Points.  The finite points the slot holds, whatever the handle's mode and device layout.  No pose is applied: a
 *     descriptor lives in the sensor's own frame.  d = p - (float)sensor_origin per axis in float; d2 = dx*dx + dy*dy in float,
 *     each operation rounded.  A point is kept when (double)d2 < edge2[R] and (double)d2 >= min_range * min_range.  Every
 *     result is a count or a maximum of integers: point order plays no part.
 *  2. Tables, formed once on the host in double with libm and uploaded (sicp_place_tables hands them back):
 *     edge2[i] = b*b with b = (double)i * (max_range / (double)R), i = 0..R; cos_half[j] = cos(a), sin_half[j] = sin(a) with
 *     a = (double)j * (6.283185307179586 / (double)S), j = 0..S/2-1.
 *  3. Cell.  ring = the number of i in 1..R-1 with (double)d2 >= edge2[i].  lower = !(dy > 0 || (dy == 0 && dx > 0));
 *     (x', y') = lower ? (-dx, -dy) : (dx, dy), in double; sector = the number of j in 1..S/2-1 with
 *     cos_half[j]*y' - sin_half[j]*x' >= 0 (two products and a difference, each rounded, no contraction), plus S/2 when lower.
 *     The counts are the definition: no atan2, no sqrt, no search that assumes the predicate monotone in j.
 *  4. Code of a cell, one uint8, 0 = empty; the descriptor is desc[ring*S + sector].
 *     LABEL: a cloud without labels is refused.  A kept point with label 0 or a label in `ignore` takes no part; a kept point
 *     with a label above num_classes gives SICP_ERR_BAD_LABEL and nothing changes.  The code is the most frequent label of the
 *     cell's remaining points, ties to the smallest label; the cell is empty when fewer than min_cell_points remain.
 *     HEIGHT: labels are not read.  t = ((double)dz - z_min) * (1.0 / z_step), the reciprocal formed on the host;
 *     level = t < 0 ? 0 : t >= 254 ? 254 : (int)floor(t); the code is 1 + the largest level of the cell's kept points; the cell
 *     is empty when fewer than min_cell_points kept points fall in it.
 *  5. Score of a query q against an entry e at shift s in 0..S-1: with q_c = q[r*S + c] and e_c = e[r*S + (c + s) % S], match
 *     counts the cells with q_c == e_c != 0 and either the cells with q_c != 0 || e_c != 0.  a/b beats c/d when a*d > c*b in
 *     integers; either = 0 scores 0.  An entry's best shift has the largest score, ties to the smallest shift; entries rank by
 *     best score, largest first, ties to the smallest id.  (either <= 16384: two different scores differ by at least 2^-28, so
 *     floor(match * 2^30 / either) is an exact integer sort key -- the one the device sorts by.)
 *  6. Query.  The entries searched are first .. first+count-1 (count = -1: to the end; a loop-closure caller leaves the most
 *     recent scans out this way).  The output holds the first top_k ranked entries whose host-side score >= min_score, n_found
 *     says how many; only min(top_k, count) rows per query come back from the device.  An empty range or database: SICP_OK and
 *     n_found = 0.  sicp_place_query is sicp_place_describe followed by sicp_place_query_descriptors with n_q = 1, bit for bit,
 *     and every row of a multi-query call equals its lone call.
 *  7. Meaning of the shift.  When the query's sensor is the entry's sensor turned by psi about z, the best shift is
 *     round(psi / (2 pi / S)) mod S up to cell-boundary effects, and [0, 0, sin(yaw/2), cos(yaw/2), 0, 0, 0] is the init_qt
 *     that takes the query (source) onto the entry (target).
 *  8. Refused with SICP_ERR_INVALID_ARGUMENT, the reason in sicp_place_last_error, nothing written: NULLs; parameters outside
 *     the ranges below; num_classes = 0 with LABEL; an ignored label outside 1..num_classes; a bad `which`; an origin that is
 *     not finite; top_k < 1; min_score NaN; first < 0 or a range beyond the size; n < 1 or n_q < 1; a descriptor byte above
 *     num_classes in a LABEL database (the text names the byte); more than 2^31 - 1 entries; a handle on another device.
 *     SICP_ERR_NOT_READY: the slot holds no cloud.  SICP_ERR_OUT_OF_MEMORY: the arena refused growth; the entries already held
 *     stay.  The handle is never modified.
 * Not built: an approximate pre-filter (the search is exhaustive by design), translation-augmented descriptors, removal of
 * single entries, a stream entry point, C++ class shims, a pose-graph solver. */
enum { SICP_PLACE_LABEL = 0, SICP_PLACE_HEIGHT = 1 };
#define SICP_PLACE_MAX_IGNORE 64
typedef struct sicp_place_ctx* sicp_place;
typedef struct sicp_place_params {
  int32_t n_rings;          /* R, 1..64.  default 20 */
  int32_t n_sectors;        /* S, a multiple of 4 in 4..256.  default 60 */
  double max_range;         /* finite, > 0.  default 40 */
  double min_range;         /* >= 0 and < max_range.  default 0 */
  int32_t channel;          /* SICP_PLACE_LABEL (default) / SICP_PLACE_HEIGHT */
  int32_t num_classes;      /* LABEL: 1..255 (labels 1..C; 0 = unlabelled); default 0 = must be set.  HEIGHT: ignored */
  double z_min, z_step;     /* HEIGHT: level 0 starts at z_min; z_step finite, > 0, 1 / z_step finite.  defaults -2.0, 0.5 */
  int32_t min_cell_points;  /* a cell with fewer kept points is empty.  default 1, >= 1 */
  int32_t n_ignore;         /* LABEL: 0..SICP_PLACE_MAX_IGNORE */
  uint32_t ignore[SICP_PLACE_MAX_IGNORE]; /* labels (each in 1..C) whose points are dropped: moving classes */
} sicp_place_params;
typedef struct sicp_place_candidate {
  int32_t id, shift;        /* entry (0-based, in order of insertion) and its best shift */
  int32_t match, either;    /* the two integer counts of rule 5 at that shift */
  double score;             /* (double)match / (double)either on the host; 0 when either = 0 */
  double yaw;               /* shift * (2 pi / S) wrapped to (-pi, pi]: the rotation about z, query frame -> entry frame */
} sicp_place_candidate;
typedef struct sicp_place_describe_info {
  int64_t n_in;             /* finite points of the slot */
  int64_t n_kept;           /* ... of which rule 1 keeps */
  int32_t n_cells;          /* non-empty cells of the descriptor */
  int32_t reserved_;
  double t_total_ms;        /* host wall clock */
} sicp_place_describe_info;
int sicp_default_place_params(sicp_place_params* p);
int sicp_place_create(int device_id, const sicp_place_params* p, sicp_place* out);
int sicp_place_destroy(sicp_place db);
int sicp_place_clear(sicp_place db);  /* no entries; the buffers stay */
int sicp_place_size(sicp_place db, int64_t* n_entries);
const char* sicp_place_last_error(sicp_place db);
/* The descriptor of slot `which` of h about sensor_origin: desc (R*S bytes) and info are written on success only. */
int sicp_place_describe(sicp_place db, sicp_handle h, int which, const double sensor_origin[3] /* NULL = 0 0 0 */,
                        uint8_t* desc /* nullable */, sicp_place_describe_info* info /* nullable */);
/* describe + append: *id is the new entry's number */
int sicp_place_add(sicp_place db, sicp_handle h, int which, const double sensor_origin[3] /* NULL = 0 0 0 */, int32_t* id,
                   uint8_t* desc /* nullable */, sicp_place_describe_info* info /* nullable */);
/* n descriptors of R*S bytes each appended as they are (reload a saved database); first_id (nullable): the first one's number */
int sicp_place_add_descriptors(sicp_place db, int32_t n, const uint8_t* desc, int32_t* first_id);
/* entries first .. first+count-1 (count = -1: to the end) into desc, count*R*S bytes (save the database) */
int sicp_place_get(sicp_place db, int32_t first, int32_t count, uint8_t* desc);
/* out: top_k candidates, the first *n_found of which are written */
int sicp_place_query(sicp_place db, sicp_handle h, int which, const double sensor_origin[3] /* NULL = 0 0 0 */, int32_t first,
                     int32_t count, int32_t top_k, double min_score, sicp_place_candidate* out, int32_t* n_found);
/* n_q queries at once: out is n_q*top_k candidates, row q starting at out + q*top_k with its first n_found[q] written */
int sicp_place_query_descriptors(sicp_place db, int32_t n_q, const uint8_t* desc /* n_q*R*S */, int32_t first, int32_t count,
                                 int32_t top_k, double min_score, sicp_place_candidate* out, int32_t* n_found /* n_q */);
/* test hook: the tables of rule 2; cos_half and sin_half hold S/2 doubles, edge2 R+1 (each nullable) */
int sicp_place_tables(sicp_place db, double* cos_half, double* sin_half, double* edge2);

/* ---- pose graph: the trajectory moved by the loop closures, on the device -------- */
/* A graph of poses that lives on the device between calls.  Calls are synchronous, on the graph's device, from one thread at
 * a time; the buffers come from the arena (sicp_set_memory_limit applies).  No float atomics: two graphs driven alike hold
 * the same bytes.
 *
 *  1. Node i is a pose T_i, qt[7] = [qx qy qz qw tx ty tz] (node -> world), with a `fixed` flag.  An edge (i, j, z, Omega)
 *     measures z ~ T_i^-1 T_j: what sicp_align returns with node j's scan as the source and node i's as the target.  Omega is the
 *     6x6 information matrix (row-major) in the tangent space of z under the right perturbation z * exp(delta),
 *     delta = [upsilon; omega]: the inverse of sicp_pose_covariance's `covariance` is Omega, without any conversion.  Either
 *     order of i and j and duplicate edges are allowed; i == j is refused.
 *  2. r = log(z^-1 T_i^-1 T_j), s = r^T Omega r, cost = 1/2 sum rho(s): rho(s) = s (SICP_GRAPH_LOSS_NONE) or
 *     cauchy_a^2 log(1 + s / cauchy_a^2) (SICP_GRAPH_LOSS_CAUCHY).  The robust weight w = rho'(s) multiplies Omega in the normal
 *     equations (iteratively reweighted least squares, no second-order corrector).  The Jacobians are exact under
 *     T <- T * exp(delta): dr/d delta_j = Jr^-1(r), dr/d delta_i = -Jr^-1(r) Ad(T_j^-1 T_i).
 *  3. sicp_graph_optimize: Levenberg-Marquardt with the step control of the registration's inner solve.  Each step solves
 *     (H + D / radius) delta = -g, D = diag(H) clipped to [min_lm_diagonal, max_lm_diagonal], by conjugate gradients with a
 *     block-Jacobi preconditioner, to |residual| <= cg_eta |g| or max_cg_iterations; the host reads one record per
 *     cg_check_every iterations.  A step is accepted when (cost - candidate cost) / model decrease > min_relative_decrease;
 *     then radius /= max(1/3, 1 - (2 rho - 1)^3), otherwise radius /= decrease_factor, which doubles.  A breakdown of the
 *     linear solve (a non-finite value, p^T A p <= 0, a diagonal block that is not positive definite) or a non-finite
 *     candidate cost is an invalid step: handled like a rejection and counted against max_consecutive_invalid_steps.  The run
 *     ends on: max |g| <= gradient_tolerance; an accepted step whose relative cost decrease <= function_tolerance;
 *     |delta| <= parameter_tolerance (|x| + parameter_tolerance); max_iterations; radius < min_radius; the invalid steps.
 *     All of these return SICP_OK with the code in info; the graph holds the last accepted poses.  A fixed node, and a node
 *     without edges, keep their pose's bytes through every call.
 *  4. Refused with SICP_ERR_INVALID_ARGUMENT, the reason in sicp_graph_last_error, nothing written and the graph byte for byte
 *     what it was: NULLs; n < 1 or m < 1; a pose or z that is not finite or whose quaternion's norm differs from 1 by more than
 *     1e-6 (accepted quaternions are stored normalised); an edge end outside the nodes or i == j; an Omega that is not finite,
 *     asymmetric by more than 1e-9 of its largest entry (otherwise (Omega + Omega^T) / 2 is stored) or not positive definite
 *     (Cholesky on the host); a range beyond the size; parameters outside their ranges; more than 2^31 - 1 nodes or edges.
 *     SICP_ERR_NOT_READY: sicp_graph_optimize without a fixed node or without an edge (with priors and flags: rule 10).
 *     SICP_ERR_OUT_OF_MEMORY: the arena refused; the graph holds what it held.
 *  5. A pose prior (k, z, Omega), sicp_graph_add_priors with SICP_GRAPH_PRIOR_POSE: r = log(z^-1 T_k), a 6-vector in the tangent
 *     of z exp(delta); s = r^T Omega r; rho and w from the graph's loss, 1/2 rho(s) in the cost.  dr / d delta_k = Jr^-1(r) = J:
 *     the block w J^T Omega J, the gradient w J^T Omega r.  By definition this is node j's half of an ordinary edge
 *     (i, k, z, Omega) whose node i is fixed at the identity pose, so Omega may be the inverse of a sicp_graph_marginals block of
 *     an earlier session, with no conversion.  z and Omega are checked as sicp_graph_add_edges checks them (rule 4).
 *  6. A position prior (k, p, Omega3), SICP_GRAPH_PRIOR_POSITION: r = t_k - p in the world frame, a 3-vector; s = r^T Omega3 r
 *     under the same loss.  dr / d delta_k = [R_k | 0] (3x6), exact under T exp(delta) because t' = t + R V(omega) upsilon: the
 *     block is w [[R^T Omega3 R, 0], [0, 0]], the gradient w [R^T Omega3 r; 0].  p must be finite; Omega3 is checked like
 *     Omega, at size 3.
 *  7. Enabled flags.  Every edge and every prior is created enabled.  A disabled one contributes nothing to the cost, to any
 *     node's block or gradient, to the products of the linear solves, or to the anchoring of rule 11; it keeps its id.
 *     sicp_graph_errors and sicp_graph_prior_errors still report its chi2, residual and weight at the current poses: that is
 *     how a caller sees that an edge has become consistent and can be switched on again.  `cost` of sicp_graph_errors,
 *     sicp_graph_prior_errors and sicp_graph_linearize is one number: over the enabled edges and the enabled priors.  Setting a
 *     flag to the value it has changes nothing.
 *  8. Order of sums.  A node's 42 sums start from 0, add its enabled edge records in ascending (edge id, side), then its enabled
 *     prior records in ascending prior id: a disabled entry is left out of the node's list.  The cost's partial sums run over
 *     the edges in id order, then the priors in id order; there a disabled entry counts as +0.0 at its place.  No float atomics:
 *     two graphs driven alike hold the same bytes, and with no priors and every edge enabled every call returns the bytes it
 *     returned before priors and flags existed.
 *  9. A prior on a fixed node counts in the cost, like an edge between two fixed nodes, and contributes nothing else: the
 *     block stays the identity, the gradient 0.  A node without enabled edges and without enabled priors is "a node without
 *     edges" of the rules above in every call: a zero block, a zero gradient, a pose whose bytes survive sicp_graph_optimize.
 * 10. sicp_graph_optimize is SICP_ERR_NOT_READY unless there is at least one enabled edge or enabled prior, and at least one
 *     fixed node or one enabled prior of either kind (the damping carries what a position prior leaves undetermined).  A graph
 *     without priors and with every edge enabled is refused exactly when rule 4 refuses it.
 * 11. Covariance queries (next section): H includes the priors' blocks; components are taken over the enabled edges only; a
 *     component is anchored when it holds a fixed node or a node with an enabled POSE prior.  Position priors never anchor a
 *     query: one or two of them leave a rotation free, and "a singular system is never iterated" must keep holding.  The
 *     caller fixes a node or adds a weak pose prior.
 * 12. Further refusals (as rule 4): a kind other than the two; a prior's node outside the graph; m < 1; NULLs (the outputs of
 *     sicp_graph_counts and of the two error calls, cost apart, are nullable); a range of flags beyond the count; more than
 *     2^31 - 1 priors.  SICP_ERR_OUT_OF_MEMORY from the arena leaves the graph as it was.  sicp_graph_clear also drops the
 *     priors; sicp_graph_size keeps its meaning.
 *     Not built: physical removal or renumbering of edges; per-edge loss parameters; switchable-constraint variables; position
 *     priors as anchors of covariance queries; gravity or heading-only priors; incremental (iSAM-style) updates. */
enum { SICP_GRAPH_PRIOR_POSE = 0, SICP_GRAPH_PRIOR_POSITION = 1 };
enum { SICP_GRAPH_LOSS_NONE = 0, SICP_GRAPH_LOSS_CAUCHY = 1 };
enum {
  SICP_GRAPH_GRADIENT_TOLERANCE = 0,
  SICP_GRAPH_FUNCTION_TOLERANCE = 1,
  SICP_GRAPH_PARAMETER_TOLERANCE = 2,
  SICP_GRAPH_MAX_ITERATIONS = 3,
  SICP_GRAPH_MIN_RADIUS = 4,
  SICP_GRAPH_INVALID_STEPS = 5
};
typedef struct sicp_graph_ctx* sicp_graph;
typedef struct sicp_graph_params {
  int32_t loss;                 /* SICP_GRAPH_LOSS_NONE (default) / SICP_GRAPH_LOSS_CAUCHY */
  int32_t max_iterations;       /* 100; >= 0 */
  double cauchy_a;              /* 1.0; > 0 */
  double gradient_tolerance;    /* 1e-10; >= 0 */
  double function_tolerance;    /* 1e-12; >= 0 */
  double parameter_tolerance;   /* 1e-12; >= 0 */
  double initial_radius;        /* 1e4; min_radius <= . <= max_radius */
  double min_radius;            /* 1e-32; > 0 */
  double max_radius;            /* 1e16 */
  double min_relative_decrease; /* 1e-3; in [0, 1) */
  double min_lm_diagonal;       /* 1e-6; > 0 */
  double max_lm_diagonal;       /* 1e32; >= min_lm_diagonal */
  int32_t max_consecutive_invalid_steps; /* 5; >= 1 */
  int32_t max_cg_iterations;    /* 500; >= 1 */
  double cg_eta;                /* 0.1; in (0, 1) */
  int32_t cg_check_every;       /* 8; >= 1 */
  int32_t reserved_;
} sicp_graph_params;
typedef struct sicp_graph_info {
  int32_t iterations;           /* outer iterations (linear solves) */
  int32_t accepted_steps;
  int32_t rejected_steps;
  int32_t invalid_steps;
  int32_t cg_iterations;        /* of all linear solves */
  int32_t termination;          /* SICP_GRAPH_GRADIENT_TOLERANCE ... */
  double initial_cost;
  double final_cost;
  double gradient_max_norm;     /* at the final poses */
  double radius;                /* the trust region's, at the end */
} sicp_graph_info;
int sicp_default_graph_params(sicp_graph_params* p);
int sicp_graph_create(int device_id, const sicp_graph_params* p, sicp_graph* out);
int sicp_graph_destroy(sicp_graph g);
int sicp_graph_clear(sicp_graph g);  /* no nodes, no edges, no priors; the buffers stay */
int sicp_graph_size(sicp_graph g, int64_t* n_nodes, int64_t* n_edges);
const char* sicp_graph_last_error(sicp_graph g);
/* n poses qt[7n]; fixed[n] (NULL: none fixed); first_id (nullable): the first new node's id, the rest follow */
int sicp_graph_add_nodes(sicp_graph g, int32_t n, const double* qt, const uint8_t* fixed, int32_t* first_id);
/* m edges: ends i[m], j[m], measurements z[7m], information matrices omega[36m]; first_id nullable */
int sicp_graph_add_edges(sicp_graph g, int32_t m, const int32_t* i, const int32_t* j, const double* z, const double* omega,
                         int32_t* first_id);
/* m priors of one kind on nodes node[m].  POSE: z[7m], omega[36m].  POSITION: z[3m] (a point in the world frame), omega[9m].
 * first_id (nullable): the first new prior's id, the rest follow; priors have ids of their own, from 0 */
int sicp_graph_add_priors(sicp_graph g, int32_t kind, int32_t m, const int32_t* node, const double* z, const double* omega,
                          int32_t* first_id);
/* the enabled flags of the edges / the priors first .. first + count (rule 7); a nonzero byte is "enabled" */
int sicp_graph_set_edges_enabled(sicp_graph g, int32_t first, int32_t count, const uint8_t* enabled);
int sicp_graph_get_edges_enabled(sicp_graph g, int32_t first, int32_t count, uint8_t* enabled);
int sicp_graph_set_priors_enabled(sicp_graph g, int32_t first, int32_t count, const uint8_t* enabled);
int sicp_graph_get_priors_enabled(sicp_graph g, int32_t first, int32_t count, uint8_t* enabled);
/* per prior at the current poses, each nullable: chi2[P], residual[6P] (a POSITION prior writes r in the first 3 and 0.0 in the
 * other 3), weight[P]; cost = the graph's whole cost */
int sicp_graph_prior_errors(sicp_graph g, double* chi2, double* residual, double* weight, double* cost);
int sicp_graph_counts(sicp_graph g, int64_t* n_nodes, int64_t* n_edges, int64_t* n_edges_enabled, int64_t* n_priors,
                      int64_t* n_priors_enabled); /* each nullable */
int sicp_graph_set_poses(sicp_graph g, int32_t first, int32_t count, const double* qt);
int sicp_graph_get_poses(sicp_graph g, int32_t first, int32_t count, double* qt);
int sicp_graph_set_fixed(sicp_graph g, int32_t first, int32_t count, const uint8_t* fixed);
/* per edge at the current poses, a disabled one too: chi2[M] = s, residual[6M] = r, weight[M] = w (each nullable), and the
 * cost (rule 7).  A false loop closure shows as a large chi2; sicp_graph_set_edges_enabled takes it out. */
int sicp_graph_errors(sicp_graph g, double* chi2, double* residual, double* weight, double* cost);
/* inspection: the gradient[6N] and the diagonal blocks[36N] of the normal equations at the current poses (each nullable),
 * and the cost.  A fixed node has the identity block and a zero gradient, a node without edges a zero block (rule 9). */
int sicp_graph_linearize(sicp_graph g, double* gradient, double* diag_blocks, double* cost);
int sicp_graph_optimize(sicp_graph g, sicp_graph_info* info);

/* ---- pose-graph covariances: blocks of H^-1 for gating a loop closure before it enters the graph -------- */
/* What the graph itself knows about a node, or about the relative pose of two nodes, at the current poses: the question to ask
 * before sicp_graph_add_edges (an edge that passed the gate wrongly can still be switched off: sicp_graph_set_edges_enabled),
 * and the drift that sets a search radius.  With priors and enabled flags, rule 11 of the section above says what H holds, what
 * a component is and what anchors it; where the rules below say "edges" they mean enabled edges, and a node with an enabled
 * pose prior counts as anchored.
 *
 *  1. H is the undamped Gauss-Newton matrix at the current poses: exactly what sicp_graph_linearize reports, robust weights
 *     included; a fixed node's block is the identity and its couplings are dropped.  The call linearises and gathers first.  It
 *     leaves poses, edges and parameters byte for byte as they were, and a later sicp_graph_optimize returns the bytes it
 *     returns on a twin graph that never made the call.
 *  2. sicp_graph_marginals: cov[q] is the 6x6 block (H^-1)[k, k], k = nodes[q], row-major, in the tangent space of
 *     T_k <- T_k exp(delta), delta = [upsilon; omega].  A fixed node answers exact zeros with status OK.
 *  3. sicp_graph_relative_covariances: cov[q] is the covariance of z = T_a^-1 T_b under z exp(delta) -- the convention of an
 *     edge's Omega, so inv(cov[q] + Sigma_measured) gates the residual log(z_graph^-1 z_measured) with no conversion.  To first
 *     order delta_z = delta_b - Ad(T_b^-1 T_a) delta_a: J has the block -Ad(T_b^-1 T_a) at a and I at b, cov = J H^-1 J^T, found
 *     from the six columns of H X = J^T as J X.  A fixed end contributes no block; both ends fixed: zeros, status OK.
 *  4. Every block is written as (S + S^T) / 2.
 *  5. The call returns SICP_OK when it ran; status[q] says what became of query q:
 *       SICP_GRAPH_COV_OK             the six columns met |r| <= tolerance |b|
 *       SICP_GRAPH_COV_NOT_CONVERGED  max_cg_iterations was reached; the block of the last iterate is returned
 *       SICP_GRAPH_COV_UNANCHORED     the query names a free node without edges, or one whose connected component holds no fixed
 *                                     node: NaN.  Found on the host before any solve (a singular system is never iterated)
 *       SICP_GRAPH_COV_BREAKDOWN      a non-finite value or p^T H p <= 0 in the query's columns, or a diagonal block of H that is
 *                                     not positive definite: NaN
 *     Inside the solve a free node without edges has an identity block, so it cannot disturb another query's columns.
 *     The solve: conjugate gradients with the block-Jacobi preconditioner on max_columns right-hand sides in lock step (the
 *     matrix is read once per iteration for all of them); more queries run as further passes.  max_cg_iterations = 0 means
 *     20 x the node count, at least 200 (at 1e-10 a ring needs 5-10 x its node count, a short ill-conditioned chain 13 x).  The host reads one record per check_every
 *     iterations.  max_columns = 0 means 24; either is lowered to what the queries need and, by halving down to 6, to what the
 *     arena's limit leaves room for.
 *  6. Refused with SICP_ERR_INVALID_ARGUMENT, the reason in sicp_graph_last_error, nothing written: NULL nodes, a, b or cov;
 *     n < 1; an index outside the nodes; a == b; parameters outside their ranges (a max_columns that is not a multiple of 6
 *     among them).  SICP_ERR_OUT_OF_MEMORY: not even a six-column pass fits the arena's limit; nothing written, the graph
 *     untouched.
 *  7. A query's 36 doubles and its status are the same bytes asked alone, with any other queries, in any order and at any
 *     max_columns, and two graphs driven alike return the same bytes: every column has its own scalars and is frozen when it is
 *     done, and no sum's order depends on the company.  info describes the call as a whole and does depend on it. */
enum { SICP_GRAPH_COV_OK = 0, SICP_GRAPH_COV_NOT_CONVERGED = 1, SICP_GRAPH_COV_UNANCHORED = 2, SICP_GRAPH_COV_BREAKDOWN = 3 };
typedef struct sicp_graph_cov_params {
  double tolerance;           /* 1e-10; in (0, 1): a column is done when |r| <= tolerance |b| */
  int32_t max_cg_iterations;  /* 0 = automatic (rule 5); otherwise >= 1 */
  int32_t check_every;        /* 32; >= 1: iterations enqueued between two reads of the device record */
  int32_t max_columns;        /* 0 = automatic (rule 5); otherwise a multiple of 6: columns solved in one pass */
  int32_t reserved_;
} sicp_graph_cov_params;
typedef struct sicp_graph_cov_info {
  int32_t passes;
  int32_t cg_iterations;      /* summed over the passes (a pass counts its longest column) */
  int32_t n_ok, n_failed;     /* queries with status OK / any other status */
  double worst_relative_residual; /* max |r| / |b| over the columns that were solved */
} sicp_graph_cov_info;
int sicp_default_graph_cov_params(sicp_graph_cov_params* p);
int sicp_graph_marginals(sicp_graph g, const sicp_graph_cov_params* p /* NULL = defaults */, int32_t n, const int32_t* nodes,
                         double* cov /* 36 n, row-major */, int32_t* status /* n, nullable */, sicp_graph_cov_info* info /* nullable */);
int sicp_graph_relative_covariances(sicp_graph g, const sicp_graph_cov_params* p /* NULL = defaults */, int32_t n, const int32_t* a,
                                    const int32_t* b, double* cov /* 36 n */, int32_t* status /* nullable */,
                                    sicp_graph_cov_info* info /* nullable */);

/* test / bench hook: the keypoints of cloud `which` with their normals, FPFH features and feature-radius
 * neighbour lists (CSR: nbr_offsets[n + 1], nbr_idx sorted by (d^2, index)).  Counts are always written; an output
 * array is written when it is non-NULL and its capacity (points / neighbour entries) suffices, otherwise the call
 * answers SICP_ERR_INVALID_ARGUMENT.  xyz3: n*3, normal3: n*3 (NaN with < 3 neighbours), fpfh33: n*33 (NaN likewise). */
int sicp_bootstrap_keypoints(sicp_handle h, int which, const sicp_bootstrap_params* p, int32_t capacity,
                             int64_t nbr_capacity, int32_t* n_keypoints, int64_t* n_nbrs, float* xyz3,
                             double* normal3, float* fpfh33, int64_t* nbr_offsets, int32_t* nbr_idx);
/* test / bench hook: the hypotheses of n caller-supplied samples (keypoint indices of both clouds, nr_samples per
 * hypothesis, row-major), scored as sicp_bootstrap scores its own: M12 n*12 (rows 0..2 of the 4x4 matrix, nullable),
 * err n.  feat_knn (nullable, n_source_keypoints * k_correspondences): the feature neighbours of every source
 * keypoint, target keypoint indices, -1 where there are fewer or the keypoint has no feature. */
int sicp_bootstrap_score(sicp_handle h, const sicp_bootstrap_params* p, int32_t n, const int32_t* src_idx,
                         const int32_t* tgt_idx, double* M12, double* err, int32_t knn_capacity, int32_t* feat_knn);
/* test / bench hooks of sicp_bootstrap_semantic.  keypoints: the keypoints of cloud `which` under p and lp and their
 * voted labels (xyz3 n*3, label n; the count is always written, an array when it is non-NULL and capacity suffices).
 * score: sicp_bootstrap_score under lp -- feat_knn holds the label-restricted rows when match_same_label is set, err the
 * label-aware errors when score_same_label is. */
int sicp_bootstrap_semantic_keypoints(sicp_handle h, int which, const sicp_bootstrap_params* p,
                                      const sicp_bootstrap_label_params* lp, int32_t capacity, int32_t* n_keypoints,
                                      float* xyz3, uint32_t* label);
int sicp_bootstrap_semantic_score(sicp_handle h, const sicp_bootstrap_params* p, const sicp_bootstrap_label_params* lp,
                                  int32_t n, const int32_t* src_idx, const int32_t* tgt_idx, double* M12, double* err,
                                  int32_t knn_capacity, int32_t* feat_knn);

/* ---- test / bench hooks: the individual stages -------------------------------- */
/* ComputeCovariances (em_icp.hpp:270-343 = gicp.hpp:177-239 =
 * semantic_point_cloud.hpp:25-84) for one cloud.  Any output may be NULL.
 * cov9: n*9 row-major 3x3; normal3: n*3; hist: n*C uint8 neighbour counts
 * (the reference's double histogram is count * (1/k) accumulated, em_icp.hpp:301);
 * nn_idx: n*k_cov neighbour indices. */
int sicp_covariances(sicp_handle h, int which, double* cov9, double* normal3, uint8_t* hist,
                     int32_t* nn_idx);
/* transform + nearestKSearch + gate (+ EM weight) at pose qt, i.e. the
 * correspondence loop em_icp.hpp:46-108.  idx: n_source*K target indices
 * (-1 = gated out), d2: n_source*K float32 squared distances, w: n_source*K
 * weights (prob; 1 for non-EM).  Any output may be NULL; results stay on the
 * device for sicp_accumulate. */
int sicp_correspondences(sicp_handle h, const double qt[7], int32_t* idx, float* d2, double* w);
/* one evaluation sweep of the inner solve at pose qt over the current
 * correspondences: out28 = [H upper-triangular 21 | g 6 | cost], H = sum rho1 J J^T,
 * g = sum rho1 r J, cost = 1/2 sum rho0 (what ceres::Evaluator produces from
 * GICPCostFunction::Evaluate gicp_cost_function.h:27-73 through the losses). */
int sicp_accumulate(sicp_handle h, const double qt[7], double out28[28]);
/* the same sweep for n handles in ONE launch (the kernel sicp_align_batch runs): qt n*7,
 * out28 n*28.  The launch is issued `repeat` (>= 1) times back to back between two HIP
 * events on handles[0]'s stream; kernel_ms (nullable) = event time / repeat. */
int sicp_accumulate_batch(sicp_handle* handles, int32_t n, const double* qt, double* out28,
                          int32_t repeat, double* kernel_ms);
/* the search kernels of n handles as sicp_align_batch launches them (one job per handle and label
 * segment, up to 8 jobs per launch), issued `repeat` times back to back between two HIP events on
 * handles[0]'s stream; kernel_ms (nullable) = event time / repeat, for all n searches together.
 *   what = 0: the correspondence search at poses qt (n*7): transform + K nearest targets + gate
 *             (em_icp.hpp:46-65); use_hint = 0 starts every walk from the curve position like the first
 *             search of an align(), 1 from the handle's previous result like the later ones
 *   what = 1 / 2: the k_cov self-search of the source / target cloud (em_icp.hpp:283-296)
 *   what = 3: what = 0 as an EM-ICP align() launches it after its first flush of features: the search writes the slots' EM
 *             weights in its epilogue (em_icp.hpp:77-89,108; K = 4, at most 16 classes), or a weight kernel follows once
 * The handles end up as after sicp_correspondences / sicp_covariances. */
int sicp_search_batch(sicp_handle* handles, int32_t n, const double* qt, int32_t what, int32_t use_hint,
                      int32_t repeat, double* kernel_ms);
/* the inner ceres::Solve (em_icp.hpp:162-177) on the current correspondences */
int sicp_solve(sicp_handle h, const double init_qt[7], double out_qt[7], int32_t* lm_iters,
               int32_t* evals, double* final_cost);

/* the device build of csrc/se3.hpp (what the device-resident LM step runs in place of Sophus,
 * local_parameterization_se3.h:17-25), one lane per item; op and layouts:
 *   SICP_SE3_EXP  in n*6 tangents [upsilon; omega]      -> out n*7 poses
 *   SICP_SE3_LOG  in n*7 poses                          -> out n*6
 *   SICP_SE3_PLUS in n*13 = pose (7) | delta (6)        -> out n*7 = pose * exp(delta)
 *   SICP_SE3_MUL  in n*14 = pose a (7) | pose b (7)     -> out n*7
 *   SICP_SE3_INV  in n*7                                -> out n*7
 * and the device build of csrc/lm.hpp (the inner ceres::Solve's step control, em_icp.hpp:162-177), one wavefront per item:
 *   SICP_LM_SEQUENCE           in n*679 = start pose (7) | 24 evaluations x 28 sums [H upper 21 | g 6 | cost], fed in turn to
 *                              the trust-region machine (csrc/lm.hpp, default options) AS THE KERNELS RUN IT -- by a whole
 *                              wavefront, the finite test by ballot -- until it stops or the sequence ends
 *                              -> out n*37 = pose 7 | x 7 | diag 6 | scale 6 | radius, cost, model change, decrease factor,
 *                              |x| | status, iterations, evaluations, invalid steps, reuse_diagonal, phase
 *   SICP_LM_SEQUENCE_ONE_LANE  the same in the one-lane form the host loop runs: the two must agree bit for bit on ANY
 *                              sequence (the machine is a pure function of state and evaluation) */
enum { SICP_SE3_EXP = 0, SICP_SE3_LOG = 1, SICP_SE3_PLUS = 2, SICP_SE3_MUL = 3, SICP_SE3_INV = 4, SICP_LM_SEQUENCE = 5, SICP_LM_SEQUENCE_ONE_LANE = 6 };
int sicp_se3_device(sicp_handle h, int op, int32_t n, const double* in, double* out);

/* counters accumulated since the last sicp_align() began (the hooks above add to them) */
int sicp_get_stats(sicp_handle h, sicp_stats* stats);

int sicp_synchronize(sicp_handle h);

#ifdef __cplusplus
}
#endif
#endif /* SICP_H_ */
