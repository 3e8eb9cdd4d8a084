// build_tree.h -- interface of the GPU tree build (build_tree.hip).
#ifndef SICP_BUILD_TREE_H_
#define SICP_BUILD_TREE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh.hpp"

namespace sicp {

// one segment of a cloud: the whole of a flat cloud, or one label's points (everything here is derived from point counts and
// bounding boxes on the host).  The host fills a table of these, pinned; the build uploads it and every kernel finds an
// element's segment by binary search of the begin offsets.
struct BuildSegment {
  int off, cnt;               // device-order range of the segment
  int padded;                 // cnt rounded up to whole leaves (>= one leaf)
  int pt_begin;               // first packed point
  int node_begin;             // first box
  int code_begin;             // first leaf code
  int n_leaf, top;            // the complete tree's 4^top leaves (bvh.hpp: make_levels)
  float lox, loy, loz, scale; // curve quantisation of the segment (bounding box corner, cells per metre)
};

struct BuildBuffers {
  // in: the cloud in caller order, and (a cloud grouped by label only) caller indices grouped by segment
  const float *rx, *ry, *rz;
  const uint32_t* rl;  // nullable
  const int* ids;      // nullable = identity
  // scratch
  unsigned long long *keys_in, *keys_out;
  int *vals_in, *vals_out;
  void* sort_temp;
  size_t sort_temp_bytes;
  // the segment table: filled by the caller in `h_segs` (pinned, >= 1 entry), uploaded to `d_segs` by the build
  BuildSegment* d_segs;
  const BuildSegment* h_segs;
  // out
  float *x, *y, *z;
  uint32_t* label;
  int *perm, *inv;
  float4 *pts4, *box_lo, *box_hi;
  unsigned long long* leaf_code;
};

// keys_in / keys_out / vals_in / vals_out hold ALL points (every segment sorts its own range); the sort's temporary storage
// is sized by the largest segment
size_t build_sort_temp_bytes(int max_segment_points);
hipError_t build_tree_device(const BuildBuffers& b, int n_seg, hipStream_t st);

}  // namespace sicp
#endif
