// prim_kernels.hip -- the rocPRIM sorts and scans of the feature calls (bootstrap, merge, pose covariance), instantiated
// here once.  All follow rocPRIM's convention: temp == nullptr asks for the temporary bytes, nothing runs.  A length
// below one is passed on as one, so that a size query always names some storage.
// (build_tree.hip keeps its own sort calls: its segment logic is part of the upload path.)
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "kernels.h"

namespace sicp {
namespace {
inline size_t prim_len(long long n) { return (size_t)(n > 0 ? n : 1); }
}  // namespace

hipError_t prim_sort_keys(void* temp, size_t& bytes, const unsigned long long* in, unsigned long long* out, long long n, int begin_bit,
                          int end_bit, hipStream_t st) {
  return rocprim::radix_sort_keys(temp, bytes, in, out, prim_len(n), (unsigned)begin_bit, (unsigned)end_bit, st);
}

hipError_t prim_sort_pairs(void* temp, size_t& bytes, const unsigned long long* kin, unsigned long long* kout, const int* vin, int* vout,
                           long long n, int begin_bit, int end_bit, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, bytes, kin, kout, vin, vout, prim_len(n), (unsigned)begin_bit, (unsigned)end_bit, st);
}

hipError_t prim_scan_int(void* temp, size_t& bytes, const int* in, int* out, long long n, hipStream_t st) {
  return rocprim::exclusive_scan(temp, bytes, in, out, 0, prim_len(n), rocprim::plus<int>(), st);
}

hipError_t prim_scan_ll(void* temp, size_t& bytes, const long long* in, long long* out, long long n, hipStream_t st) {
  return rocprim::exclusive_scan(temp, bytes, in, out, 0ll, prim_len(n), rocprim::plus<long long>(), st);
}

hipError_t prim_segmented_sort_keys(void* temp, size_t& bytes, const unsigned long long* in, unsigned long long* out, long long n,
                                    int segments, const long long* off, hipStream_t st) {
  return rocprim::segmented_radix_sort_keys(temp, bytes, in, out, (unsigned)prim_len(n), (unsigned)segments, off, off + 1, 0, 64, st);
}

}  // namespace sicp
