// job_table.hpp -- the job-table convention of the feature calls (bootstrap, pose covariance, evaluate, merge), stated once:
// the device-side lookup of a workgroup's job, and the host-side packing of a launch's arguments into one upload.
// Plain C++: no HIP call, so the host half is tested on the CPU (tests/test_job_table_cpu.py).
#ifndef SICP_JOB_TABLE_HPP_
#define SICP_JOB_TABLE_HPP_

#include <cstddef>
#include <cstring>
#include <vector>

#ifndef SICP_HD
#define SICP_HD
#endif

namespace sicp {

// ONE launch runs the jobs (clouds, pairs, parts) of a whole group.  The jobs live in device memory, and job j owns the
// workgroups [blk_end[j - 1], blk_end[j]) of the launch: blk_end is the INCLUSIVE prefix of the per-job workgroup counts,
// built on the host.  job_of returns the job of workgroup b -- the first j with blk_end[j] > b, by bisection -- and
// *local = b's place among that job's workgroups.
//   - A job with zero workgroups stays in the table at its index (kernels and hosts that index jobs or result rows by
//     position rely on it); its blk_end equals its predecessor's, so it is never found.
//   - A workgroup never straddles two jobs: a job indexes everything from its own origin and sees exactly the workgroup
//     shapes of a launch of its own, so its results have the same bits alone and in any group.
// b must be below blk_end[nj - 1] (the launch has that many workgroups).  Wave-uniform: on the device the bisection and the
// job's fields stay in scalar registers.
SICP_HD inline int job_of(const int* blk_end, int nj, int b, int* local) {
  int lo = 0, hi = nj - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (blk_end[mid] > b) hi = mid; else lo = mid + 1;
  }
  *local = b - (lo > 0 ? blk_end[lo - 1] : 0);
  return lo;
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The layout of an argument block: typed sections one behind the other, each at a multiple of 256 bytes, for a host copy
// and a device copy of bytes() bytes each.  Where the host bytes live (pinned or pageable) is the caller's choice.
class ArgBlock {
 public:
  struct Section {
    size_t at = 0;
  };
  template <class T>
  Section add(size_t count) {
    const Section s{bytes_};
    bytes_ = up256(bytes_ + sizeof(T) * count);
    return s;
  }
  size_t bytes() const { return bytes_; }
  // (one body under two names: a call site says which copy it points into)
  template <class T>
  static T* host(Section s, void* host_base) { return reinterpret_cast<T*>(static_cast<unsigned char*>(host_base) + s.at); }
  template <class T>
  static T* dev(Section s, void* dev_base) { return reinterpret_cast<T*>(static_cast<unsigned char*>(dev_base) + s.at); }

 private:
  size_t bytes_ = 0;
};

// The common block: the jobs of one launch and the prefix of their workgroup counts.  Built job by job, then packed into a
// host copy that the caller uploads to `dev_base`.
template <class J>
class JobTable {
 public:
  int blocks = 0;  // workgroups of the launch
  void add(const J& job, long long nblocks) {
    jobs_.push_back(job);
    blocks += nblocks > 0 ? (int)nblocks : 0;
    end_.push_back(blocks);
  }
  int nj() const { return (int)jobs_.size(); }
  size_t bytes() const {
    ArgBlock b;
    b.add<J>(jobs_.size());
    b.add<int>(end_.size());
    return b.bytes();
  }
  // writes all bytes() bytes of the host copy; d_jobs() / d_end() then point into the device copy at dev_base
  void pack(void* host_base, void* dev_base) {
    ArgBlock b;
    const ArgBlock::Section sj = b.add<J>(jobs_.size()), se = b.add<int>(end_.size());
    std::memset(host_base, 0, b.bytes());
    if (!jobs_.empty()) {
      std::memcpy(ArgBlock::host<J>(sj, host_base), jobs_.data(), sizeof(J) * jobs_.size());
      std::memcpy(ArgBlock::host<int>(se, host_base), end_.data(), sizeof(int) * end_.size());
    }
    d_jobs_ = ArgBlock::dev<J>(sj, dev_base);
    d_end_ = ArgBlock::dev<int>(se, dev_base);
  }
  const J* d_jobs() const { return d_jobs_; }
  const int* d_end() const { return d_end_; }

 private:
  std::vector<J> jobs_;
  std::vector<int> end_;
  const J* d_jobs_ = nullptr;
  const int* d_end_ = nullptr;
};

}  // namespace sicp
#endif
