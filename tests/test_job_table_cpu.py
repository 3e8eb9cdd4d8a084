"""CPU test of the job-table convention (csrc/job_table.hpp, compiled for the host with g++): the lookup every job-table
kernel runs per workgroup against a linear scan -- tables with zero-workgroup jobs at the front, in the middle and at the
end included -- and the layout of the argument blocks the drivers upload.  The same program also runs under the address
and undefined-behaviour sanitizers: it is host code only."""
import os
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = textwrap.dedent(
    r"""
    #include <cstdint>
    #include <cstdio>
    #include <vector>
    #include "job_table.hpp"
    using namespace sicp;

    static int fails = 0;
    #define CHECK(c) do { if (!(c)) { ++fails; std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

    // job_of for every workgroup of the table against a linear scan over the counts
    static void check_table(const std::vector<int>& cnt) {
      std::vector<int> end;
      int total = 0;
      for (int c : cnt) { total += c; end.push_back(total); }
      int b = 0;
      for (int j = 0; j < (int)cnt.size(); ++j)
        for (int l = 0; l < cnt[j]; ++l, ++b) {
          int local = -1;
          const int got = job_of(end.data(), (int)cnt.size(), b, &local);
          CHECK(got == j);
          CHECK(got >= 0 && got < (int)cnt.size() && cnt[got] > 0);
          CHECK(local == l);
        }
      CHECK(b == total);
    }

    struct Big { char bytes[200]; };
    static_assert(sizeof(Big) == 200, "a 200-byte element");

    template <class T>
    static void check_packer(size_t n0, size_t n1, size_t n2) {
      ArgBlock blk;
      const size_t n[3] = {n0, n1, n2};
      ArgBlock::Section s[3];
      for (int k = 0; k < 3; ++k) s[k] = blk.add<T>(n[k]);
      for (int k = 0; k < 3; ++k) {
        CHECK(s[k].at % 256 == 0);
        const size_t stop = s[k].at + sizeof(T) * n[k];
        CHECK(stop <= (k < 2 ? s[k + 1].at : blk.bytes()));  // no overlap with what follows
      }
      CHECK(blk.bytes() % 256 == 0);
      std::vector<unsigned char> host(blk.bytes() + 1), dev(blk.bytes() + 1);
      for (int k = 0; k < 3; ++k) {
        const T* hp = ArgBlock::host<T>(s[k], host.data());
        const T* dp = ArgBlock::dev<T>(s[k], dev.data());
        CHECK((const unsigned char*)hp - host.data() == (std::ptrdiff_t)s[k].at);
        CHECK((const unsigned char*)dp - dev.data() == (std::ptrdiff_t)s[k].at);
      }
    }

    struct Job { int id; double pad[3]; };

    int main() {
      check_table({1});
      check_table({5});
      check_table({0, 3});
      check_table({3, 0});
      check_table({0, 0, 2, 0, 0});
      check_table({2, 0, 0, 3});
      check_table({1, 1, 1, 1});
      uint64_t state = 0x9e3779b97f4a7c15ull;
      auto next = [&](int n) {  // (a 64-bit LCG: the tables are the same on every machine)
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((state >> 33) % (uint64_t)n);
      };
      for (int t = 0; t < 300; ++t) {
        std::vector<int> cnt((size_t)(1 + next(40)));
        int total = 0;
        for (int& c : cnt) { c = next(6); total += c; }
        if (total == 0) cnt[(size_t)next((int)cnt.size())] = 1 + next(5);
        check_table(cnt);
      }

      check_packer<int32_t>(1, 64, 65);
      check_packer<int32_t>(0, 3, 1000);
      check_packer<int64_t>(1, 32, 33);
      check_packer<int64_t>(7, 0, 31);
      check_packer<Big>(1, 32, 33);
      check_packer<Big>(5, 0, 64);
      {  // sections of different element sizes in one block
        ArgBlock blk;
        const ArgBlock::Section a = blk.add<Big>(3), b = blk.add<int32_t>(3), c = blk.add<int64_t>(3);
        CHECK(a.at == 0 && b.at == 768 && c.at == 1024 && blk.bytes() == 1280);
        CHECK(up256(0) == 0 && up256(1) == 256 && up256(256) == 256 && up256(257) == 512);
      }

      {  // JobTable: a zero-workgroup job keeps its index, the prefix is inclusive, the packed block holds both
        JobTable<Job> tab;
        const int cnt[5] = {2, 0, 3, 0, 0};
        for (int j = 0; j < 5; ++j) { Job job = {}; job.id = 100 + j; tab.add(job, cnt[j]); }
        CHECK(tab.nj() == 5 && tab.blocks == 5);
        CHECK(tab.bytes() % 256 == 0 && tab.bytes() >= sizeof(Job) * 5 + sizeof(int) * 5);
        std::vector<unsigned char> host(tab.bytes(), 0xff);
        tab.pack(host.data(), host.data());  // (the "device" copy is the host copy here)
        const int want_end[5] = {2, 2, 5, 5, 5};
        for (int j = 0; j < 5; ++j) {
          CHECK(tab.d_jobs()[j].id == 100 + j);
          CHECK(tab.d_end()[j] == want_end[j]);
        }
        CHECK((const unsigned char*)tab.d_jobs() == host.data());
        CHECK(((const unsigned char*)tab.d_end() - host.data()) % 256 == 0);
        CHECK((const unsigned char*)tab.d_end() >= host.data() + sizeof(Job) * 5);
        for (int b = 0; b < tab.blocks; ++b) {
          int local = -1;
          const int j = job_of(tab.d_end(), tab.nj(), b, &local);
          CHECK(j == (b < 2 ? 0 : 2) && local == (b < 2 ? b : b - 2));
        }
        std::vector<unsigned char> other(tab.bytes());
        tab.pack(host.data(), other.data());  // the device pointers follow the device base by the same offsets
        CHECK((const unsigned char*)tab.d_jobs() == other.data());
        CHECK((const unsigned char*)tab.d_end() - other.data() == (std::ptrdiff_t)up256(sizeof(Job) * 5));
      }
      std::printf("%s\n", fails ? "FAILED" : "ok");
      return fails ? 1 : 0;
    }
    """
)


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_job_table(tmp_path, flags):
    c = tmp_path / "t.cpp"
    c.write_text(CODE)
    exe = tmp_path / "t"
    subprocess.run(["g++", "-std=c++17", "-DSICP_HD=", *flags, "-I", os.path.join(ROOT, "semantic-icp_amd", "csrc"), str(c), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
