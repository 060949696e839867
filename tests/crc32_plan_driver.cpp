// crc32_plan_driver.cpp -- prints the standalone CRC32 pass's launch plan (plan_crc32, kernels.hpp) of
// libcfsec.so for tests/test_crc32_geometry.py.  Host only: nothing is launched, no device is opened.
//
// Reads "len n affine total" lines from standard input and prints one record per line:
//   <len> <n> <affine> <total> <tiles> <groups> <tpw> <pw> <slots> <per_launch> <ends>
// <ends>: ','-joined end offsets of the workgroups.
#include <cstdio>

#include "kernels.hpp"

int main() {
  unsigned long long len, total;
  int n, affine;
  while (std::scanf("%llu %d %d %llu", &len, &n, &affine, &total) == 4) {
    const cfsec::Crc32Plan p = cfsec::plan_crc32((size_t)len, n, affine != 0, (uint32_t)total);
    std::printf("%llu %d %d %llu %u %u %u %u %d %d ", len, n, affine, total, p.tiles, p.groups, p.tpw, p.pw, p.slots,
                p.per_launch);
    for (size_t g = 0; g < p.end.size(); ++g) std::printf("%s%lld", g ? "," : "", (long long)p.end[g]);
    std::printf("\n");
  }
  return 0;
}
