// delta_plan_driver -- prints plan_delta's launches (gf_delta.hpp) for the jobs named on the command
// line; links libcfsec.so, needs no device: the plan is a pure host function and the row addresses
// made up here are never dereferenced.
//
// An argument is nc:m:delta:len:layout:nstripes, layout one of
//   aff   stripes at one stride from each other on every row
//   aff1  the same with the last output row of the last stripe 1 byte off
//   scat  stripes at unrelated distances (stripe s a further 256 s^2 bytes on)
// One line per job: "job nc m delta len layout nstripes error steps", steps = "-" or
// delta,r0,mc,c0,kc,s0,ns,M,OS,len,affine,tile,gx,gy,exists joined by ";".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gf_delta.hpp"

namespace {
std::string g_steps;

hipError_t print_step(const cfsec::DeltaStep& st, void*) {
  char buf[256];
  std::snprintf(buf, sizeof buf, "%s%d,%d,%d,%d,%d,%d,%d,%d,%d,%llu,%d,%u,%u,%u,%d", g_steps.empty() ? "" : ";",
                st.delta ? 1 : 0, st.r0, st.mc, st.c0, st.kc, st.s0, st.ns, st.M, st.OS, (unsigned long long)st.len,
                st.sstride != 0, st.tile, st.grid_x, st.grid_y, cfsec::delta_kernel_exists(st.M) ? 1 : 0);
  g_steps += buf;
  return hipSuccess;
}
}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    int nc = 0, m = 0, delta = 0, ns = 0;
    unsigned long long len = 0;
    char layout[16] = {0};
    if (std::sscanf(argv[i], "%d:%d:%d:%llu:%15[a-z0-9]:%d", &nc, &m, &delta, &len, layout, &ns) != 6) {
      std::fprintf(stderr, "bad job %s\n", argv[i]);
      return 2;
    }
    const bool scat = !std::strcmp(layout, "scat");
    const uint64_t pitch = (len + 255) / 256 * 256 + 256;
    const int width = 2 * nc + m;  // a stripe's rows: old columns, new columns, outputs
    const auto row = [&](int s, int r) {
      return (uint8_t*)(uintptr_t)(0x100000000ull + ((uint64_t)s * width + r) * pitch + (scat ? 256ull * s * s : 0));
    };
    // (one spare entry: an empty job still hands plan_delta arrays, not NULL)
    std::vector<uint8_t*> old((size_t)ns * nc + 1), out((size_t)ns * m + 1);
    std::vector<const uint8_t*> neu((size_t)ns * nc + 1);
    for (int s = 0; s < ns; ++s) {
      for (int c = 0; c < nc; ++c) {
        old[(size_t)s * nc + c] = row(s, c);
        neu[(size_t)s * nc + c] = row(s, nc + c);
      }
      for (int r = 0; r < m; ++r) out[(size_t)s * m + r] = row(s, 2 * nc + r);
    }
    if (!std::strcmp(layout, "aff1") && ns * m > 0) out[(size_t)ns * m - 1] += 1;
    std::vector<uint8_t> coef((size_t)m * nc + 1);
    for (size_t j = 0; j < coef.size(); ++j) coef[j] = (uint8_t)(1 + j % 255);
    cfsec::DeltaJob job;
    job.nc = nc, job.m = m, job.coef = coef.data(), job.len = (size_t)len, job.nstripes = ns;
    job.old = old.data();
    job.neu = delta ? neu.data() : nullptr;
    job.out = out.data();
    g_steps.clear();
    const hipError_t e = cfsec::plan_delta(job, print_step, nullptr);
    std::printf("job %d %d %d %llu %s %d %d %s\n", nc, m, delta, len, layout, ns, (int)e,
                g_steps.empty() ? "-" : g_steps.c_str());
  }
  return 0;
}
