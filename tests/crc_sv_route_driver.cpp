// crc_sv_route_driver.cpp -- prints the library's route, accepts and launch plan of kStoreVerify jobs
// (Reconstruct + Verify with every row checksummed, gf_crc_sv_kernel) for tests/test_crc_sv_route.py.
// Host only: links libcfsec.so, launches nothing.
//
// Arguments: lengths.  For every k, m, nstore and variant it prints one line per length and stripe
// layout:
//   sv <k> <m> <nstore> <variant> <len> <layout> <nst> <route> <accepts> <tiles> <per> <dy> <sstride>
//      <groups> <tpw> <grid_x> <grid_y> <end count> <end[0]> <end[last]> <sum of end>
// variant: full (every slot set, one length, flags), skip (slot[0] = -1), lens (per-stripe lengths),
// noflags (flags NULL), store (the same job as kStore: the control).
// layout: one (1 stripe), affine (5 stripes at one pitch), table (20 stripes, no common stride).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels.hpp"

using namespace cfsec;

int main(int argc, char** argv) {
  std::vector<uint64_t> lens;
  for (int i = 1; i < argc; ++i) lens.push_back(std::strtoull(argv[i], nullptr, 10));
  const int ks[] = {3, 4, 6, 8, 10, 12, 15, 16, 18};
  const char* variants[] = {"full", "skip", "lens", "noflags", "store"};
  struct Layout {
    const char* name;
    int nst;
    bool affine;
  };
  const Layout layouts[] = {{"one", 1, true}, {"affine", 5, true}, {"table", 20, false}};
  const int64_t pitch = int64_t(1) << 33;  // past the largest length
  uint32_t flagword = 0;
  for (int k : ks)
    for (int m = 1; m <= 7; ++m)
      for (int nstore = 0; nstore <= m; ++nstore)
        for (int v = 0; v < 5; ++v)
          for (uint64_t len : lens)
            for (const Layout& lay : layouts) {
              std::vector<uint8_t> coef((size_t)k * m);
              for (size_t i = 0; i < coef.size(); ++i) coef[i] = (uint8_t)(1 + (i * 37 + 11) % 255);
              std::vector<const uint8_t*> in((size_t)lay.nst * k);
              std::vector<uint8_t*> out((size_t)lay.nst * m);
              for (int s = 0; s < lay.nst; ++s) {
                // table: the stripes' distances differ, so no stride covers them
                const int64_t base = (int64_t(1) << 40) + (int64_t)s * (k + m) * pitch + (lay.affine ? 0 : (int64_t)s * s * 4096);
                for (int c = 0; c < k; ++c) in[(size_t)s * k + c] = reinterpret_cast<const uint8_t*>(base + c * pitch);
                for (int r = 0; r < m; ++r) out[(size_t)s * m + r] = reinterpret_cast<uint8_t*>(base + (k + r) * pitch);
              }
              std::vector<uint64_t> slens((size_t)lay.nst, len);
              std::vector<int> slot(k + m);
              for (int i = 0; i < k + m; ++i) slot[i] = i;
              MatVecJob job;
              job.k = k;
              job.m = m;
              job.coef = coef.data();
              job.len = len;
              job.nstripes = lay.nst;
              job.in = in.data();
              job.out = out.data();
              job.mode = v == 4 ? MatVecMode::kStore : MatVecMode::kStoreVerify;
              job.nstore = v == 4 ? 0 : nstore;
              job.flags = v == 3 || v == 4 ? nullptr : &flagword;
              if (v == 1) slot[0] = -1;
              if (v == 2) {
                job.lens = slens.data();
                job.len = 0;
              }
              const int stride = k + m;
              const CrcRoute route = matvec_crc_route(job, stride, slot.data());
              const bool acc = matvec_crc_accepts(job, stride, slot.data());
              if (v == 2) job.len = len;  // the plan of the length the stripes share
              const CrcPlan p = plan_matvec_crc(job, route, 0);
              int64_t sum = 0;
              for (int64_t e : p.end) sum += e;
              std::printf("sv %d %d %d %s %llu %s %d %s %d %u %d %d %lld %u %u %u %u %zu %lld %lld %lld\n", k, m, nstore,
                          variants[v], (unsigned long long)len, lay.name, lay.nst, crc_route_name(route), (int)acc,
                          p.tiles, p.per, p.dy, (long long)p.sstride, p.groups, p.tpw, p.grid_x, p.grid_y, p.end.size(),
                          (long long)(p.end.empty() ? 0 : p.end.front()), (long long)(p.end.empty() ? 0 : p.end.back()),
                          (long long)sum);
            }
  return 0;
}
