// crc_route_driver.cpp -- prints the fused product + checksum routing table of libcfsec.so for
// tests/test_crc_route.py.  Host only: it plans reconstructs (RSEngine::plan_reconstruct, which needs
// no device), fills MatVecJobs with dummy pointers (only their nullness is read) and asks the
// library's routing predicates; nothing is launched and no shard memory is allocated.
//
//   crc_route_driver rs:N:M ... lrc:N:M:L:AZ:PUTQUORUM ...
//   crc_route_driver matvec rs:N:M ... lrc:... gen:K:M ...     (the plans of launch_matvec, below)
//   crc_route_driver plan                                      (the fused launches' plans, below)
//
// Output, one record per line:
//   L <len> <nst0> <nst1> <nst2>                       the lengths and the stripe counts of each
//   rs <N> <M> <data_only> <erased,...> <k> <m> <coef hex> <cells>
//   lrc <N> <M> <L> <AZ> <k> <m> <coef hex> <plain_matches> <cells> <plain cells>
// <cells>: for cin in (0, 1), for every length, for every stripe count, three characters: the route
// (0 none, 1 bit-sliced, 2 lookup, 3 v_perm), matvec_crc_accepts, bs_crc_takes.  lrc records carry
// the cin = 1 half only, then one bs_plain_takes character per (length, stripe count).
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "engine.hpp"

namespace cfsec {  // gf_launch.hpp (device-side includes keep that header out of a host build)
bool bs_crc_takes(const MatVecJob& job, int crc_stride, const int* slot);
bool bs_plain_matches(int k, int m, const uint8_t* coef);
bool bs_plain_takes(const MatVecJob& job);
}  // namespace cfsec

using namespace cfsec;

namespace {

const uint64_t kLens[] = {1, 2048, 2049, 512ull << 20, (512ull << 20) + 1, 0xFFFFFFFFull - 4096};
constexpr int kNLens = 6, kNStripes = 3;

// 1, 5 and the smallest count that puts 2 KiB tiles x stripes over 2^32 - 1 (INT_MAX where no int does)
int stripes(uint64_t len, int i) {
  if (i == 0) return 1;
  if (i == 1) return 5;
  const uint64_t tiles = (len + 2047) / 2048;
  return (int)std::min<uint64_t>(INT_MAX, 0xFFFFFFFFull / tiles + 1);
}

const uint8_t* const kDummyIn[1] = {nullptr};
uint8_t* const kDummyOut[1] = {nullptr};

MatVecJob make_job(int k, int m, const uint8_t* coef, uint64_t len, int nst) {
  MatVecJob job;
  job.k = k;
  job.m = m;
  job.coef = coef;
  job.len = (size_t)len;
  job.nstripes = nst;
  job.in = kDummyIn;
  job.out = kDummyOut;
  return job;
}

std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s.empty() ? "-" : s;
}

// the cells of one (matrix, slots) over the lengths and stripe counts
std::string cells(int k, int m, const uint8_t* coef, int stride, const std::vector<int>& slot) {
  std::string s;
  for (int li = 0; li < kNLens; ++li)
    for (int si = 0; si < kNStripes; ++si) {
      const MatVecJob job = make_job(k, m, coef, kLens[li], stripes(kLens[li], si));
      s += (char)('0' + (int)matvec_crc_route(job, stride, slot.data()));
      s += matvec_crc_accepts(job, stride, slot.data()) ? '1' : '0';
      s += bs_crc_takes(job, stride, slot.data()) ? '1' : '0';
    }
  return s;
}

// ---- "matvec" as the first argument: the plans of launch_matvec (plan_matvec) instead of the
// checksum routes, for tests/test_matvec_route.py.  Records:
//   mat <id> <tag> <k> <m> <coef hex>       tag: enc, rec, rep, fused, gen
//   mv <id> <mode> <nstore> <len> <layout> <nstripes> <error> <steps>
// <steps>: ';'-joined "family,bs,mode,r0,mc,c0,kc,s0,ns,off,prefix,tail,affine,M,OS,threads,B,E,tile,gx,gy"
// ('-' when there are none).  Row addresses are synthesised and never dereferenced.
bool g_matvec = false;
std::set<std::string> g_seen;
int g_next_id = 0;

const uint64_t kMvLens[] = {1,    15,   16,   17,   2047, 2048, 2049, 4096, 4097, 0xFFFFFFFFull - 4096, 0xFFFFFFFFull - 4095,
                            (512ull << 20) + 1};
// (cap1x: cap1 with a visitor that reports every table launch as failed: the dispatcher's one fallback)
const char* const kLayouts[] = {"one", "aff", "aff1", "cap", "cap1", "cap1x", "far", "lens33", "lens2p32"};
struct StepLog {
  std::string out;
  bool refuse_table;
};

hipError_t print_step(MatVecStep& s, void* ctx) {
  StepLog& log = *static_cast<StepLog*>(ctx);
  std::string& out = log.out;
  if (s.bs == BsPrefix::kTable && log.refuse_table) s.table_ok = false;
  char b[256];
  std::snprintf(b, sizeof b, "%s%s,%s,%d,%d,%d,%d,%d,%d,%d,%llu,%llu,%llu,%d,%d,%d,%d,%d,%d,%u,%u,%u", out.empty() ? "" : ";",
                matvec_family_name(s.family), bs_prefix_name(s.bs), (int)s.mode, s.r0, s.mc, s.c0, s.kc, s.s0, s.ns,
                (unsigned long long)s.off, (unsigned long long)s.prefix, (unsigned long long)s.tail, s.sstride != 0, s.M,
                s.OS, s.threads, s.B, s.E, s.tile, s.grid_x, s.grid_y);
  out += b;
  return hipSuccess;
}

void mv_plan(int id, int k, int m, const uint8_t* coef, MatVecMode mode, int nstore, uint64_t len, const char* layout) {
  const std::string lay = layout;
  const int cap = 288 / (std::min(k, 32) + std::min(m, 32));  // stripes one argument block holds
  const int nst = lay == "one" ? 1 : lay == "aff" || lay == "aff1" ? 2 : lay == "cap" ? cap : lay[0] == 'l' ? 33 : cap + 1;
  const uint64_t base = 0x100000000000ull, pitch = (len + 255) / 256 * 256 + 256;
  std::vector<const uint8_t*> in((size_t)nst * k);
  std::vector<uint8_t*> out((size_t)nst * m);
  for (int s = 0; s < nst; ++s)
    for (int i = 0; i < k + m; ++i) {
      uint64_t a = base + ((uint64_t)s * (k + m) + i) * pitch;
      if (lay == "aff1" && i == 1) a += 1;                                 // one row 1 byte off, still affine
      if (lay != "one" && lay != "aff" && lay != "aff1") a += 256ull * s * s;  // no common stride
      if (lay == "far" && s == nst - 1) a += 8ull << 30;                   // the rows span >= 4 GiB
      if (i < k) in[(size_t)s * k + i] = reinterpret_cast<const uint8_t*>(a);
      else out[(size_t)s * m + i - k] = reinterpret_cast<uint8_t*>(a);
    }
  std::vector<uint64_t> lens;
  if (lay[0] == 'l') {
    for (int s = 0; s < nst; ++s) lens.push_back(s % 3 == 0 ? len : len / 2 + (uint64_t)(s & 1));
    if (lay == "lens2p32") lens[5] = 1ull << 32;
  }
  MatVecJob job;
  job.k = k;
  job.m = m;
  job.coef = coef;
  job.len = lens.empty() ? (size_t)len : 0;
  job.lens = lens.empty() ? nullptr : lens.data();
  job.nstripes = nst;
  job.in = in.data();
  job.out = out.data();
  job.mode = mode;
  job.nstore = nstore;
  job.flags = reinterpret_cast<uint32_t*>(base - 4096);
  StepLog log{"", lay == "cap1x"};
  const hipError_t e = plan_matvec(job, print_step, &log);
  const std::string& steps = log.out;
  std::printf("mv %d %d %d %llu %s %d %d %s\n", id, (int)mode, nstore, (unsigned long long)len, layout, nst, (int)e,
              steps.empty() ? "-" : steps.c_str());
}

// every mode x length x layout for the named matrices; for the (thousands of) reconstruct matrices
// two lengths, two modes and one layout, and for every 64th of them ("rep") every mode and layout at
// three lengths
void mv_matrix(const char* tag, int k, int m, const uint8_t* coef) {
  if (m == 0) return;
  const bool full = std::strcmp(tag, "rec") != 0;  // (reconstruct matrices repeat rarely: not looked up)
  if (full && !g_seen.insert(std::to_string(k) + ":" + std::to_string(m) + ":" + hex(coef, (size_t)k * m)).second) return;
  const int id = g_next_id++;
  const bool rep = !full && id % 64 == 0;
  std::printf("mat %d %s %d %d %s\n", id, rep ? "rep" : tag, k, m, hex(coef, (size_t)k * m).c_str());
  const struct { MatVecMode mode; int nstore; } modes[] = {{MatVecMode::kStore, 0}, {MatVecMode::kStoreVerify, 1},
                                                          {MatVecMode::kVerify, 0}, {MatVecMode::kStoreVerify, 0},
                                                          {MatVecMode::kStoreVerify, m}};
  for (int mi = 0; mi < (full || rep ? 5 : 2); ++mi)
    for (uint64_t len : kMvLens) {
      if (!full && len != 2049 && len != 4097 && !(rep && len == 17)) continue;
      for (const char* lay : kLayouts) {
        if (!full && !rep && std::strcmp(lay, "aff") != 0) continue;
        if (!std::strcmp(lay, "lens2p32") && len != 4097) continue;
        mv_plan(id, k, m, coef, modes[mi].mode, modes[mi].nstore, len, lay);
      }
    }
}

// ---- "plan" as the first argument: the launch plans of the fused kernels (plan_bs_crc,
// plan_matvec_crc) for tests/test_crc_plan.py, over lengths x stripe counts x layouts (aff: one stride
// between the stripes, tab: separate allocations) x resident workgroup counts (0: the query failed).
// Records (jobs outside the bit-sliced range print no bs record):
//   bs <k> <m> <len> <layout> <nstripes> <resident> <resident used> <pad> <pw0> <pw1> <pw2> <runs>
//   lk <route> <k> <m> <coef hex> <len> <layout> <nstripes> <resident> <tiles> <per> <dy> <affine> <groups> <tpw> <gx> <gy> <ends>
// <runs>: ';'-joined "n*s0,ns,tab,affine,tps,W,groups,bend,tail,tblk,grid,jump": n consecutive launches
// alike but for s0, which advances by ns.  <ends>: ','-joined end offsets of the workgroups.
struct PlanRows {
  std::vector<const uint8_t*> in;
  std::vector<uint8_t*> out;
};
PlanRows plan_rows(int k, int m, uint64_t len, int nst, bool affine) {
  PlanRows r;
  const uint64_t base = 0x100000000000ull, pitch = (len + 255) / 256 * 256 + 256;
  for (int s = 0; s < nst; ++s)
    for (int i = 0; i < k + m; ++i) {
      const uint64_t a = base + ((uint64_t)s * (k + m) + i) * pitch + (affine ? 0 : 256ull * ((s * (i + 1)) % 5));
      if (i < k) r.in.push_back(reinterpret_cast<const uint8_t*>(a));
      else r.out.push_back(reinterpret_cast<uint8_t*>(a));
    }
  return r;
}

int plans() {
  const int kNst[] = {1, 5, 6, 7, 13, 48, 1536, 65536};
  const int kResident[] = {1, 256, 768, 1024, 0};
  const int kBs[][2] = {{12, 4}, {6, 12}, {3, 3}, {16, 22}, {6, 18}};
  struct Lk { CrcRoute route; int k, m; bool enc; };  // enc: the Reed-Solomon encode rows, else a generic matrix
  const Lk kLk[] = {{CrcRoute::kLookup, 12, 4, true}, {CrcRoute::kLookup, 6, 12, false}, {CrcRoute::kLookup, 8, 2, false},
                    {CrcRoute::kVperm, 12, 4, true},  {CrcRoute::kVperm, 16, 4, true},   {CrcRoute::kVperm, 6, 6, true},
                    {CrcRoute::kVperm, 6, 12, false}, {CrcRoute::kVperm, 18, 3, false},  {CrcRoute::kVperm, 8, 4, false}};
  const auto lens = [](int k) {
    return std::vector<uint64_t>{1, 2047, 2048, 2049, 8193, 4096ull * k - 1, 4096ull * k + 1, 699051, 5592406, 512ull << 20};
  };
  for (const auto& km : kBs)
    for (uint64_t len : lens(km[0]))
      for (int nst : kNst)
        for (int aff = 0; aff < 2; ++aff) {
          if ((len + 2047) / 2048 * (uint64_t)nst > 0xFFFFFFFFull) continue;
          const PlanRows rows = plan_rows(km[0], km[1], len, nst, aff != 0);
          MatVecJob job = make_job(km[0], km[1], nullptr, len, nst);
          job.in = rows.in.data();
          job.out = rows.out.data();
          for (int res : kResident) {
            const BsCrcPlan p = plan_bs_crc(job, res);
            std::printf("bs %d %d %llu %s %d %d %d %lld %lld %lld %lld ", km[0], km[1], (unsigned long long)len,
                        aff ? "aff" : "tab", nst, res, p.resident, (long long)p.pad, (long long)p.pw[0], (long long)p.pw[1],
                        (long long)p.pw[2]);
            for (size_t i = 0; i < p.steps.size();) {
              const BsCrcStep& a = p.steps[i];
              size_t n = 1;
              for (; i + n < p.steps.size(); ++n) {
                const BsCrcStep& b = p.steps[i + n];
                if (b.s0 != a.s0 + (int)n * a.ns || b.ns != a.ns || b.tab != a.tab || b.sstride != a.sstride || b.tps != a.tps ||
                    b.W != a.W || b.groups != a.groups || b.bend != a.bend || b.tail != a.tail || b.tblk != a.tblk ||
                    b.grid != a.grid || b.jump != a.jump)
                  break;
              }
              std::printf("%s%zu*%d,%d,%u,%d,%u,%u,%u,%u,%u,%u,%u,%llu", i ? ";" : "", n, a.s0, a.ns, a.tab, a.sstride != 0, a.tps,
                          a.W, a.groups, a.bend, a.tail, a.tblk, a.grid, (unsigned long long)a.jump);
              i += n;
            }
            std::printf("\n");
          }
        }
  for (const Lk& c : kLk) {
    std::vector<uint8_t> coef((size_t)c.k * c.m);
    for (size_t i = 0; i < coef.size(); ++i) coef[i] = (uint8_t)(1 + (i * 37 + 11) % 255);
    if (c.enc) {
      std::unique_ptr<RSEngine> e;
      if (RSEngine::create(c.k, c.m, -1, &e) != CFSEC_OK) return 1;
      std::vector<bool> present(c.k + c.m, true);
      for (int i = 0; i < c.m; ++i) present[c.k + i] = false;
      ReconPlan plan;
      if (e->plan_reconstruct(present, false, &plan) != CFSEC_OK || (int)plan.outputs.size() != c.m) return 2;
      coef = plan.rows.v;
    }
    for (uint64_t len : lens(c.k))
      for (int nst : kNst)
        for (int aff = 0; aff < 2; ++aff) {
          const PlanRows rows = plan_rows(c.k, c.m, len, nst, aff != 0);
          MatVecJob job = make_job(c.k, c.m, coef.data(), len, nst);
          job.in = rows.in.data();
          job.out = rows.out.data();
          for (int res : kResident) {
            const CrcPlan p = plan_matvec_crc(job, c.route, res);
            std::printf("lk %d %d %d %s %llu %s %d %d %u %d %d %d %u %u %u %u ", (int)c.route, c.k, c.m,
                        hex(coef.data(), coef.size()).c_str(), (unsigned long long)len, aff ? "aff" : "tab", nst, res, p.tiles,
                        p.per, p.dy, p.sstride != 0, p.groups, p.tpw, p.grid_x, p.grid_y);
            for (size_t g = 0; g < p.end.size(); ++g) std::printf("%s%lld", g ? "," : "", (long long)p.end[g]);
            std::printf("\n");
          }
        }
  }
  return 0;
}

int generic(int k, int m) {
  std::vector<uint8_t> coef((size_t)k * m);
  for (size_t i = 0; i < coef.size(); ++i) coef[i] = (uint8_t)(1 + (i * 37 + 11) % 255);
  mv_matrix("gen", k, m, coef.data());
  return 0;
}

int rs_shape(int N, int M) {
  std::unique_ptr<RSEngine> e;
  if (RSEngine::create(N, M, -1, &e) != CFSEC_OK) return 1;
  const int T = N + M;
  std::vector<std::vector<int>> sets;
  // every set of 1..M shards where there are at most 3000 of them
  uint64_t count = 0, c = 1;
  for (int j = 1; j <= M; ++j) {
    c = c * (uint64_t)(T - j + 1) / (uint64_t)j;
    count += c;
  }
  if (count <= 3000) {
    for (uint32_t bits = 1; bits < (1u << T); ++bits) {
      if (__builtin_popcount(bits) > M) continue;
      std::vector<int> s;
      for (int i = 0; i < T; ++i)
        if (bits >> i & 1u) s.push_back(i);
      sets.push_back(s);
    }
  } else {
    for (int j = 1; j <= M; ++j) {  // each parity prefix (j = M: all parity)
      std::vector<int> s;
      for (int i = 0; i < j; ++i) s.push_back(N + i);
      sets.push_back(s);
    }
    for (int j = 1; j <= std::min(N, M); ++j) {  // data only
      std::vector<int> s;
      for (int i = 0; i < j; ++i) s.push_back(i);
      sets.push_back(s);
    }
    std::mt19937 rng(1000u * (uint32_t)N + (uint32_t)M);
    for (int t = 0; t < 200; ++t) {
      std::vector<int> all(T);
      for (int i = 0; i < T; ++i) all[i] = i;
      for (int i = T - 1; i > 0; --i) std::swap(all[i], all[rng() % (uint32_t)(i + 1)]);
      std::vector<int> s(all.begin(), all.begin() + 1 + (int)(rng() % (uint32_t)M));
      std::sort(s.begin(), s.end());
      sets.push_back(s);
    }
  }
  for (const auto& s : sets)
    for (int data_only = 0; data_only < 2; ++data_only) {
      std::vector<bool> present(T, true);
      for (int i : s) present[i] = false;
      ReconPlan plan;
      if (e->plan_reconstruct(present, data_only != 0, &plan) != CFSEC_OK) return 2;
      const int m = (int)plan.outputs.size();
      // the slots of RSEngine::reconstruct_crc_batch (outputs only), and with the inputs' too
      std::vector<int> slot(N + m, -1);
      for (int r = 0; r < m; ++r) slot[N + r] = plan.outputs[r];
      const uint8_t* coef = plan.rows.v.data();
      static const uint8_t none = 0;
      if (m == 0) coef = &none;  // (an empty matrix: nothing to rebuild)
      if (g_matvec) {
        mv_matrix(!data_only && (int)s.size() == M && s[0] == N ? "enc" : "rec", N, m, coef);
        continue;
      }
      std::string out = cells(N, m, coef, T, slot);
      for (int c2 = 0; c2 < N; ++c2) slot[c2] = plan.valid[c2];
      out += cells(N, m, coef, T, slot);
      std::string es;
      for (size_t i = 0; i < s.size(); ++i) es += (i ? "," : "") + std::to_string(s[i]);
      std::printf("rs %d %d %d %s %d %d %s %s\n", N, M, data_only, es.c_str(), N, m,
                  hex(plan.rows.v.data(), (size_t)m * N).c_str(), out.c_str());
    }
  return 0;
}

int lrc_mode(int N, int M, int L, int AZ, int PQ) {
  cfsec_tactic t{};
  t.n = N;
  t.m = M;
  t.l = L;
  t.az_count = AZ;
  t.put_quorum = PQ;
  std::unique_ptr<ECEncoder> enc;
  if (ECEncoder::create(t, false, 0, -1, &enc) != CFSEC_OK) return 1;
  // the fused LRC encode rows: every global and local parity shard as a row over the data
  std::vector<int> want(M + L), in(N);
  for (int i = 0; i < M + L; ++i) want[i] = N + i;
  std::vector<uint8_t> rows((size_t)(M + L) * N);
  if (enc->repair_rows(nullptr, 0, want.data(), M + L, in.data(), rows.data()) != CFSEC_OK) return 2;
  for (int i = 0; i < N; ++i)
    if (in[i] != i) return 3;
  if (g_matvec) {
    mv_matrix("fused", N, M + L, rows.data());
    return 0;
  }
  std::vector<int> slot(N + M + L);
  for (int i = 0; i < N + M + L; ++i) slot[i] = i;
  std::string plain;
  for (int li = 0; li < kNLens; ++li)
    for (int si = 0; si < kNStripes; ++si)
      plain += bs_plain_takes(make_job(N, M + L, rows.data(), kLens[li], stripes(kLens[li], si))) ? '1' : '0';
  std::printf("lrc %d %d %d %d %d %d %s %d %s %s\n", N, M, L, AZ, N, M + L, hex(rows.data(), rows.size()).c_str(),
              (int)bs_plain_matches(N, M + L, rows.data()), cells(N, M + L, rows.data(), N + M + L, slot).c_str(),
              plain.c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "plan")) return plans();
  g_matvec = argc > 1 && !std::strcmp(argv[1], "matvec");
  for (int li = 0; li < kNLens && !g_matvec; ++li)
    std::printf("L %llu %d %d %d\n", (unsigned long long)kLens[li], stripes(kLens[li], 0), stripes(kLens[li], 1),
                stripes(kLens[li], 2));
  for (int i = g_matvec ? 2 : 1; i < argc; ++i) {
    int a[5] = {0, 0, 0, 0, 0};
    int rc = 64;
    if (std::sscanf(argv[i], "rs:%d:%d", &a[0], &a[1]) == 2) rc = rs_shape(a[0], a[1]);
    else if (std::sscanf(argv[i], "lrc:%d:%d:%d:%d:%d", &a[0], &a[1], &a[2], &a[3], &a[4]) == 5)
      rc = lrc_mode(a[0], a[1], a[2], a[3], a[4]);
    else if (g_matvec && std::sscanf(argv[i], "gen:%d:%d", &a[0], &a[1]) == 2) rc = generic(a[0], a[1]);
    if (rc != 0) {
      std::fprintf(stderr, "crc_route_driver: %s failed (%d)\n", argv[i], rc);
      return 1;
    }
  }
  return 0;
}
