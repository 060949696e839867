// crc_route_driver.cpp -- prints the fused product + checksum routing table of libcfsec.so for
// tests/test_crc_route.py.  Host only: it plans reconstructs (RSEngine::plan_reconstruct, which needs
// no device), fills MatVecJobs with dummy pointers (only their nullness is read) and asks the
// library's routing predicates; nothing is launched and no shard memory is allocated.
//
//   crc_route_driver rs:N:M ... lrc:N:M:L:AZ:PUTQUORUM ...
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
  for (int li = 0; li < kNLens; ++li)
    std::printf("L %llu %d %d %d\n", (unsigned long long)kLens[li], stripes(kLens[li], 0), stripes(kLens[li], 1),
                stripes(kLens[li], 2));
  for (int i = 1; i < argc; ++i) {
    int a[5] = {0, 0, 0, 0, 0};
    int rc = 64;
    if (std::sscanf(argv[i], "rs:%d:%d", &a[0], &a[1]) == 2) rc = rs_shape(a[0], a[1]);
    else if (std::sscanf(argv[i], "lrc:%d:%d:%d:%d:%d", &a[0], &a[1], &a[2], &a[3], &a[4]) == 5)
      rc = lrc_mode(a[0], a[1], a[2], a[3], a[4]);
    if (rc != 0) {
      std::fprintf(stderr, "crc_route_driver: %s failed (%d)\n", argv[i], rc);
      return 1;
    }
  }
  return 0;
}
