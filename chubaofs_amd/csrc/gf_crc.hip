// gf_crc.hip -- host side of the fused matvec + shard CRC32 kernels (device code: gf_crc.hpp).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

#include "gf_crc.hpp"
#include "gf_launch.hpp"

namespace cfsec {
namespace crcdev {
CFSEC_CRC_EXTERN(6)
CFSEC_CRC_EXTERN(8)
CFSEC_CRC_EXTERN(12)
CFSEC_CRC_EXTERN(16)
CFSEC_CRC_EXTERN(18)
CFSEC_CRC_SV_EXTERN(6)
CFSEC_CRC_SV_EXTERN(8)
CFSEC_CRC_SV_EXTERN(12)
CFSEC_CRC_SV_EXTERN(16)
CFSEC_CRC_SV_EXTERN(18)
}  // namespace crcdev

namespace {

using crcdev::GfCrcArgs;
constexpr uint32_t kX0 = 0x80000000u;    // x^0 (reflected)
constexpr uint32_t kX1 = 0x40000000u;    // x^1
constexpr uint32_t kXInv = 0xDB710641u;  // x^-1 mod P: the y with y*x = x^0 (P has a constant term)

uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t bit = kX0; bit; bit >>= 1) {
    if (a & bit) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? crcdev::kPoly : 0u);
  }
  return p;
}

// x^e mod P for any integer e (e < 0: powers of x^-1).
uint32_t xpow(int64_t e) {
  uint32_t base = e >= 0 ? kX1 : kXInv;
  uint64_t n = e >= 0 ? (uint64_t)e : (uint64_t)(-e);
  uint32_t p = kX0;
  while (n) {
    if (n & 1) p = mulmod(p, base);
    base = mulmod(base, base);
    n >>= 1;
  }
  return p;
}

std::vector<uint32_t> host_tables() {
  std::vector<uint32_t> t(crcdev::kShiftBase + crcdev::kShiftWords);
  const uint32_t k4096 = xpow(8 * 4096);
  uint32_t* nt = t.data() + crcdev::kNibTabBase;
  for (int p = 0; p < 32; ++p)  // Np[n] = f(0, 16-byte piece with nibble p = n, the rest 0)
    for (uint32_t n = 0; n < 16; ++n) {
      uint8_t piece[16] = {};
      piece[p / 2] = (uint8_t)(n << (4 * (p & 1)));
      uint32_t c = 0;
      for (uint8_t b : piece) {
        c ^= b;
        for (int i = 0; i < 8; ++i) c = (c & 1u) ? (c >> 1) ^ crcdev::kPoly : c >> 1;
      }
      nt[p * 16 + n] = c;
    }
  uint32_t* ft = t.data() + crcdev::kFiveTabBase;
  for (int w = 0; w < 5; ++w)  // Q(w, f)[e]: word w of (d0..d3, R) = e << 5f, the rest 0
    for (int f = 0; f < crcdev::kFiveFields; ++f)
      for (uint32_t e = 0; e < (f < 6 ? 32u : 4u); ++e) {
        const uint32_t v = e << (5 * f);
        uint32_t c = 0;
        if (w == 4) {
          c = mulmod(k4096, v);
        } else {
          for (int i = 0; i < 16; ++i) {
            c ^= i / 4 == w ? (v >> (8 * (i % 4))) & 0xFFu : 0u;
            for (int q = 0; q < 8; ++q) c = (c & 1u) ? (c >> 1) ^ crcdev::kPoly : c >> 1;
          }
        }
        ft[(w * crcdev::kFiveFields + f) * 32 + e] = c;
      }
  for (int j = 0; j < 256; ++j) {  // basis of shift(., 16*(255-j)) for thread j
    const uint32_t kj = xpow(8LL * 16 * (255 - j));
    for (int i = 0; i < 32; ++i) t[crcdev::kBasisBase + j * 32 + i] = mulmod(kj, 1u << i);
    t[crcdev::kShiftBase + j] = kj;
  }
  return t;
}

}  // namespace

// The lookup tables on the current device, uploaded once per device.
hipError_t crc_device_tables(const uint32_t** out) {
  static std::mutex mu;
  static std::map<int, uint32_t*> per_device;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> l(mu);
  auto it = per_device.find(dev);
  if (it == per_device.end()) {
    static const std::vector<uint32_t> host = host_tables();
    uint32_t* d = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&d), host.size() * 4);
    if (e != hipSuccess) return e;
    e = hipMemcpy(d, host.data(), host.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return e;
    }
    it = per_device.emplace(dev, d).first;
  }
  *out = it->second;
  return hipSuccess;
}

uint32_t crc_xpow(int64_t e) { return xpow(e); }
uint32_t crc_mulmod(uint32_t a, uint32_t b) { return mulmod(a, b); }

// Every stripe's rows at one byte distance from the stripe before (0: not so, or a single stripe):
// the job then goes out as one pointer set and a stride, whatever its stripe count.
int64_t job_affine_stride(const MatVecJob& job) {
  if (job.nstripes < 2) return 0;
  const auto addr = [](const void* p) { return (int64_t)(uintptr_t)p; };
  const int64_t ss = addr(job.in[job.k]) - addr(job.in[0]);
  if (ss == 0) return 0;
  for (int s = 1; s < job.nstripes; ++s) {
    for (int c = 0; c < job.k; ++c)
      if (addr(job.in[(size_t)s * job.k + c]) != addr(job.in[c]) + s * ss) return 0;
    for (int r = 0; r < job.m; ++r)
      if (addr(job.out[(size_t)s * job.m + r]) != addr(job.out[r]) + s * ss) return 0;
  }
  return ss;
}

namespace {

template <bool CIN>
int lds_per_cu(int k, int m) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, int> cache;  // (device, k * 64 + m)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> l(mu);
  const auto key = std::make_pair(dev, k * 64 + m);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int n = 0;
  switch (k) {
    case 6: n = crcdev::lds_blocks_per_cu<6, CIN>(m); break;
    case 8: n = crcdev::lds_blocks_per_cu<8, CIN>(m); break;
    case 12: n = crcdev::lds_blocks_per_cu<12, CIN>(m); break;
    case 16: n = crcdev::lds_blocks_per_cu<16, CIN>(m); break;
    default: n = 0;
  }
  cache.emplace(key, n);
  return n;
}

template <bool CIN>
hipError_t launch_crc(int k, int m, const GfCrcArgs& a, dim3 grid, hipStream_t st, int dy) {
  switch (k) {
    case 6: return crcdev::launch_crc_k<6, CIN>(m, a, grid, st, dy);
    case 8: return crcdev::launch_crc_k<8, CIN>(m, a, grid, st, dy);
    case 12: return crcdev::launch_crc_k<12, CIN>(m, a, grid, st, dy);
    case 16: return crcdev::launch_crc_k<16, CIN>(m, a, grid, st, dy);
    case 18: return crcdev::launch_crc_k<18, CIN>(m, a, grid, st, dy);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_crc_sv(int k, int m, const GfCrcArgs& a, dim3 grid, hipStream_t st) {
  switch (k) {
    case 6: return crcdev::launch_crc_sv_k<6>(m, a, grid, st);
    case 8: return crcdev::launch_crc_sv_k<8>(m, a, grid, st);
    case 12: return crcdev::launch_crc_sv_k<12>(m, a, grid, st);
    case 16: return crcdev::launch_crc_sv_k<16>(m, a, grid, st);
    case 18: return crcdev::launch_crc_sv_k<18>(m, a, grid, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

// The lookup-product fused kernel (gf_crc_lds_kernel): m <= 4, k <= 16, and (round 6) k = 6, m = 12 --
// EC6P10L2's fused LRC encode with every shard checksummed, any 6 x 12 matrix (CFSEC_CRC_LDS=0 /
// CFSEC_CRC_LDS12=0 keep the v_perm kernels for A/B, which need the 2x2-dyadic + 2 plain-row form).
static bool crc_lds_on() {
  static const bool v = env_u32("CFSEC_CRC_LDS", 1) != 0;
  return v;
}
static bool crc_lds12_on() {
  static const bool v = crc_lds_on() && env_u32("CFSEC_CRC_LDS12", 1) != 0;
  return v;
}

// Reconstruct + Verify with every row checksummed (gf_crc_sv_kernel); CFSEC_SV_CRC=0 sends those jobs
// to the product and the separate pass (A/B).
static bool crc_sv_on() {
  static const bool v = env_u32("CFSEC_SV_CRC", 1) != 0;
  return v;
}

// The one routing decision of the fused product + checksum kernels (kernels.hpp): host arithmetic on
// the job's scalars, coef, slot and the masks above, no HIP calls.
CrcRoute matvec_crc_route(const MatVecJob& job, int crc_stride, const int* slot) {
  const int k = job.k, m = job.m;
  const bool sv = job.mode == MatVecMode::kStoreVerify;
  if ((job.mode != MatVecMode::kStore && !sv) || k < 1 || m < 1 || job.len > 0xFFFFFFFFull - crcdev::kTile || !slot ||
      crc_stride <= 0 || crc_stride > 256 || job.nstripes < 0 || !job.coef || !job.in || !job.out)
    return CrcRoute::kNone;
  const bool cin = slot[0] >= 0;
  for (int i = 0; i < k + m; ++i) {
    const bool want = i >= k || cin;
    if (want && (slot[i] < 0 || slot[i] >= crc_stride)) return CrcRoute::kNone;
  }
  // Reconstruct + Verify (kStoreVerify): the v_perm kernel gf_crc_sv_kernel alone -- a stored and a
  // compared row at least, every row checksummed, one length, the Verify words given
  if (sv) {
    const bool shape = (k == 6 || k == 8 || k == 12 || k == 16 || k == 18) && m >= 2 && m <= 6;
    return crc_sv_on() && shape && job.nstore > 0 && job.nstore < m && cin && !job.lens && job.flags
               ? CrcRoute::kVperm
               : CrcRoute::kNone;
  }
  // a code mode's bit-sliced network, checksums from its bit planes (gf_bs_crc.hip): only with the
  // inputs checksummed and the tile counts in its range -- a shape nothing else covers (k = 3, 4, 10,
  // 15, m > 6) has no route otherwise
  if (bs_crc_takes(job, crc_stride, slot)) return CrcRoute::kBitSliced;
  // the kernels of gf_crc.hpp: the input counts of the code modes of SURVEY §8, m <= 6 outputs
  if (k != 6 && k != 8 && k != 12 && k != 16 && k != 18) return CrcRoute::kNone;
  if (m <= 6) return crc_lds_on() && m <= 4 && k <= 16 ? CrcRoute::kLookup : CrcRoute::kVperm;
  // EC6P10L2's fused encode (6 x (10 dyadic + 2 local) rows), instantiated with its inputs
  // checksummed only (every shard, as Put does)
  if (k == 6 && m == 12 && cin) {
    if (crc_lds12_on()) return CrcRoute::kLookup;
    const DyPlan dp = dyadic_plan(job.coef, m, k);
    if (dp.B == 2 && dp.E == 2) return CrcRoute::kVperm;
  }
  return CrcRoute::kNone;
}

const char* crc_route_name(CrcRoute r) {
  switch (r) {
    case CrcRoute::kBitSliced: return "bit-sliced";
    case CrcRoute::kLookup: return "lookup";
    case CrcRoute::kVperm: return "v_perm";
    default: return "none";
  }
}

uint32_t crc32_shift_ones(size_t len) { return mulmod(xpow(8 * (int64_t)len), 0xFFFFFFFFu) ^ 0xFFFFFFFFu; }

bool matvec_crc_accepts(const MatVecJob& job, int crc_stride, const int* slot) {
  return matvec_crc_route(job, crc_stride, slot) != CrcRoute::kNone;
}

// The launches of a lookup / v_perm job (kernels.hpp): host arithmetic only.
CrcPlan plan_matvec_crc(const MatVecJob& job, CrcRoute route, int resident) {
  CrcPlan p{};
  if ((route != CrcRoute::kLookup && route != CrcRoute::kVperm) || job.nstripes <= 0 || job.len == 0) return p;
  const int k = job.k, m = job.m;
  p.tiles = (uint32_t)((job.len + crcdev::kTile - 1) / crcdev::kTile);
  p.sstride = job_affine_stride(job);
  p.per = std::min(p.sstride ? job.nstripes : crcdev::kPtrSlots / (k + m), 65535);
  // matrices of dyadic blocks the v_perm kernel has a reduced-product form for: 4 outputs of 4x4
  // blocks (EC12P4 / EC16P4 encode, coset-aligned repairs), 6 x 6 of 2x2 blocks (EC6P6 encode);
  // 6 x 12 is EC6P10L2's fused encode + its 18 checksums (the route: that form, inputs checksummed)
  if (route == CrcRoute::kLookup) {
    p.dy = -1;
  } else if (job.mode == MatVecMode::kStoreVerify) {
    p.dy = 0;  // decode rows: the plain product
  } else if (m == 12) {
    p.dy = 2;
  } else if ((m == 4 && k % 4 == 0) || (k == 6 && m == 6)) {
    const DyPlan dp = dyadic_plan(job.coef, m, k);
    p.dy = dp.E == 0 && ((dp.B == 4 && m == 4) || (dp.B == 2 && m == 6)) ? dp.B : 0;
  }
  // Workgroups per launch.  The v_perm kernels: ~1024, each folding ~11 tiles per row before its
  // per-thread basis epilogue (16 rows x 32 columns); 512 / 2048 / 4096 were 3-7 % slower
  // (profiles/r01/crc_wgs_sweep.txt).  The lookup kernel: exactly the resident count (its 48-64 KiB
  // LDS table allows 2-3 per CU), so no second partial wave of workgroups: 768 vs 1024 for k = 12
  // is 200 vs 220 us.  CFSEC_CRC_GROUPS overrides (probes).
  static const uint32_t kGroupsEnv = env_u32("CFSEC_CRC_GROUPS", 0);
  const uint32_t total = kGroupsEnv ? kGroupsEnv : p.dy == -1 && resident > 0 ? (uint32_t)resident : 1024u;
  const uint32_t want = std::max<uint32_t>(1, total / (uint32_t)std::min(job.nstripes, p.per));
  const uint32_t fit = std::min<uint32_t>({p.tiles, want, (uint32_t)crcdev::kMaxGroups});
  p.tpw = (p.tiles + fit - 1) / fit;
  p.groups = p.grid_x = (p.tiles + p.tpw - 1) / p.tpw;
  p.grid_y = (uint32_t)std::min(job.nstripes, p.per);
  for (uint32_t g = 0; g < p.groups; ++g)
    p.end.push_back((int64_t)std::min<uint64_t>((uint64_t)(g + 1) * p.tpw, p.tiles) * crcdev::kTile);
  return p;
}

// m <= 4, k <= 16: the lookup-product kernel (gf_crc_lds_kernel; CFSEC_CRC_LDS=0 keeps the v_perm
// kernels for A/B): EC12P4 8 x 64 MiB encode + 16 checksums 225-230 -> 200 us
// (profiles/r03/crc_lds_ab*.txt).  EC6P10L2's fused LRC encode + 18 checksums (C4) on the same lookup
// kernel with 16-byte entries: C4's put batch 245 -> 211 us per call against the v_perm form
// (profiles/r06/c4_crc_lds12.txt)
hipError_t launch_matvec_crc(const MatVecJob& job, uint32_t* crc, int crc_stride, const int* slot,
                             hipStream_t stream, bool zero) {
  const CrcRoute route = crc ? matvec_crc_route(job, crc_stride, slot) : CrcRoute::kNone;
  if (route == CrcRoute::kNone) return hipErrorInvalidValue;
  const int k = job.k, m = job.m;
  const bool cin = slot[0] >= 0;
  const bool sv = job.mode == MatVecMode::kStoreVerify;
  const bool trace = env_u32("CFSEC_TRACE_CRC", 0) != 0;  // read per call: tests turn it on mid-process
  if (trace && !sv)
    std::fprintf(stderr, "cfsec: crc route=%s k=%d m=%d cin=%d stripes=%d len=%llu\n", crc_route_name(route), k, m,
                 (int)cin, job.nstripes, (unsigned long long)job.len);
  hipError_t e = zero ? hipMemsetAsync(crc, 0, sizeof(uint32_t) * (size_t)crc_stride * job.nstripes, stream)
                      : hipSuccess;
  if (e != hipSuccess || job.nstripes == 0 || job.len == 0) return e;
  if (route == CrcRoute::kBitSliced) return launch_bs_crc(job, crc, crc_stride, slot, stream);

  GfCrcArgs a{};
  e = crc_device_tables(&a.tabs);
  if (e != hipSuccess) return e;
  int resident = 0;  // the lookup kernel's workgroups on the device at once (0: not known)
  if (route == CrcRoute::kLookup) {
    const int per_cu = cin ? lds_per_cu<true>(k, m) : lds_per_cu<false>(k, m);
    int dev = 0, cus = 0;
    if (per_cu > 0 && hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
      resident = per_cu * cus;
  }
  const CrcPlan p = plan_matvec_crc(job, route, resident);
  if (trace && sv)
    std::fprintf(stderr, "cfsec: crc sv k=%d m=%d nstore=%d stripes=%d len=%llu tpw=%u groups=%u per=%d\n", k, m,
                 job.nstore, job.nstripes, (unsigned long long)job.len, p.tpw, p.groups, p.per);
  a.nstore = sv ? (uint32_t)job.nstore : 0u;
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < k; ++c) a.coef[r * k + c] = job.coef[(size_t)r * k + c];
  a.len = job.len;
  a.k = (uint32_t)k;
  a.m = (uint32_t)m;
  a.tiles = p.tiles;
  a.tpw = p.tpw;
  a.sstride = p.sstride;
  a.fin = crc32_shift_ones(job.len);
  a.crc_stride = (uint32_t)crc_stride;
  for (int i = 0; i < k + m; ++i) a.slot[i] = (uint8_t)std::max(slot[i], 0);
  for (uint32_t g = 0; g < p.groups; ++g) a.gconst[g] = xpow(8 * ((int64_t)job.len - p.end[g]));
  for (int s0 = 0; s0 < job.nstripes; s0 += p.per) {
    const int ns = std::min(p.per, job.nstripes - s0);
    const int tab = p.sstride ? 1 : ns;
    a.tab = (uint32_t)tab;
    a.crc = crc + (size_t)s0 * crc_stride;
    for (int s = 0; s < tab; ++s) {
      for (int c = 0; c < k; ++c) a.ptr[s * k + c] = job.in[(size_t)(s0 + s) * k + c];
      for (int r = 0; r < m; ++r) a.ptr[tab * k + s * m + r] = job.out[(size_t)(s0 + s) * m + r];
    }
    const dim3 grid(p.grid_x, (unsigned)ns);
    if (sv) {
      a.flags = job.flags + s0;
      e = launch_crc_sv(k, m, a, grid, stream);
      if (e != hipSuccess) return e;
      continue;
    }
    e = cin ? launch_crc<true>(k, m, a, grid, stream, p.dy) : launch_crc<false>(k, m, a, grid, stream, p.dy);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace cfsec
