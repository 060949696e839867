// gf_kernels.hip -- gfx950 kernels for GF(2^8) Reed-Solomon shard coding (launcher).
//
// Replaces the CPU kernels of klauspost/reedsolomon v1.11.7 (the generated
// mulAvxTwo_RxC / mulGFNI_RxC_64 families in KRS/galois_gen_amd64.s and the
// galMulSlice[Xor] tails in KRS/galois_amd64.go:57-122) with one HBM-streaming
// kernel per output-row count.  Device code: gf_device.hpp.
//
// Arithmetic.  GF(2^8) multiplication by a constant is linear over GF(2), so a
// byte x is split into bit fields x = x[2:0] | x[5:3] | x[7:6] and
//     c*x = T0_c[x[2:0]] ^ T1_c[x[5:3]] ^ T2_c[x[7:6]]
// with 8-, 8- and 4-entry product tables.  An 8-entry byte table is exactly
// what one v_perm_b32 indexes: the two table dwords are the perm's data
// operands and the 3-bit fields (one per byte of the lane's dword) its
// selector, so one VALU op looks up 4 bytes at once.  Per (coefficient, dword)
// the cost is 3 v_perm_b32 + v_bitop3_b32 + v_xor; per input dword the 3
// selectors cost 5 ops, amortised over all outputs.  No MFMA: GF arithmetic is
// not an FP/int contraction.
//
// Data movement.  Each lane owns 16 consecutive bytes of the shard (one
// global_load_dwordx4 per input row, one global_store_dwordx4 per output row),
// so a workgroup streams whole 1 KiB-per-wave runs of every row and every byte
// of HBM is touched exactly once: read k*len, write m*len (verify: read
// (k+m)*len, write nothing).  Loads and stores are non-temporal (each byte is
// touched once).  The product tables are rebuilt per workgroup in LDS from the
// coefficient matrix carried in the kernel argument block, which keeps the
// launch free of device allocations and host->device copies (safe under
// concurrent callers and hipGraph capture).
//
// Kernel families.  plan_matvec (below) picks one per launch, plan_dy16_repair the last one; each
// line gives the condition in the order the plan tests it:
//   bit-sliced plain (gf_bs_crc.hip launch_bs_plain): a whole kStore job whose matrix is EC6P6L9's
//                or EC6P8L10's fused encode (6 x 15, 6 x 18), one length of at most 512 MiB; no chunks
//   lookup-product (gf_lut.hpp): the products of each input byte with a whole column from two LDS
//                table reads, for the shapes lut_outputs() names (EC12P9, EC15P12, EC16P20(L2)
//                repairs of 5-16 shards, non-dyadic k = 6 products)
//   16x16-dyadic (gf_dyadic16.hpp): EC16P20's 20 parity rows, EC16P20L2's 20 + 2
//   dyadic-block (gf_dyadic.hpp): 4x4 / 2x2 dyadic matrices (code-mode encodes, coset-aligned
//                repairs, fused LRC encodes with 2 plain rows)
//   fixed-K (gf_fixed.hpp, every code-mode input count k in {3,4,6,7,8,10,12,15,16,18}, m up to
//                fixed_max_m(k), shards up to 2^32 - 1 - 4096 bytes): 256-thread workgroups, 1 chunk
//                per lane, all outputs in one wave, rows pipelined 2 ahead with the issue order
//                pinned (tools/gf_pipe.hip: +6% over the runtime-k loop on EC12P4).  The three
//                families above are fixed-K shapes too, and a kStoreVerify split keeps this one
//   runtime-k (any other k, or k > 32 chunked with accumulate): policies from
//                tools/gf_variants.hip -- store/accum 256-thread, 1 chunk per lane, one row at a
//                time; verify 128-thread, 2 chunks per lane, rows loaded in pairs
// In front of the family kernel, the bit-sliced 16 + 20 network (gf_bs16.hip) takes the whole 2 KiB
// column tiles of EC16P20 / EC16P20L2 jobs with 16-byte aligned rows (bs_prefix_bytes); the family
// kernel then codes only the rows' tails:
//   encode prefix (launch_bs): a kStore run, affine or held in the argument block
//   pointer-table form (launch_bs_tab): a scattered kStore job of more stripes than one argument
//                block holds, every stripe in one launch through a device table of row offsets
//   Verify form (launch_bs16_repair, nothing missing, every row compared): an affine kVerify run
//   repair (launch_dy16_repair: launch_bs16_repair / launch_bs16_repair_tab): up to 2 missing data
//                rows in syndrome form, optionally with the stored rows' checksums; its tail, and
//                every other repair, is the 16x16-dyadic repair kernel (launch_dy16_repair_args)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gf_device.hpp"
#include "gf_launch.hpp"
#include "gf_lut_launch.hpp"
#include "kernels.hpp"

namespace cfsec {
namespace {

using dev::GfArgs;
constexpr int kStoreW = 1;
constexpr int kVerifyW = 2;

#ifndef CFSEC_SPLIT_G
#define CFSEC_SPLIT_G 1  // input rows loaded together by output-split (compute-heavy) kernels
#endif

template <int M, int OS, MatVecMode MODE>
__global__ __launch_bounds__(256) void gf_matvec_kernel(const GfArgs a) {
  constexpr int G = OS > 1 ? CFSEC_SPLIT_G : 1;
  if constexpr (MODE == MatVecMode::kVerify || MODE == MatVecMode::kStoreVerify)
    dev::matvec<M, MODE, kVerifyW, 2, false, true, true, false, false, OS>(a);
  else
    dev::matvec<M, MODE, kStoreW, G, false, true, true, false, false, OS>(a);
}

template <MatVecMode MODE>
hipError_t launch_fixed(int k, int m, const GfArgs& a, dim3 grid, hipStream_t st) {
  switch (k) {
    case 3: return launch_k<3, MODE>(m, a, grid, st);
    case 4: return launch_k<4, MODE>(m, a, grid, st);
    case 6: return launch_k<6, MODE>(m, a, grid, st);
    case 7: return launch_k<7, MODE>(m, a, grid, st);
    case 8: return launch_k<8, MODE>(m, a, grid, st);
    case 10: return launch_k<10, MODE>(m, a, grid, st);
    case 15: return launch_k<15, MODE>(m, a, grid, st);
    case 12: return launch_k<12, MODE>(m, a, grid, st);
    case 16: return launch_k<16, MODE>(m, a, grid, st);
    case 18: return launch_k<18, MODE>(m, a, grid, st);
    default: return hipErrorInvalidValue;
  }
}

template <MatVecMode MODE>
hipError_t launch_mode(Shape sh, const GfArgs& a, dim3 grid, int threads, hipStream_t st) {
#define CFSEC_CASE(MV, OSV)                                                                      \
  case MV * 8 + OSV:                                                                             \
    hipLaunchKernelGGL((gf_matvec_kernel<MV, OSV, MODE>), grid, dim3(threads), 0, st, a);        \
    break;
  switch (sh.M * 8 + sh.OS) {
    CFSEC_CASE(1, 1) CFSEC_CASE(2, 1) CFSEC_CASE(3, 1) CFSEC_CASE(4, 1) CFSEC_CASE(5, 1)
    CFSEC_CASE(6, 1) CFSEC_CASE(4, 2) CFSEC_CASE(5, 2) CFSEC_CASE(6, 2) CFSEC_CASE(4, 4)
    CFSEC_CASE(5, 4) CFSEC_CASE(6, 4) CFSEC_CASE(8, 4)
    default: return hipErrorInvalidValue;
  }
#undef CFSEC_CASE
  return hipGetLastError();
}

// The A/B switches this file reads, each once per process (bs_plain_takes reads CFSEC_BS_CRC):
//   CFSEC_LUT=0           the lookup-product shapes keep the dyadic / fixed-K kernels
//   CFSEC_BS16=0          no bit-sliced 16 + 20 kernel: no prefix of any form, no bit-sliced repair
//   CFSEC_BS_TAB=0        no pointer-table form: scattered stripes take the per-run prefix (product)
//                         or the dyadic repair kernel alone (repair)
//   CFSEC_BS_FORCE_TAB=1  repairs of affine batches go through the table launch too
// CFSEC_TRACE_MATVEC is read per call (tests turn it on mid-process).
bool env_switch(const char* name, char off, bool dflt) {
  const char* v = std::getenv(name);
  return v && v[0] == off ? !dflt : dflt;
}
const bool kLut = env_switch("CFSEC_LUT", '0', true);
const bool kBs16 = env_switch("CFSEC_BS16", '0', true);
const bool kBsTab = env_switch("CFSEC_BS_TAB", '0', true);
const bool kForceTab = env_switch("CFSEC_BS_FORCE_TAB", '1', false);
bool trace_matvec() {
  const char* v = std::getenv("CFSEC_TRACE_MATVEC");
  return v && v[0] && v[0] != '0';
}

// ---- helpers shared by the product and the repair launcher: stripe s holds K input rows
// in[s * K ..] and M output rows out[s * M ..]

// Byte distance between consecutive stripes when every stripe of the job has the same relative row
// layout (input rows c0..c0+kc, output rows r0..r0+mc); 0 otherwise.  Such a batch (e.g. stripes
// carved from one pitched HBM buffer) runs as a single launch whatever its stripe count; anything
// else is carried as an explicit pointer table, kPtrSlots per launch.
int64_t affine_stride(const uint8_t* const* in, int K, int c0, int kc, uint8_t* const* out, int M, int r0, int mc,
                      int nstripes, bool varlen) {
  if (nstripes < 2 || varlen) return 0;
  const auto addr = [](const void* p) { return (int64_t)(uintptr_t)p; };
  const int64_t ss = addr(in[K + c0]) - addr(in[c0]);
  if (ss == 0) return 0;
  for (int s = 1; s < nstripes; ++s) {
    for (int c = c0; c < c0 + kc; ++c)
      if (addr(in[(size_t)s * K + c]) != addr(in[c]) + s * ss) return 0;
    for (int r = r0; r < r0 + mc; ++r)
      if (addr(out[(size_t)s * M + r]) != addr(out[r]) + s * ss) return 0;
  }
  return ss;
}

// Every row of stripes [s0, s0 + n) is 16-byte aligned (global_load_lds and the 16-byte accesses of
// the bit-sliced kernels).  With `list`: the rows gathered there, stripe by stripe, inputs then
// outputs (the table launches' argument), and they must lie within 4 GiB (32-bit row offsets).
bool rows_fit_bs(const uint8_t* const* in, int K, uint8_t* const* out, int M, int s0, int n,
                 std::vector<const uint8_t*>* list) {
  uintptr_t bits = 0, lo = ~(uintptr_t)0, hi = 0;
  const uint8_t** dst = nullptr;
  if (list) {
    list->resize((size_t)n * (K + M));
    dst = list->data();
  }
  for (int s = s0; s < s0 + n; ++s)
    for (int i = 0; i < K + M; ++i) {
      const uint8_t* p = i < K ? in[(size_t)s * K + i] : out[(size_t)s * M + i - K];
      const uintptr_t v = reinterpret_cast<uintptr_t>(p);
      bits |= v;
      lo = std::min(lo, v);
      hi = std::max(hi, v);
      if (dst) *dst++ = p;
    }
  return !(bits & 15) && (!list || bs_tab_span_ok(lo, hi));
}
thread_local std::vector<const uint8_t*> tl_rows;  // a table step's rows, alive while it is visited

// The longest stripe of a run (the plans' one pass over lens; the dispatchers only copy slen[])
uint64_t run_len(size_t len, const uint64_t* lens, int s0, int ns) {
  if (!lens) return len;
  uint64_t llen = 0;
  for (int s = 0; s < ns; ++s) llen = std::max<uint64_t>(llen, lens[s0 + s]);
  return llen;
}

// The argument block's pointers for stripes [s0, s0 + tab): rows [c0, c0 + kc) and [r0, r0 + mc)
void fill_ptrs(GfArgs& a, const uint8_t* const* in, int K, int c0, int kc, uint8_t* const* out, int M, int r0, int mc,
               int s0, int tab) {
  for (int s = 0; s < tab; ++s) {
    for (int c = 0; c < kc; ++c) a.ptr[s * kc + c] = in[(size_t)(s0 + s) * K + c0 + c];
    for (int r = 0; r < mc; ++r) a.ptr[tab * kc + s * mc + r] = out[(size_t)(s0 + s) * M + r0 + r];
  }
}

// The bit-sliced kernel has covered the first `done` bytes of every row: the rest for the next launch
void skip_prefix(GfArgs& a, uint64_t done) {
  for (uint32_t i = 0; i < a.tab * (a.k + a.m); ++i) a.ptr[i] += done;
  a.len -= done;
}

// missing[j]: the data row that missing row j rebuilds (src[i] = 16 + j)
void missing_rows(const uint8_t* src, uint8_t* missing) {
  std::memset(missing, 0, 4);
  for (int i = 0; i < 16; ++i)
    if (src[i] >= 16) missing[src[i] - 16] = (uint8_t)i;
}

// Bytes per row that the bit-sliced 16 + 20 kernels (gf_bs16.hip) take in front of the family
// kernel: the whole 2 KiB column tiles of a job that is one chunk (`whole`) with one length, the
// network's matrix and 16-byte aligned rows; 0: none.  What differs between the three forms:
//   kEncode  a kStore run, its `tab` stripes from s0 (1: affine, the stride aligned too)
//   kVerify  a kVerify run, affine only (tab == 1; flags are there: plan_matvec has checked)
//   kTable   a scattered kStore job of more stripes than the `cap` one argument block holds, all of
//            them (s0 = 0, tab = nstripes) gathered into tl_rows and within 4 GiB
uint64_t bs_prefix_bytes(const MatVecJob& job, bool whole, MatVecMode mode, BsPrefix kind, int64_t sstride, int s0,
                         int tab, int cap = 0) {
  if (!kBs16 || !whole || job.lens || job.len < kBs16Tile) return 0;
  if (mode != (kind == BsPrefix::kVerify ? MatVecMode::kVerify : MatVecMode::kStore)) return 0;
  if (kind == BsPrefix::kVerify && tab != 1) return 0;
  if (kind == BsPrefix::kTable && (!kBsTab || sstride || job.nstripes <= cap)) return 0;
  if ((sstride & 15) || !bs_matches(job.coef, job.m, job.k)) return 0;
  if (!rows_fit_bs(job.in, job.k, job.out, job.m, s0, tab, kind == BsPrefix::kTable ? &tl_rows : nullptr)) return 0;
  return job.len / kBs16Tile * kBs16Tile;
}

const char* const kModeName[] = {"store", "accum", "verify", "store-verify"};
const char* const kFamilyName[] = {"runtime-k", "fixed-k", "dyadic", "dyadic-16", "lookup", "bs-plain"};
const char* const kPrefixName[] = {"none", "encode", "verify", "table"};

}  // namespace

const char* matvec_family_name(MatVecFamily f) { return kFamilyName[(int)f]; }
const char* bs_prefix_name(BsPrefix p) { return kPrefixName[(int)p]; }

hipError_t plan_matvec(const MatVecJob& job, MatVecVisitor visit, void* ctx) {
  using dev::kMaxK;
  using dev::kMaxM;
  if (job.k <= 0 || job.m < 0 || job.nstripes < 0 || !job.coef || !job.in || !job.out)
    return hipErrorInvalidValue;
  MatVecMode jmode = job.mode;
  if (jmode == MatVecMode::kStoreVerify) {
    if (job.nstore < 0 || job.nstore > job.m) return hipErrorInvalidValue;
    if (job.nstore == job.m) jmode = MatVecMode::kStore;
    else if (job.nstore == 0) jmode = MatVecMode::kVerify;
    else if (job.m > kMaxM) return hipErrorInvalidValue;  // the stored/compared split lives in one launch
  }
  const uint64_t maxlen = run_len(job.len, job.lens, 0, job.nstripes);
  if (job.lens && maxlen > 0xFFFFFFFFull) return hipErrorInvalidValue;  // slen[] is 32-bit
  if (job.m == 0 || job.nstripes == 0 || maxlen == 0) return hipSuccess;
  MatVecStep st{};
  // the wide LRC modes' fused encodes (EC6P6L9, EC6P8L10): one bit-sliced product instead of two passes
  // (stores beyond its tile counts, shards over 512 MiB, keep the fixed-K kernels below)
  if (jmode == MatVecMode::kStore && bs_plain_takes(job)) {
    st.mc = job.m;
    st.kc = job.k;
    st.ns = job.nstripes;
    st.mode = jmode;
    st.family = MatVecFamily::kBsPlain;  // (launch_bs_plain sizes its own grid)
    st.tail = job.len;
    return visit(st, ctx);
  }
  if ((jmode == MatVecMode::kVerify || jmode == MatVecMode::kStoreVerify) && (job.k > kMaxK || !job.flags))
    return hipErrorInvalidValue;

  for (int r0 = 0; r0 < job.m; r0 += kMaxM) {
    const int mc = std::min(kMaxM, job.m - r0);
    for (int c0 = 0; c0 < job.k; c0 += kMaxK) {
      const int kc = std::min(kMaxK, job.k - c0);
      MatVecMode mode = jmode;
      if (mode == MatVecMode::kStore && c0 > 0) mode = MatVecMode::kAccum;
      const bool verify = mode == MatVecMode::kVerify || mode == MatVecMode::kStoreVerify;
      const Shape sh = choose(mc);
      // the code-mode input counts take the fixed-K pipelined kernels (256 threads, one wave per
      // column chunk holding every output, 1 chunk per lane); anything else the runtime-k
      // kernel, whose verify policy is 128-thread workgroups with 2 chunks per lane unless the
      // outputs are split over waves
      const bool fixed = fixed_k(kc) && kc == job.k && mc <= fixed_max_m(kc) && mode != MatVecMode::kAccum &&
                         maxlen <= 0xFFFFFFFFull - 4096;  // 32-bit lane offsets
      const int threads = (!fixed && verify && sh.OS == 1) ? 128 : 256;
      // matrices of 4x4 / 2x2 dyadic blocks (encode of every code mode but the LRC local stripes,
      // coset-aligned reconstructs such as EC12P4's worst case) take the reduced-product kernel.
      // `fixed` has kc == job.k: with every row in the chunk too, job.coef is the chunk's matrix
      const bool whole = c0 == 0 && r0 == 0 && kc == job.k && mc == job.m;
      DyPlan dy{0, 0};
      bool dy16 = false;
      if (fixed && whole && mode != MatVecMode::kStoreVerify) {
        dy16 = dyadic16_plan(job.coef, mc, kc);
        if (!dy16) dy = dyadic_plan(job.coef, mc, kc);
      }
      const bool lut = kLut && fixed && lut_outputs(kc, mc, dy16 || dy.B != 0) > 0;
      st = MatVecStep{};
      st.r0 = r0, st.mc = mc, st.c0 = c0, st.kc = kc;
      st.mode = mode;
      st.family = lut      ? MatVecFamily::kLookup
                  : dy16   ? MatVecFamily::kDyadic16
                  : dy.B   ? MatVecFamily::kDyadic
                  : fixed  ? MatVecFamily::kFixedK
                           : MatVecFamily::kRuntimeK;
      st.M = sh.M, st.OS = sh.OS, st.threads = threads;
      st.B = dy.B, st.E = dy.E;
      const size_t tile = fixed ? size_t(256) * 4 * dev::fixed_lane_dwords(kc, mc)
                                : size_t(threads / sh.OS) * dev::kLaneBytes * (verify ? kVerifyW : kStoreW);
      st.tile = (uint32_t)tile;
      st.sstride = affine_stride(job.in, job.k, c0, kc, job.out, job.m, r0, mc, job.nstripes, job.lens != nullptr);
      int stripes_per_launch = st.sstride ? job.nstripes : dev::kPtrSlots / (kc + mc);
      if (job.lens) stripes_per_launch = std::min(stripes_per_launch, dev::kLenSlots);
      const size_t tiles = (maxlen + tile - 1) / tile;  // (varlen: per launch below)
      // one launch covers tiles * stripes workgroups: keep that in a 32-bit grid
      stripes_per_launch = (int)std::min<size_t>(stripes_per_launch, std::max<size_t>(1, 0x7fffffffu / tiles));
      if (fixed) stripes_per_launch = std::min(stripes_per_launch, 65535);  // grid.y = stripes
      if (tiles > 0x7fffffffu) return hipErrorInvalidValue;
      // stripes at unrelated addresses (more than one argument block holds) of the bit-sliced
      // encode shapes: one launch through a device table of row offsets for the whole 2 KiB column
      // runs (launch_bs_tab); the runs below then code only the rows' tails
      uint64_t off = 0;
      if (const uint64_t full = bs_prefix_bytes(job, whole, mode, BsPrefix::kTable, st.sstride, 0, job.nstripes,
                                                stripes_per_launch)) {
        MatVecStep t = st;
        t.ns = job.nstripes;
        t.bs = BsPrefix::kTable;
        t.prefix = full;
        t.rows = tl_rows.data();
        t.table_ok = true;
        const hipError_t e = visit(t, ctx);
        if (e != hipSuccess) return e;
        if (t.table_ok) off = full;  // else: the per-run prefix, as if the table had not been chosen
        if (off == job.len) continue;
      }
      for (int s0 = 0; s0 < job.nstripes; s0 += stripes_per_launch) {
        st.s0 = s0;
        st.ns = std::min(stripes_per_launch, job.nstripes - s0);
        const uint64_t llen = run_len(job.len, job.lens, s0, st.ns);
        if (llen == 0) continue;
        // encodes and Verifies of the bit-sliced shapes (gf_bs16.hip: EC16P20, EC16P20L2's fused
        // encode): the whole 2 KiB column runs through the network, the rest of each row through
        // the family kernel
        st.bs = mode == MatVecMode::kVerify ? BsPrefix::kVerify : BsPrefix::kEncode;
        st.off = off;
        st.prefix = off ? 0 : bs_prefix_bytes(job, whole, mode, st.bs, st.sstride, s0, st.sstride ? 1 : st.ns);
        if (!st.prefix) st.bs = BsPrefix::kNone;
        st.tail = llen - off - st.prefix;
        const size_t ltiles = (st.tail + tile - 1) / tile;
        if (lut) {
          const size_t lt = lut_tile_bytes(kc);
          st.grid_x = (uint32_t)((st.tail + lt - 1) / lt), st.grid_y = (uint32_t)st.ns;
        } else if (fixed) {  // (the dyadic launchers size grid.x themselves)
          st.grid_x = (uint32_t)ltiles, st.grid_y = (uint32_t)st.ns;
        } else {
          st.grid_x = (uint32_t)(ltiles * st.ns), st.grid_y = 1;
        }
        const hipError_t e = visit(st, ctx);
        if (e != hipSuccess) return e;
      }
    }
  }
  return hipSuccess;
}

namespace {
struct MatVecDispatch {
  const MatVecJob& job;
  hipStream_t stream;
  bool trace;
  GfArgs& a;  // the launcher's block, filled per step (left uninitialised: 3.5 KiB per call)
};

void trace_step(const MatVecStep& st) {
  std::fprintf(stderr,
               "cfsec: matvec family=%s bs=%s mode=%s k=%d m=%d r0=%d c0=%d stripes=%d prefix=%llu tail=%llu affine=%d\n",
               matvec_family_name(st.family), bs_prefix_name(st.bs), kModeName[(int)st.mode], st.kc, st.mc, st.r0, st.c0,
               st.ns, (unsigned long long)st.prefix, (unsigned long long)st.tail, st.sstride != 0);
}

// One step of the plan: fill the argument block, call the launchers the step names.
hipError_t dispatch_matvec(MatVecStep& st, void* ctx) {
  MatVecDispatch& d = *static_cast<MatVecDispatch*>(ctx);
  const MatVecJob& job = d.job;
  GfArgs& a = d.a;
  if (d.trace && st.bs != BsPrefix::kTable) trace_step(st);
  if (st.family == MatVecFamily::kBsPlain) return launch_bs_plain(job, d.stream);
  const int kc = st.kc, mc = st.mc, ns = st.ns;
  if (st.bs == BsPrefix::kTable) {
    a.flags = nullptr;
    a.pstore = a.pcmp = 0;
    // The one routing outcome decided here and not in plan_matvec: whether a device row-offset table
    // is free is known only now.  table_ok = false sends the plan back to the per-run prefix.
    const hipError_t e = launch_bs_tab(kc, mc, a, st.rows, (unsigned)ns, st.prefix, d.stream, &st.table_ok);
    if (d.trace && st.table_ok && e == hipSuccess) trace_step(st);  // (only a launch that happened)
    return e;
  }
  const int tab = st.sstride ? 1 : ns;  // stripes held in the pointer table
  a.len = st.off + st.prefix + st.tail;  // the run's longest stripe
  for (int s = 0; job.lens && s < ns; ++s) a.slen[s] = (uint32_t)job.lens[st.s0 + s];
  a.k = (uint32_t)kc;
  a.m = (uint32_t)mc;
  a.nstripes = (uint32_t)ns;
  a.tiles_per_stripe = (uint32_t)((a.len + st.tile - 1) / st.tile);
  a.flags = job.flags ? job.flags + st.s0 : nullptr;
  a.sstride = st.sstride;
  a.tab = (uint32_t)tab;
  a.nstore = (uint16_t)(st.mode == MatVecMode::kStoreVerify ? job.nstore - st.r0 : 0);
  a.varlen = job.lens ? 1 : 0;
  for (int r = 0; r < mc; ++r)
    for (int c = 0; c < kc; ++c) a.coef[r * kc + c] = job.coef[(size_t)(st.r0 + r) * job.k + (st.c0 + c)];
  fill_ptrs(a, job.in, job.k, st.c0, kc, job.out, job.m, st.r0, mc, st.s0, tab);
  hipError_t e = hipSuccess;
  if (st.bs == BsPrefix::kVerify) {  // the bit-sliced repair kernel with nothing missing, every row compared
    a.pstore = 0;
    a.pcmp = (1u << mc) - 1;
    for (int i = 0; i < 16; ++i) a.src[i] = (uint8_t)i;
    a.zw = nullptr;
    a.nzw = 0;
    e = launch_bs16_repair(0, mc - 20, nullptr, nullptr, nullptr, a, (unsigned)ns, st.prefix, d.stream);
  } else if (st.bs == BsPrefix::kEncode) {
    e = launch_bs(kc, mc, a, (unsigned)ns, st.prefix, d.stream);
  }
  if (e != hipSuccess || st.tail == 0) return e;
  if (st.off + st.prefix) {
    skip_prefix(a, st.off + st.prefix);
    a.tiles_per_stripe = (uint32_t)((a.len + st.tile - 1) / st.tile);
  }
  switch (st.family) {
    case MatVecFamily::kLookup: return launch_lut(kc, mc, st.mode, a, dim3(st.grid_x, st.grid_y), d.stream);
    case MatVecFamily::kDyadic16: return launch_dy16(mc, st.mode, a, (unsigned)ns, d.stream);
    case MatVecFamily::kDyadic:
      return kc == 6    ? launch_dy<6>(mc, st.B, st.E, st.mode, a, (unsigned)ns, d.stream)
             : kc == 12 ? launch_dy<12>(mc, st.B, st.E, st.mode, a, (unsigned)ns, d.stream)
                        : launch_dy<16>(mc, st.B, st.E, st.mode, a, (unsigned)ns, d.stream);
    default: break;
  }
  const bool fx = st.family == MatVecFamily::kFixedK;  // (never a kAccum step)
  const dim3 grid(st.grid_x, st.grid_y);
  const Shape sh{st.M, st.OS};
  using MV = MatVecMode;
  switch (st.mode) {
    case MV::kStore:
      return fx ? launch_fixed<MV::kStore>(kc, mc, a, grid, d.stream) : launch_mode<MV::kStore>(sh, a, grid, st.threads, d.stream);
    case MV::kAccum: return launch_mode<MV::kAccum>(sh, a, grid, st.threads, d.stream);
    case MV::kStoreVerify:
      return fx ? launch_fixed<MV::kStoreVerify>(kc, mc, a, grid, d.stream)
                : launch_mode<MV::kStoreVerify>(sh, a, grid, st.threads, d.stream);
    default:
      return fx ? launch_fixed<MV::kVerify>(kc, mc, a, grid, d.stream) : launch_mode<MV::kVerify>(sh, a, grid, st.threads, d.stream);
  }
}
}  // namespace

hipError_t launch_matvec(const MatVecJob& job, hipStream_t stream) {
  GfArgs a;
  MatVecDispatch d{job, stream, trace_matvec(), a};
  return plan_matvec(job, dispatch_matvec, &d);
}

namespace {
constexpr int kGatherSlots = 256;  // items and words per gather launch (argument block < 3 KiB)
struct GatherArgs {
  uint32_t* tmp;
  uint32_t* out;
  uint32_t nitems;
  uint32_t acc;
  uint32_t item[kGatherSlots];
  uint32_t word[kGatherSlots];
  uint16_t first[kGatherSlots + 1];
};

// One thread per item: OR of its tasks' words, which are reset to 0.
__global__ __launch_bounds__(kGatherSlots) void flag_gather_kernel(const GatherArgs a) {
  const uint32_t o = threadIdx.x;
  if (o >= a.nitems) return;
  uint32_t v = 0;
  for (int j = a.first[o]; j < a.first[o + 1]; ++j) {
    v |= a.tmp[a.word[j]];
    a.tmp[a.word[j]] = 0;
  }
  uint32_t* p = a.out + a.item[o];
  *p = a.acc ? (*p | (v != 0 ? 1u : 0u)) : (v != 0 ? 1u : 0u);
}
}  // namespace

namespace {
__global__ __launch_bounds__(256) void stream_copy_kernel(const dev::u32x4* __restrict__ src, dev::u32x4* __restrict__ dst,
                                                          size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}
}  // namespace

hipError_t launch_stream_copy(void* dst, const void* src, size_t bytes, hipStream_t stream) {
  if ((bytes & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15) || (bytes && (!dst || !src)))
    return hipErrorInvalidValue;
  if (bytes == 0) return hipSuccess;
  const size_t n = bytes / 16;
  // 8192 x 256 threads: tools/rot_probe.hip's flat copy (32 resident workgroups per CU)
  const unsigned grid = (unsigned)std::min<size_t>(8192, (n + 255) / 256);
  hipLaunchKernelGGL(stream_copy_kernel, dim3(grid), dim3(256), 0, stream, static_cast<const dev::u32x4*>(src),
                     static_cast<dev::u32x4*>(dst), n);
  return hipGetLastError();
}

hipError_t launch_flag_gather(uint32_t* tmp, uint32_t* out, const int* item, const int* word, int n,
                              bool accumulate, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (!tmp || !out || !item || !word) return hipErrorInvalidValue;
  GatherArgs a;
  a.tmp = tmp;
  a.out = out;
  a.acc = accumulate ? 1u : 0u;
  int j = 0;
  while (j < n) {
    // one launch: whole items only, up to kGatherSlots items and kGatherSlots words
    int ni = 0, nw = 0;
    a.first[0] = 0;
    while (j < n && ni < kGatherSlots) {
      int e = j;
      while (e < n && item[e] == item[j]) ++e;
      if (e - j > kGatherSlots) return hipErrorInvalidValue;
      if (nw + (e - j) > kGatherSlots) break;
      a.item[ni] = (uint32_t)item[j];
      for (int q = j; q < e; ++q) a.word[nw++] = (uint32_t)word[q];
      a.first[++ni] = (uint16_t)nw;
      j = e;
    }
    a.nitems = (uint32_t)ni;
    hipLaunchKernelGGL(flag_gather_kernel, dim3(1), dim3(kGatherSlots), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t plan_dy16_repair(const Dy16RepairJob& job, RepairVisitor visit, void* ctx) {
  const int nd = job.nd, ne = job.e, mo = nd + 20 + ne;
  if (nd < 0 || nd > 4 || (ne != 0 && ne != 2) || job.nstripes < 0 || !job.coef || !job.in || !job.out ||
      (job.pcmp && !job.flags) || (job.pstore | job.pcmp) >> (20 + ne))
    return hipErrorInvalidValue;
  if (job.nstripes == 0) return hipSuccess;
  const uint64_t maxlen = run_len(job.len, job.lens, 0, job.nstripes);
  if (maxlen == 0) return hipSuccess;
  if (maxlen > 0xFFFFFFFFull - 4096) return hipErrorInvalidValue;  // 32-bit lane offsets, slen[]
  RepairStep st{};
  // one stride between stripes on every row: one affine launch
  st.sstride = affine_stride(job.in, 16, 0, 16, job.out, mo, 0, mo, job.nstripes, job.lens != nullptr);
  int per = st.sstride ? std::min(job.nstripes, 65535) : dev::kPtrSlots / (16 + mo);
  if (job.lens) per = std::min(per, dev::kLenSlots);
  // the syndrome form of the bit-sliced network (gf_bs16.hip) takes the whole 2 KiB column runs of
  // 16-byte aligned rows, the dyadic repair kernel the rest of each row ...
  const bool net = job.syn && kBs16 && nd <= kBsRepairMaxNd && !job.lens && job.len >= kBs16Tile &&
                   bs_matches(job.coef, 20 + ne, 16);
  const uint64_t full = net ? job.len / kBs16Tile * kBs16Tile : 0;
  // Stripes at unrelated addresses (every shard its own buffer, as blobnode assembles a bid): the
  // bit-sliced repair over a table of 32-bit row offsets, every stripe in one step
  uint64_t off = 0;
  if (net && kBsTab && (!st.sstride || kForceTab) && job.nstripes > 1 &&
      rows_fit_bs(job.in, 16, job.out, mo, 0, job.nstripes, &tl_rows)) {
    RepairStep t = st;
    t.ns = job.nstripes;
    t.bs = RepairBs::kTable;
    t.prefix = full;
    t.rows = tl_rows.data();
    const hipError_t e = visit(t, ctx);
    if (e != hipSuccess) return e;
    off = full;
    if (off == job.len) return hipSuccess;
  }
  for (int s0 = 0; s0 < job.nstripes; s0 += per) {
    st.s0 = s0;
    st.ns = std::min(per, job.nstripes - s0);
    const uint64_t llen = run_len(job.len, job.lens, s0, st.ns);
    if (llen == 0) continue;
    const bool affine = net && !off && (st.sstride || st.ns == 1) && !(st.sstride & 15) &&
                        rows_fit_bs(job.in, 16, job.out, mo, s0, 1, nullptr);
    st.bs = affine ? RepairBs::kAffine : RepairBs::kNone;
    st.off = off;
    st.prefix = affine ? full : 0;
    st.tail = llen - off - st.prefix;
    const hipError_t e = visit(st, ctx);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

namespace {
struct RepairDispatch {
  const Dy16RepairJob& job;
  hipStream_t stream;
  bool trace, first;
  GfArgs& a;  // the launcher's block: its job-wide fields at the first step
};

// One step of the plan: the bit-sliced launch it names, then the dyadic kernel on the rows' tails.
hipError_t dispatch_repair(RepairStep& st, void* ctx) {
  RepairDispatch& d = *static_cast<RepairDispatch*>(ctx);
  const Dy16RepairJob& job = d.job;
  GfArgs& a = d.a;
  const int nd = job.nd, ne = job.e, mo = nd + 20 + ne, ns = st.ns;
  if (d.trace)
    std::fprintf(stderr, "cfsec: repair bs=%s nd=%d e=%d s0=%d stripes=%d prefix=%llu tail=%llu affine=%d\n",
                 st.bs == RepairBs::kTable ? "table" : st.bs == RepairBs::kAffine ? "affine" : "none", nd, ne, st.s0,
                 ns, (unsigned long long)st.prefix, (unsigned long long)st.tail, st.sstride != 0);
  if (d.first) {  // what every launch of the (validated) job shares
    d.first = false;
    a.k = 16;
    a.m = (uint32_t)mo;
    a.sstride = st.sstride;
    a.nstore = 0;
    a.pstore = job.pstore;
    a.pcmp = job.pcmp;
    a.zw = job.zero_words;
    a.nzw = job.nzero;
    a.varlen = job.lens ? 1 : 0;
    std::memcpy(a.src, job.src, 16);
    std::memcpy(a.coef, job.coef, (size_t)(20 + ne + nd) * 16);
  }
  a.flags = job.flags ? job.flags + st.s0 : nullptr;
  if (st.bs != RepairBs::kTable) {
    a.len = st.off + st.prefix + st.tail;
    for (int s = 0; job.lens && s < ns; ++s) a.slen[s] = (uint32_t)job.lens[st.s0 + s];
    a.nstripes = (uint32_t)ns;
    a.tab = (uint32_t)(st.sstride ? 1 : ns);
    fill_ptrs(a, job.in, 16, 0, 16, job.out, mo, 0, mo, st.s0, (int)a.tab);
  }
  hipError_t e = hipSuccess;
  if (st.bs != RepairBs::kNone) {
    uint8_t missing[4];
    missing_rows(job.src, missing);
    bool ok = true;  // (the 4 GiB span, which the plan has checked)
    e = st.bs == RepairBs::kTable
            ? launch_bs16_repair_tab(nd, ne, missing, job.prow, job.ainv, a, st.rows, (unsigned)ns, st.prefix,
                                     d.stream, &ok)
            : launch_bs16_repair(nd, ne, missing, job.prow, job.ainv, a, (unsigned)ns, st.prefix, d.stream);
    if (e == hipSuccess && !ok) e = hipErrorInvalidValue;  // (not reached: rows_fit_bs has used the launcher's span test)
  }
  if (e == hipSuccess && st.tail) {
    if (st.off + st.prefix) skip_prefix(a, st.off + st.prefix);
    e = launch_dy16_repair_args(nd, ne, a, (unsigned)ns, d.stream);
  }
  a.zw = nullptr;  // the first launch zeroed them
  a.nzw = 0;
  return e;
}
}  // namespace

hipError_t launch_dy16_repair(const Dy16RepairJob& job, hipStream_t stream) {
  GfArgs a;
  RepairDispatch d{job, stream, trace_matvec(), true, a};
  return plan_dy16_repair(job, dispatch_repair, &d);
}

}  // namespace cfsec
