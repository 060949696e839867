// gf_delta.hip -- the delta-accumulate kernels behind EncodeIdx and Update (gf_delta.hpp).
//
// One kernel family, two input modes.  A lane owns 16 consecutive bytes of every row of its stripe:
//   * it loads its bytes of the m output rows into its accumulators (the loads go out first);
//   * per column: delta mode loads old and new, XORs them and stores the difference back to old --
//     the only read of those bytes of old, by the lane that overwrites them, before it does; plain
//     mode loads the column as it stands; the difference (or the column) times the column's m
//     coefficients is folded into the accumulators (dev::mac_row: 3-bit-field v_perm_b32 lookups and
//     v_bitop3 XOR3, tables built per workgroup in LDS from the coefficients in the argument block);
//   * it stores the accumulators.
// So each byte of old, new and the outputs is read once and each byte of old and the outputs is
// written once: (3 nc + 2 m) len bytes per stripe in delta mode, (nc + 2 m) len in plain mode.
//
// Outputs accumulate, so no byte may be coded twice: a row's ragged end (fewer than 16 bytes left for
// its lane) goes through byte stores of the lane's own bytes (the rule at dev::matvec's ragged end).
// The loads there are dev::ld_tail_row's one load of the row's last 16 bytes shifted down: the bytes
// below the lane's own -- a neighbour's, which it may already have rewritten -- are shifted out and
// reach no result.  Rows may start at any byte.  One wave per column chunk (OS = 1): waves sharing
// a column chunk would re-read old after another wave had rewritten it.  Stores are the compiler's
// own (non-temporal), never inline assembly (the store-data hazard, gf_device.hpp).
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "gf_delta.hpp"
#include "gf_device.hpp"

namespace cfsec {
namespace {

using dev::GfArgs;
using dev::u32x4;

// Argument block (dev::GfArgs): k = columns, m = rows, len, sstride, tab, coef (m x k), and
// ptr = [tab * k old / input columns][DELTA: tab * k new columns][tab * m output rows].
template <int M, bool DELTA>
__global__ __launch_bounds__(256) void gf_delta_kernel(const GfArgs a) {
  __shared__ u32x4 tab01[dev::kMaxK * M];
  __shared__ uint32_t tab2[dev::kMaxK * M];
  dev::build_tables<M>(a, tab01, tab2);
  __syncthreads();

  const int k = (int)a.k, m = (int)a.m;
  const uint32_t stripe = blockIdx.y;
  const size_t ts = a.sstride ? 0 : (size_t)stripe;  // affine: stripe 0's pointers plus a byte offset
  const size_t tab = a.tab;
  uint8_t* const* old = const_cast<uint8_t* const*>(a.ptr + ts * k);
  const uint8_t* const* neu = a.ptr + tab * k + ts * k;
  uint8_t* const* out = const_cast<uint8_t* const*>(a.ptr + tab * k * (DELTA ? 2 : 1) + ts * m);
  const uint64_t len = a.len;
  const uint64_t off = (uint64_t)blockIdx.x * kDeltaTile + (uint64_t)threadIdx.x * dev::kLaneBytes;
  if (off >= len) return;
  const size_t at = (size_t)((int64_t)stripe * a.sstride) + (size_t)off;

  u32x4 acc[M];
  if (off + dev::kLaneBytes <= len) {
#pragma unroll
    for (int r = 0; r < M; ++r) acc[r] = r < m ? dev::ld16<true>(out[r] + at) : u32x4{0u, 0u, 0u, 0u};
    for (int c = 0; c < k; ++c) {
      u32x4 x = dev::ld16<true>(old[c] + at);
      if constexpr (DELTA) {
        x ^= dev::ld16<true>(neu[c] + at);
        dev::st16<true>(old[c] + at, x);
      }
      dev::mac_row<M>(acc, x, tab01 + c * M, tab2 + c * M);
    }
#pragma unroll
    for (int r = 0; r < M; ++r)
      if (r < m) dev::st16<true>(out[r] + at, acc[r]);
  } else {
    // the row's ragged end: this lane's rem < 16 bytes, byte stores
    const size_t rem = (size_t)(len - off);
#pragma unroll
    for (int r = 0; r < M; ++r) acc[r] = r < m ? dev::ld_tail_row(out[r] + at, rem, len) : u32x4{0u, 0u, 0u, 0u};
    for (int c = 0; c < k; ++c) {
      u32x4 x = dev::ld_tail_row(old[c] + at, rem, len);
      if constexpr (DELTA) {
        x ^= dev::ld_tail_row(neu[c] + at, rem, len);
        dev::st_tail(old[c] + at, x, rem);
      }
      dev::mac_row<M>(acc, x, tab01 + c * M, tab2 + c * M);
    }
#pragma unroll
    for (int r = 0; r < M; ++r)
      if (r < m) dev::st_tail(out[r] + at, acc[r], rem);
  }
}

// Accumulator rows of the shipped instantiations; a step runs on the smallest that holds its rows.
constexpr int kDeltaM[] = {1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 32};
static_assert(kDeltaM[sizeof(kDeltaM) / sizeof(kDeltaM[0]) - 1] == kDeltaMaxRows, "the largest holds a full row chunk");
static_assert(kDeltaMaxCols == dev::kMaxK && kDeltaMaxRows <= dev::kMaxM, "coef[] holds a launch's matrix");

int delta_rows(int mc) {
  for (int M : kDeltaM)
    if (M >= mc) return M;
  return 0;
}

template <bool DELTA>
hipError_t launch_rows(int M, const GfArgs& a, dim3 grid, hipStream_t st) {
#define CFSEC_CASE(MV)                                                                  \
  case MV:                                                                              \
    hipLaunchKernelGGL((gf_delta_kernel<MV, DELTA>), grid, dim3(256), 0, st, a);        \
    break;
  switch (M) {
    CFSEC_CASE(1) CFSEC_CASE(2) CFSEC_CASE(3) CFSEC_CASE(4) CFSEC_CASE(6) CFSEC_CASE(8) CFSEC_CASE(12)
    CFSEC_CASE(16) CFSEC_CASE(20) CFSEC_CASE(24) CFSEC_CASE(32)
    default: return hipErrorInvalidValue;
  }
#undef CFSEC_CASE
  return hipGetLastError();
}

// Byte distance between consecutive stripes when every stripe has the same relative layout of the
// step's rows (columns [c0, c0 + kc) of old and, in delta steps, new; rows [r0, r0 + mc)); else 0.
int64_t delta_stride(const DeltaJob& job, int c0, int kc, int r0, int mc, bool delta) {
  if (job.nstripes < 2) return 0;
  const auto addr = [](const void* p) { return (int64_t)(uintptr_t)p; };
  const int64_t ss = addr(job.old[job.nc + c0]) - addr(job.old[c0]);
  if (ss == 0) return 0;
  for (int s = 1; s < job.nstripes; ++s) {
    for (int c = c0; c < c0 + kc; ++c) {
      if (addr(job.old[(size_t)s * job.nc + c]) != addr(job.old[c]) + s * ss) return 0;
      if (delta && addr(job.neu[(size_t)s * job.nc + c]) != addr(job.neu[c]) + s * ss) return 0;
    }
    for (int r = r0; r < r0 + mc; ++r)
      if (addr(job.out[(size_t)s * job.m + r]) != addr(job.out[r]) + s * ss) return 0;
  }
  return ss;
}

bool trace_delta() {
  const char* v = std::getenv("CFSEC_TRACE_DELTA");
  return v && v[0] && v[0] != '0';
}

}  // namespace

bool delta_kernel_exists(int M) { return M > 0 && delta_rows(M) == M; }

hipError_t plan_delta(const DeltaJob& job, DeltaVisitor visit, void* ctx) {
  if (job.nc <= 0 || job.m < 0 || job.nstripes < 0 || !job.coef || !job.old || !job.out) return hipErrorInvalidValue;
  if (job.m == 0 || job.nstripes == 0 || job.len == 0) return hipSuccess;
  const uint64_t tiles = (job.len + kDeltaTile - 1) / kDeltaTile;
  if (tiles > 0x7fffffffu) return hipErrorInvalidValue;  // grid.x
  for (int c0 = 0; c0 < job.nc; c0 += kDeltaMaxCols) {
    const int kc = std::min(kDeltaMaxCols, job.nc - c0);
    for (int r0 = 0; r0 < job.m; r0 += kDeltaMaxRows) {
      DeltaStep st{};
      st.r0 = r0, st.mc = std::min(kDeltaMaxRows, job.m - r0), st.c0 = c0, st.kc = kc;
      // the chunk's first row chunk forms and stores its columns' deltas; the launches after it on the
      // stream read the rewritten columns as they stand
      st.delta = job.delta() && r0 == 0;
      st.M = delta_rows(st.mc);
      st.OS = 1;
      st.len = job.len;
      st.sstride = delta_stride(job, c0, kc, r0, st.mc, st.delta);
      st.tile = kDeltaTile;
      const int per = st.sstride ? 65535 : dev::kPtrSlots / ((st.delta ? 2 : 1) * kc + st.mc);  // grid.y / pointer slots
      for (int s0 = 0; s0 < job.nstripes; s0 += per) {
        st.s0 = s0;
        st.ns = std::min(per, job.nstripes - s0);
        st.grid_x = (uint32_t)tiles, st.grid_y = (uint32_t)st.ns;
        const hipError_t e = visit(st, ctx);
        if (e != hipSuccess) return e;
      }
    }
  }
  return hipSuccess;
}

namespace {
struct DeltaDispatch {
  const DeltaJob& job;
  hipStream_t stream;
  bool trace;
  GfArgs& a;  // filled per step (left uninitialised: 3.5 KiB per call)
};

hipError_t dispatch_delta(const DeltaStep& st, void* ctx) {
  DeltaDispatch& d = *static_cast<DeltaDispatch*>(ctx);
  const DeltaJob& job = d.job;
  GfArgs& a = d.a;
  if (d.trace)
    std::fprintf(stderr, "cfsec: delta mode=%s nc=%d m=%d r0=%d c0=%d stripes=%d s0=%d len=%llu affine=%d\n",
                 st.delta ? "delta" : "plain", st.kc, st.mc, st.r0, st.c0, st.ns, st.s0, (unsigned long long)st.len,
                 st.sstride != 0);
  const int kc = st.kc, mc = st.mc;
  const int tab = st.sstride ? 1 : st.ns;
  a.len = st.len;
  a.k = (uint32_t)kc;
  a.m = (uint32_t)mc;
  a.nstripes = (uint32_t)st.ns;
  a.tiles_per_stripe = st.grid_x;
  a.flags = nullptr;
  a.sstride = st.sstride;
  a.tab = (uint32_t)tab;
  a.nstore = 0;
  a.varlen = 0;
  for (int r = 0; r < mc; ++r)
    for (int c = 0; c < kc; ++c) a.coef[r * kc + c] = job.coef[(size_t)(st.r0 + r) * job.nc + (st.c0 + c)];
  const int outs = tab * kc * (st.delta ? 2 : 1);
  for (int s = 0; s < tab; ++s) {
    // an affine run's pointers are its first stripe's
    const size_t js = (size_t)(st.s0 + s);
    for (int c = 0; c < kc; ++c) {
      a.ptr[s * kc + c] = job.old[js * job.nc + st.c0 + c];
      if (st.delta) a.ptr[tab * kc + s * kc + c] = job.neu[js * job.nc + st.c0 + c];
    }
    for (int r = 0; r < mc; ++r) a.ptr[outs + s * mc + r] = job.out[js * job.m + st.r0 + r];
  }
  const dim3 grid(st.grid_x, st.grid_y);
  return st.delta ? launch_rows<true>(st.M, a, grid, d.stream) : launch_rows<false>(st.M, a, grid, d.stream);
}
}  // namespace

hipError_t launch_delta(const DeltaJob& job, hipStream_t stream) {
  GfArgs a;
  DeltaDispatch d{job, stream, trace_delta(), a};
  return plan_delta(job, dispatch_delta, &d);
}

}  // namespace cfsec
