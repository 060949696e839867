// gf_bs16.hip -- the EC16P20 / EC16P20L2 parity as a bit-sliced XOR network (gf_bitslice.hpp,
// bs_net_ec16p20l2.hpp): the encodes' whole 2 KiB column runs; the launcher (gf_kernels.hip) sends
// the rest of each row (and every other matrix) to the dyadic kernels.
//
// Persistent waves, 8 per CU (2 per SIMD at <= 256 VGPRs: the 128 input planes of a 32-byte column
// stay in registers).  While a wave runs the network on its tile, data rows 0-7 of its next tile
// are copied into its 16 KiB of LDS by global_load_lds (no VGPRs); rows 8-15 are loaded at the
// tile's top, where the other wave of the SIMD covers their latency.  EC16P20L2's fused encode,
// 64 x 262,144: 131.9 us against 148.6 us for the 16x16-dyadic v_perm kernel (profiles/r04/
// bs_probe.txt); it issues ~40 % fewer VALU instructions at 2 instead of 4 waves per SIMD.
// The network takes its inputs in the paired basis (gf_bitslice.hpp bs_pair_basis): each dyadic
// row pair of the 20 global rows then shares the half over the odd columns, 3262 instead of 3904
// XOR ops per 32-byte column for the 22 rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstring>
#include <mutex>

#include "bs_net_ec16p20l2.hpp"
#include "gf_bitslice.hpp"
#include "gf256.hpp"
#include "gf_launch.hpp"

namespace cfsec {

namespace {
constexpr int kBsK = 16, kBsPrefetch = 8, kBsWaves = 8;
// LDS-DMA cache policy (gf_bitslice.hpp bs_glds_row): encode default, repair non-temporal
constexpr int kBsEncGlds = 0, kBsRepGlds = 2;
// (the register loads of the rows not prefetched are non-temporal in both kernels: bs_ld_row)

// Both kernels end their tile loop with an LDS-DMA re-prefetch in flight (branch-free: the last
// tile re-reads itself).  s_endpgm does not wait for it, and once every wave of the workgroup has
// ended its 160 KiB of LDS goes to the next workgroup placed on the CU -- possibly another launch's,
// whose freshly prefetched slots the late DMA then overwrites.  Round 4's false ErrVerify (two
// processes, or two streams, repairing at once; profiles/r05/stale_dma_probe.txt) was this.  So
// every wave drains its vector memory operations before it ends.
__device__ __forceinline__ void bs_drain_exit() { __builtin_amdgcn_s_waitcnt(dev::bs_waitcnt_vm(0)); }

// Row pointer j of the repair kernel's GfArgs (its first argument, at offset 0 of the argument
// segment) by a scalar load whose offset the compiler cannot see through: the kernel names up to 40
// rows, and held across the tile loop their pointers (with the per-row conditions) outgrow the SGPRs
// -- the spilled ones come back through v_readlane, ~240 per tile.  Re-read where used, they cost a
// scalar-cache load each: the repair 1-2 % faster; the encode no faster, so it reads a.ptr plainly
// (profiles/r04/bs_reload_ab.txt).
__device__ __forceinline__ const uint8_t* bs_kernarg_ptr(uint32_t j) {
  typedef const __attribute__((address_space(4))) uint64_t ku64;
  uint32_t w = __builtin_amdgcn_readfirstlane((uint32_t)(offsetof(dev::GfArgs, ptr) / 8) + j);
  asm volatile("" : "+s"(w));
  return reinterpret_cast<const uint8_t*>(((ku64*)__builtin_amdgcn_kernarg_segment_ptr())[w]);
}

// A row-offset table in device memory (TAB 2 launches): row i of stripe s at base + dtab[s * (K +
// M) + i] -- stripes whose shards each sit at their own address, any number per launch
struct BsTabArgs {
  const uint8_t* base;
  const uint32_t* dtab;
};

// Encode: Net's K inputs -> its first M rows (K <= 16: 8 K input planes in registers)
template <class Net, int M, int TAB>
__global__ __launch_bounds__(64 * kBsWaves) __attribute__((amdgpu_waves_per_eu(2, 2))) void gf_bs_kernel(
    const dev::GfArgs a, const BsTabArgs tb, uint32_t tiles_per_stripe, uint32_t ntiles) {
  using namespace dev;
  constexpr int K = Net::K, PF = K < kBsPrefetch ? K : kBsPrefetch;
  constexpr int NW = 2 * (K - PF) + 2 * M;  // vector memory ops a tile issues after its prefetch
  __shared__ __attribute__((aligned(16))) uint8_t lds[kBsWaves][PF * kBsWaveBytes];
  // the wave index as a scalar: tiles, stripes and row pointers are then wave-uniform (scalar loads
  // of the pointer table, no vector memory operations besides the shard copies counted below)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  uint8_t* pre = lds[wave];
  const uint32_t nw = gridDim.x * kBsWaves;
  // row i of stripe s (inputs 0..K-1, then outputs), at the lane's first byte of column tile c
  const auto row = [&](uint32_t s, int i, uint32_t c) -> uint8_t* {
    const uint8_t* base;
    if constexpr (TAB == 2) {
      typedef const __attribute__((address_space(4))) uint32_t cu32;
      uint32_t w = __builtin_amdgcn_readfirstlane(s * (uint32_t)(K + M) + (uint32_t)i);
      asm volatile("" : "+s"(w));
      base = tb.base + ((cu32*)tb.dtab)[w];  // a scalar load: the table is read-only for the launch
    } else if (i < K) {
      base = a.sstride ? a.ptr[i] + (int64_t)s * a.sstride : a.ptr[s * K + i];
    } else {
      base = a.sstride ? a.ptr[K + (i - K)] + (int64_t)s * a.sstride : a.ptr[a.tab * K + s * M + (i - K)];
    }
    return const_cast<uint8_t*>(base) + (size_t)c * kBsWaveBytes + lane * 16;
  };
  const auto prefetch = [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe, c = t % tiles_per_stripe;
#pragma unroll
    for (int i = 0; i < PF; ++i) bs_glds_row<kBsEncGlds>(row(s, i, c), pre + i * kBsWaveBytes);
  };
  uint32_t t = blockIdx.x * kBsWaves + wave;
  if (t >= ntiles) return;  // no barrier in this kernel: idle waves leave at once
  prefetch(t);
  __builtin_amdgcn_s_waitcnt(bs_waitcnt_vm(0));
  for (; t < ntiles; t += nw) {
    const uint32_t s = t / tiles_per_stripe, c = t % tiles_per_stripe;
    uint32_t x[8 * K];
#pragma unroll
    for (int i = PF; i < K; ++i) bs_ld_row(row(s, i, c), &x[8 * i]);
    // the prefetched rows were issued before the previous tile's stores and these loads, and
    // vector memory operations retire in issue order
    __builtin_amdgcn_s_waitcnt(bs_waitcnt_vm(NW > 63 ? 63 : NW));
#pragma unroll
    for (int i = 0; i < PF; ++i) bs_lds_row(pre + i * kBsWaveBytes, lane, &x[8 * i]);
    __builtin_amdgcn_s_waitcnt(kBsWaitLgkm0);
#pragma unroll
    for (int i = 0; i < K; ++i) bs_transpose8(&x[8 * i]);
    if constexpr (Net::Paired) bs_pair_basis<K>(x);
    __builtin_amdgcn_sched_barrier(0);
    prefetch(t + nw < ntiles ? t + nw : t);  // branch-free: nothing sinks below it (the last re-reads)
    __builtin_amdgcn_sched_barrier(0);
    Net::template net<M>(x, [&](int r, uint32_t (&o)[8]) {
      bs_transpose8(o);
      bs_st_row(row(s, K + r, c), o);
    });
  }
  // the last tile's re-prefetch is still in flight: the wave's LDS must not be handed to the next
  // workgroup on this CU (another launch's) while a DMA can still land in it (bs_drain_exit)
  bs_drain_exit();
}

// Reconstruct + Verify of the 16 + 20 code (C5's repair pass) in the same form, the syndrome way:
//   1. the 16 data slots as planes, a missing data row's slot loaded from a zero buffer;
//   2. s_q = stored(prow[q]) ^ (row prow[q] of the network over the present data): the stand-in
//      parities' syndromes, = A d with A the nd x nd block of the parity matrix at those rows and
//      the missing columns;
//   3. d = A^-1 s in byte form (v_perm products, tables from the host), stored, transposed and
//      written into their (zero) slots and the paired basis' pair sums -- no register indexing;
//   4. the full network: each parity (and extra) row stored (pstore), compared with its stored copy
//      through a 3-deep LDS ring filled by global_load_lds 2 compared rows ahead (pcmp; a mismatch
//      sets the stripe's flag), or skipped (the stand-ins, consistent by construction).
// Slots 0-6 of the next tile are prefetched into LDS during the network, slots 7-15 and the
// stand-ins load at the tile's top; 20 KiB of LDS per wave, 8 waves per CU.  C5's tasklet:
// 158.7-161.6 us against 173.0 us for the dyadic repair kernel (profiles/r04/bs_probe.txt).
struct BsRepairArgs {
  uint8_t slot[4];      // missing data row q (its slot), q < nd <= kBsRepairMaxNd
  uint8_t prow[4];      // the parity row standing in for it (input 16 - nd + q)
  dev::u32x4 t01[16];   // A^-1 product tables, entry j * 4 + q (gf_device.hpp coef_tables layout)
  uint32_t t2[16];
  const uint8_t* zero;  // kBsWaveBytes of zeros
  const uint8_t* base;  // TAB: row (s, i) at base + the 32-bit offset s * (16 + ND + M) + i of the table
  const uint32_t* dtab; // TAB 2: that table in device memory (TAB 1: in the argument block)
};

// TAB launches keep their row offsets where a repair launch does not read its GfArgs: from coef to
// the end of ptr (coef, slen, padding, ptr: the struct's last fields, in that order)
constexpr size_t kBsTabOff = offsetof(dev::GfArgs, coef);
static_assert(offsetof(dev::GfArgs, slen) > kBsTabOff && offsetof(dev::GfArgs, ptr) > offsetof(dev::GfArgs, slen) &&
                  offsetof(dev::GfArgs, ptr) + sizeof(dev::GfArgs::ptr) + 16 > sizeof(dev::GfArgs) && kBsTabOff % 4 == 0,
              "GfArgs: coef, slen, ptr last");
static_assert(sizeof(dev::GfArgs) + sizeof(BsRepairArgs) + 8 <= 4096, "repair kernel arguments within 4 KiB");
constexpr int kBsTabWords = (int)((offsetof(dev::GfArgs, ptr) + sizeof(dev::GfArgs::ptr) - kBsTabOff) / 4);

// word j of the kernel arguments' table area, by an opaque scalar load (as bs_kernarg_ptr)
__device__ __forceinline__ uint32_t bs_kernarg_u32(uint32_t j) {
  typedef const __attribute__((address_space(4))) uint32_t ku32;
  uint32_t w = __builtin_amdgcn_readfirstlane((uint32_t)(kBsTabOff / 4) + j);
  asm volatile("" : "+s"(w));
  return ((ku32*)__builtin_amdgcn_kernarg_segment_ptr())[w];
}

// 6 prefetched slots, or plain stores for the rebuilt rows, measured no faster (profiles/r04/bs_rep_variants.txt)
constexpr int kRepPrefetch = 7;  // slots prefetched into LDS per wave
constexpr int kRepRing = 3;      // LDS ring of compared rows per wave
static_assert(kRepRing >= 3 || kRepRing == 2, "ring of 2 or more rows");
#ifndef CFSEC_BS_DEBUG_FLAGS
// 1: a failed compare writes 0x80000000 | row << 24 | column tile (the stripe's first mismatching
// compared row of the lane that wrote last) instead of 1 into the stripe's flag word (diagnosis)
#define CFSEC_BS_DEBUG_FLAGS 0
#endif

__device__ __forceinline__ void bs_mul_acc8(uint32_t* acc, const uint32_t* s0, const uint32_t* s1, const uint32_t* s2,
                                            const dev::u32x4 q, uint32_t t2) {
#pragma unroll
  for (int w = 0; w < 8; ++w)
    acc[w] = dev::bs_x3(acc[w], __builtin_amdgcn_perm(q.y, q.x, s0[w]), __builtin_amdgcn_perm(q.w, q.z, s1[w])) ^
             __builtin_amdgcn_perm(0u, t2, s2[w]);
}

// (GfArgs must stay the first parameter: bs_kernarg_ptr / bs_kernarg_u32 read it at offset 0 of
// the arguments)
template <int M, int ND, int TAB>
__global__ __launch_bounds__(64 * kBsWaves) __attribute__((amdgpu_waves_per_eu(2, 2))) void gf_bs16_repair_kernel(
    const dev::GfArgs a, const BsRepairArgs r, uint32_t tiles_per_stripe, uint32_t ntiles) {
  using namespace dev;
  constexpr int PF = kRepPrefetch;
  constexpr int kWaveLds = (PF + kRepRing) * kBsWaveBytes;
  // one LDS array (a second __shared__ object can cost a vmcnt(0) before the first ds_read)
  __shared__ __attribute__((aligned(16))) uint8_t lds[kBsWaves * kWaveLds];
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  uint8_t* pre = lds + wave * kWaveLds;
  uint8_t* ring = pre + PF * kBsWaveBytes;
  const uint32_t nw = gridDim.x * kBsWaves;
  if (blockIdx.x == 0)  // the checksum words the pass after this one accumulates into
    for (uint32_t i = threadIdx.x; i < a.nzw; i += blockDim.x) a.zw[i] = 0u;
  // affine batches: row i of stripe s at ptr[i] + s * sstride; TAB: at base + its table offset
  const auto row_ptr = [&](uint32_t s, int i) -> const uint8_t* {
    if constexpr (TAB == 2) {
      typedef const __attribute__((address_space(4))) uint32_t cu32;
      uint32_t w = __builtin_amdgcn_readfirstlane(s * (uint32_t)(kBsK + ND + M) + (uint32_t)i);
      asm volatile("" : "+s"(w));
      return r.base + ((cu32*)r.dtab)[w];  // a scalar load: the table is read-only for the launch
    } else if constexpr (TAB == 1) {
      return r.base + bs_kernarg_u32(s * (uint32_t)(kBsK + ND + M) + (uint32_t)i);
    } else {
      return bs_kernarg_ptr(i) + (int64_t)s * a.sstride;
    }
  };
  const auto input = [&](uint32_t s, int i, uint32_t c) -> const uint8_t* {
    return row_ptr(s, i) + (size_t)c * kBsWaveBytes + lane * 16;
  };
  const auto output = [&](uint32_t s, int o, uint32_t c) -> uint8_t* {
    return const_cast<uint8_t*>(row_ptr(s, kBsK + o)) + (size_t)c * kBsWaveBytes + lane * 16;
  };
  const auto slot_ptr = [&](uint32_t s, int i, uint32_t c) -> const uint8_t* {  // data row i, or zeros
    const int src = a.src[i];
    return src < kBsK ? input(s, src, c) : r.zero + lane * 16;
  };
  const auto prefetch = [&](uint32_t t) {
    const uint32_t s = t / tiles_per_stripe, c = t % tiles_per_stripe;
#pragma unroll
    for (int i = 0; i < PF; ++i) bs_glds_row<kBsRepGlds>(slot_ptr(s, i, c), pre + i * kBsWaveBytes);
  };
  // tiles: every nw-th, from the wave's index (per-stripe order cost 2 %, blocks of consecutive
  // tiles 8 %: profiles/r06/c5_perbid_order.txt, profiles/r05/c5_repair_crc.txt)
  uint32_t t = blockIdx.x * kBsWaves + wave;
  if (t >= ntiles) return;
  prefetch(t);
  __builtin_amdgcn_s_waitcnt(bs_waitcnt_vm(0));
  for (; t < ntiles; t += nw) {
    const uint32_t s = t / tiles_per_stripe, c = t % tiles_per_stripe;
    uint32_t x[128];
    uint32_t y[ND > 0 ? ND : 1][8];
#pragma unroll
    for (int i = PF; i < kBsK; ++i) bs_ld_row(slot_ptr(s, i, c), &x[8 * i]);
#pragma unroll
    for (int q = 0; q < ND; ++q) bs_ld_row(input(s, kBsK - ND + q, c), y[q]);
    // the prefetched slots were issued before everything since (in-order retirement)
    __builtin_amdgcn_s_waitcnt(bs_waitcnt_vm(2 * (kBsK - PF + ND)));
#pragma unroll
    for (int i = 0; i < PF; ++i) bs_lds_row(pre + i * kBsWaveBytes, lane, &x[8 * i]);
    __builtin_amdgcn_s_waitcnt(kBsWaitLgkm0);
    __builtin_amdgcn_sched_barrier(0);
    // which slots are present, one bit each, re-read per tile (opaque) like the row masks
    uint32_t present = 0;
#pragma unroll
    for (int i = 0; i < kBsK; ++i) present |= (a.src[i] < kBsK ? 1u : 0u) << i;
    present = __builtin_amdgcn_readfirstlane(present);
    asm volatile("" : "+s"(present));
#pragma unroll
    for (int i = 0; i < kBsK; ++i)
      if (present >> i & 1) bs_transpose8(&x[8 * i]);  // a missing slot's zeros need none
    if constexpr (BsEc16p20l2::Paired) bs_pair_basis<kBsK>(x);
    if constexpr (ND > 0) {
      // 2. syndromes of the stand-ins over the present data (missing slots are zero planes), in
      // bytes: the row's planes transposed back and XOR-ed into the stored copy
#pragma unroll
      for (int q = 0; q < ND; ++q) {
        uint32_t o[8];
        bs_row_ec16p20l2_rt(r.prow[q], x, o);
        bs_transpose8(o);
#pragma unroll
        for (int w = 0; w < 8; ++w) y[q][w] ^= o[w];
      }
      // 3. d = A^-1 s, stored, into its slot (the slot bytes re-read per tile, as the row masks)
      uint32_t slots = (uint32_t)r.slot[0] | (uint32_t)r.slot[1] << 8 | (uint32_t)r.slot[2] << 16 | (uint32_t)r.slot[3] << 24;
      asm volatile("" : "+s"(slots));
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        const uint32_t slot_j = slots >> (8 * j) & 0xFFu;
        uint32_t d[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) d[w] = 0u;
#pragma unroll
        for (int q = 0; q < ND; ++q) {
          uint32_t s0[8], s1[8], s2[8];
#pragma unroll
          for (int w = 0; w < 8; ++w) {
            s0[w] = y[q][w] & 0x07070707u;
            s1[w] = (y[q][w] >> 3) & 0x07070707u;
            s2[w] = (y[q][w] >> 6) & 0x03030303u;
          }
          bs_mul_acc8(d, s0, s1, s2, r.t01[j * 4 + q], r.t2[j * 4 + q]);
        }
        bs_st_row(output(s, j, c), d);
        bs_transpose8(d);
#pragma unroll
        for (int i = 0; i < kBsK; ++i) {
          // the slot held zero planes; in the paired basis the even slot of its pair holds the
          // pair's sum, which takes d too (both slots of a pair missing: d_even ^ d_odd there)
          const int e = BsEc16p20l2::Paired ? (i & ~1) : i;  // folds after the unroll
          if (i == slot_j) {  // uniform: one slot's moves (not a masked XOR over every slot)
#pragma unroll
            for (int w = 0; w < 8; ++w) x[8 * e + w] ^= d[w];
            if (e != i)
#pragma unroll
              for (int w = 0; w < 8; ++w) x[8 * i + w] = d[w];
          }
        }
      }
    }
    // ring: the first two compared rows; then the next tile's slots
    uint32_t pend = a.pcmp, q_issue = 0, q_read = 0;
    const auto issue_ring = [&]() {
      if (pend) {
        const int p = __builtin_ctz(pend);
        pend &= pend - 1;
        bs_glds_row<kBsRepGlds>(output(s, ND + p, c), ring + (q_issue % kRepRing) * kBsWaveBytes);
        ++q_issue;
      }
    };
    issue_ring();
    issue_ring();
    __builtin_amdgcn_sched_barrier(0);
    prefetch(t + nw < ntiles ? t + nw : t);  // branch-free: the last tile re-reads itself
    __builtin_amdgcn_sched_barrier(0);
    uint32_t diff = 0, first_bad = 0;
    (void)first_bad;
    // the row masks re-read per tile (opaque): hoisted, their 44 per-row conditions outlive the
    // SGPRs as 64-bit lane masks and come back through v_readlane
    uint32_t pst = a.pstore, pcm = a.pcmp;
    asm volatile("" : "+s"(pst), "+s"(pcm));
    bs_net_ec16p20l2<M>(x, [&](int p, uint32_t (&o)[8]) {
      if (pst >> p & 1) {
        bs_transpose8(o);
        bs_st_row(output(s, ND + p, c), o);
      } else if (pcm >> p & 1) {
        // this row's copy; the next compared row's may still fly (anything issued between them is
        // waited for too: retirement is in order)
        if (q_issue - q_read > 1) __builtin_amdgcn_s_waitcnt(bs_waitcnt_vm(2));
        else __builtin_amdgcn_s_waitcnt(bs_waitcnt_vm(0));
        uint32_t v[8];
        bs_lds_row(ring + (q_read % kRepRing) * kBsWaveBytes, lane, v);
        __builtin_amdgcn_s_waitcnt(kBsWaitLgkm0);
        ++q_read;
        issue_ring();
        bs_transpose8(v);
        uint32_t dd = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) dd |= v[w] ^ o[w];
        if constexpr (CFSEC_BS_DEBUG_FLAGS)
          if (dd && !first_bad) first_bad = 0x80000000u | (uint32_t)p << 24 | (c & 0xFFFFFFu);
        diff |= dd;
      }
    });
    if (diff) {
      if constexpr (CFSEC_BS_DEBUG_FLAGS) __hip_atomic_store(a.flags + s, first_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      else set_flag(a.flags, s);
    }
  }
  bs_drain_exit();
}

int cu_count() {
  static int n[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!n[dev]) {
    int v = 0;
    n[dev] = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
  }
  return n[dev];
}

// One workgroup of kBsWaves persistent waves per CU, fewer when the tiles run out
unsigned bs_grid(uint32_t ntiles) {
  return (unsigned)std::min<uint64_t>((uint64_t)cu_count(), ((uint64_t)ntiles + kBsWaves - 1) / kBsWaves);
}

// Columns [0, len) of ns stripes as whole tiles: the tiles per stripe and of the launch; false for a
// length that is no positive multiple of the tile, or more tiles than the kernels' 32-bit index holds
bool bs_tiles(uint64_t len, unsigned ns, uint32_t* tps, uint32_t* ntiles) {
  const uint64_t per = len / dev::kBsWaveBytes, all = (uint64_t)(uint32_t)per * ns;
  if ((uint32_t)per == 0 || all > 0xFFFFFFFFull || (len % dev::kBsWaveBytes)) return false;
  *tps = (uint32_t)per;
  *ntiles = (uint32_t)all;
  return true;
}

// n row addresses as 32-bit offsets from the lowest (TAB launches): that address, or false when the
// rows span 4 GiB or more (bs_tab_span_ok); then the offsets
bool bs_rows_base(const uint8_t* const* rows, size_t n, uintptr_t* base) {
  uintptr_t lo = ~(uintptr_t)0, hi = 0;
  for (size_t i = 0; i < n; ++i) {
    lo = std::min(lo, (uintptr_t)rows[i]);
    hi = std::max(hi, (uintptr_t)rows[i]);
  }
  *base = lo;
  return bs_tab_span_ok(lo, hi);
}
void bs_row_offsets(const uint8_t* const* rows, size_t n, uintptr_t base, uint32_t* off) {
  for (size_t i = 0; i < n; ++i) off[i] = (uint32_t)((uintptr_t)rows[i] - base);
}

template <class Net>
bool rows_match(const uint8_t* coef, int m) {
  const uint8_t* w = Net::rows();
  for (int i = 0; i < m * Net::K; ++i)
    if (coef[i] != w[i]) return false;
  return true;
}

template <class Net, int M, int TAB = 0>
hipError_t launch_net(const dev::GfArgs& a, uint32_t tps, uint32_t nt, hipStream_t st,
                      BsTabArgs tb = {nullptr, nullptr}) {
  hipLaunchKernelGGL((gf_bs_kernel<Net, M, TAB>), dim3(bs_grid(nt)), dim3(64 * kBsWaves), 0, st, a, tb, tps, nt);
  return hipGetLastError();
}
}  // namespace

// EC15P12 / EC12P9 networks (tools/gen_bs_net.py ec15p12 | ec12p9) run 13-23 % slower than the
// lookup-product kernel on their shapes (profiles/r04/bsk_ab.txt: 2-3 tiles per wave, and the row
// tails need a second launch), so only the 16 + 20 code takes this route.
bool bs_matches(const uint8_t* coef, int m, int k) {
  if (k == 16 && (m == 20 || m == 22)) return rows_match<dev::BsEc16p20l2>(coef, m);
  return false;
}

hipError_t launch_bs(int k, int m, const dev::GfArgs& a, unsigned ns, uint64_t len, hipStream_t st) {
  uint32_t tps, nt;
  if (!bs_tiles(len, ns, &tps, &nt)) return hipErrorInvalidValue;
  if (k == 16 && m == 20) return launch_net<dev::BsEc16p20l2, 20>(a, tps, nt, st);
  if (k == 16 && m == 22) return launch_net<dev::BsEc16p20l2, 22>(a, tps, nt, st);
  return hipErrorInvalidValue;
}

namespace {
// kBsWaveBytes of zeros on the current device (the missing slots' loads), allocated once
const uint8_t* zero_tile() {
  static std::mutex mu;
  static const uint8_t* z[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (!z[dev]) {
    void* p = nullptr;
    if (hipMalloc(&p, dev::kBsWaveBytes) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, dev::kBsWaveBytes) != hipSuccess) {
      (void)hipFree(p);
      return nullptr;
    }
    z[dev] = static_cast<const uint8_t*>(p);
  }
  return z[dev];
}

void coef_tables_host(uint8_t c, dev::u32x4& t01, uint32_t& t2) {  // gf_device.hpp coef_tables
  const GF& gf = GF::get();
  uint32_t p[8];
  p[0] = c;
  for (int j = 1; j < 8; ++j) p[j] = gf.mul((uint8_t)p[j - 1], 2);
  uint32_t t0lo = 0, t0hi = 0, t1lo = 0, t1hi = 0, tt2 = 0;
  for (int e = 0; e < 8; ++e) {
    const uint32_t v0 = ((e & 1) ? p[0] : 0u) ^ ((e & 2) ? p[1] : 0u) ^ ((e & 4) ? p[2] : 0u);
    const uint32_t v1 = ((e & 1) ? p[3] : 0u) ^ ((e & 2) ? p[4] : 0u) ^ ((e & 4) ? p[5] : 0u);
    if (e < 4) {
      const uint32_t v2 = ((e & 1) ? p[6] : 0u) ^ ((e & 2) ? p[7] : 0u);
      t0lo |= v0 << (8 * e);
      t1lo |= v1 << (8 * e);
      tt2 |= v2 << (8 * e);
    } else {
      t0hi |= v0 << (8 * (e - 4));
      t1hi |= v1 << (8 * (e - 4));
    }
  }
  t01 = dev::u32x4{t0lo, t0hi, t1lo, t1hi};
  t2 = tt2;
}

template <int M, int TAB>
hipError_t launch_rep_m(int nd, const dev::GfArgs& a, const BsRepairArgs& r, uint32_t tps, uint32_t nt,
                        hipStream_t st) {
  const dim3 grid(bs_grid(nt)), block(64 * kBsWaves);
  switch (nd) {
    case 0: hipLaunchKernelGGL((gf_bs16_repair_kernel<M, 0, TAB>), grid, block, 0, st, a, r, tps, nt); break;
    case 1: hipLaunchKernelGGL((gf_bs16_repair_kernel<M, 1, TAB>), grid, block, 0, st, a, r, tps, nt); break;
    case 2: hipLaunchKernelGGL((gf_bs16_repair_kernel<M, 2, TAB>), grid, block, 0, st, a, r, tps, nt); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
template <int TAB>
hipError_t launch_rep(int nd, int ne, const dev::GfArgs& a, const BsRepairArgs& r, uint32_t tps, uint32_t nt,
                      hipStream_t st) {
  return ne == 2 ? launch_rep_m<22, TAB>(nd, a, r, tps, nt, st) : launch_rep_m<20, TAB>(nd, a, r, tps, nt, st);
}

bool rep_args(int nd, const uint8_t* missing, const uint8_t* prow, const uint8_t* ainv, BsRepairArgs& r) {
  for (int q = 0; q < nd; ++q) {
    r.slot[q] = missing[q];
    r.prow[q] = prow[q];
    for (int j = 0; j < nd; ++j) coef_tables_host(ainv[j * 4 + q], r.t01[j * 4 + q], r.t2[j * 4 + q]);
  }
  r.zero = zero_tile();
  return r.zero != nullptr;
}
}  // namespace

hipError_t launch_bs16_repair(int nd, int ne, const uint8_t* missing, const uint8_t* prow, const uint8_t* ainv,
                              const dev::GfArgs& a, unsigned ns, uint64_t len, hipStream_t st) {
  uint32_t tps, nt;
  if (nd < 0 || nd > kBsRepairMaxNd || (ne != 0 && ne != 2) || a.tab != 1 || !bs_tiles(len, ns, &tps, &nt) ||
      (a.pcmp && !a.flags))
    return hipErrorInvalidValue;
  BsRepairArgs r{};
  if (!rep_args(nd, missing, prow, ainv, r)) return hipErrorOutOfMemory;
  return launch_rep<0>(nd, ne, a, r, tps, nt, st);
}

static int bs_tab_stripes(int mo) { return kBsTabWords / (kBsK + mo); }

// The row-offset tables (TAB 2: any number of stripes in one launch): a ring of kBsDevTables per
// device, each slot a table in mapped, coherent host memory that the kernel reads directly (no copy
// launch: a blit copy into a device twin, read through another XCD's L2 by the next kernel's scalar
// loads, is the one cross-launch hand-off this path had, and round 4's and round 5's false Verify
// flags on the scattered layout came only from it; the direct read measured the same time per call,
// profiles/r05/scattered_c5_upload.txt "host"), free again once the launch that read it has
// completed (its event, polled).  A launch takes a free slot without
// waiting; only when every slot is still in flight -- the host kBsDevTables launches ahead of the
// GPU, e.g. back-to-back asynchronous tasklets -- does it wait for the oldest one, a bounded queue's
// backpressure (the argument-block fallback measured 0.147 -> 0.205 ms per scattered C5 call when
// taken instead).
constexpr int kBsDevTables = 8;
constexpr size_t kBsDevTableMin = 64 * 1024;  // words per slot: growth (a hipFree) stays rare
struct BsDevTable {
  uint32_t* host = nullptr;
  uint32_t* dev = nullptr;
  size_t cap = 0;
  hipEvent_t done = nullptr;
  bool pending = false;
  bool dead = false;  // a launch may still read it and no event says when it ends: never reused
  uint64_t seq = 0;   // when it was last taken
};
struct BsDevTables {
  std::mutex mu;
  BsDevTable slot[kBsDevTables];
  uint64_t next = 0;
};

BsDevTables* dev_tables() {
  static BsDevTables t[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return nullptr;
  return &t[d];
}

// A free slot with room for n words (under the ring's mutex) -- with every slot in flight, the oldest
// once its launch completes -- or nullptr (no memory, a failed event)
BsDevTable* dev_table_reserve(BsDevTables& r, size_t n) {
  BsDevTable* t = nullptr;
  BsDevTable* oldest = nullptr;
  for (BsDevTable& c : r.slot) {
    if (c.dead) continue;
    if (c.pending) {
      const hipError_t q = hipEventQuery(c.done);
      if (q == hipErrorNotReady) {
        if (!oldest || c.seq < oldest->seq) oldest = &c;
        continue;
      }
      if (q != hipSuccess) return nullptr;
      c.pending = false;
    }
    if (!t || (t->cap < n && c.cap >= n)) t = &c;  // prefer a slot that needs no growth
    if (t->cap >= n) break;
  }
  if (!t && oldest) {  // the host is kBsDevTables launches ahead: wait for the oldest
    if (hipEventSynchronize(oldest->done) != hipSuccess) return nullptr;
    oldest->pending = false;
    t = oldest;
  }
  if (!t) return nullptr;
  t->seq = ++r.next;
  if (!t->done && hipEventCreateWithFlags(&t->done, hipEventDisableTiming) != hipSuccess) return nullptr;
  if (n <= t->cap) return t;
  if (t->host) (void)hipHostFree(t->host);
  t->host = nullptr;
  t->dev = nullptr;
  t->cap = 0;
  const size_t cap = std::max<size_t>(n, kBsDevTableMin);
  if (hipHostMalloc(reinterpret_cast<void**>(&t->host), cap * 4, hipHostMallocMapped | hipHostMallocCoherent) !=
      hipSuccess)
    return nullptr;
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&t->dev), t->host, 0) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipHostFree(t->host);
    t->host = nullptr;
    return nullptr;
  }
  t->cap = cap;
  return t;
}

// After a launch that reads dt's table: the event that frees the slot.  If it cannot be recorded the
// launch may still be reading the row offsets, so the slot is not handed out again before the stream
// has drained (or ever, when even that fails) -- a later reservation would rewrite the mapped table
// under the kernel.
hipError_t dev_table_fence(BsDevTable* dt, hipStream_t st) {
  const hipError_t e = hipEventRecord(dt->done, st);
  if (e == hipSuccess) {
    dt->pending = true;
    return hipSuccess;
  }
  if (hipStreamSynchronize(st) != hipSuccess) dt->dead = true;
  return e;
}

hipError_t launch_bs16_repair_tab(int nd, int ne, const uint8_t* missing, const uint8_t* prow, const uint8_t* ainv,
                                  const dev::GfArgs& a, const uint8_t* const* rows, unsigned ns, uint64_t len,
                                  hipStream_t st, bool* ok) {
  const int mo = nd + 20 + ne, per = bs_tab_stripes(mo);
  uint32_t tps, nt;
  *ok = false;
  if (nd < 0 || nd > kBsRepairMaxNd || (ne != 0 && ne != 2) || !bs_tiles(len, 1, &tps, &nt) ||
      (a.pcmp && !a.flags) || !rows || ns == 0)
    return hipErrorInvalidValue;
  const size_t nrows = (size_t)ns * (kBsK + mo);
  uintptr_t lo;
  if (!bs_rows_base(rows, nrows, &lo)) return hipSuccess;  // not ok: the caller keeps its route
  *ok = true;
  BsRepairArgs r{};
  if (!rep_args(nd, missing, prow, ainv, r)) return hipErrorOutOfMemory;
  r.base = reinterpret_cast<const uint8_t*>(lo);
  static thread_local dev::GfArgs t;
  std::memcpy(&t, &a, sizeof(dev::GfArgs));
  t.sstride = 0;
  t.tab = 1;
  // more stripes than the argument block holds: one launch over a device table (when one can be had)
  if (BsDevTables* ring = ns > (unsigned)per ? dev_tables() : nullptr) {
    std::lock_guard<std::mutex> lk(ring->mu);
    if (BsDevTable* dt = dev_table_reserve(*ring, nrows)) {
      bs_row_offsets(rows, nrows, lo, dt->host);
      std::atomic_thread_fence(std::memory_order_release);  // the table before the launch that reads it
      r.dtab = dt->dev;
      t.nstripes = ns;
      if (!bs_tiles(len, ns, &tps, &nt)) return hipErrorInvalidValue;
      const hipError_t e = launch_rep<2>(nd, ne, t, r, tps, nt, st);
      return e != hipSuccess ? e : dev_table_fence(dt, st);
    }
  }
  for (unsigned s0 = 0; s0 < ns; s0 += (unsigned)per) {
    const unsigned n = std::min<unsigned>((unsigned)per, ns - s0);
    uint32_t off[kBsTabWords];
    bs_row_offsets(rows + (size_t)s0 * (kBsK + mo), (size_t)n * (kBsK + mo), lo, off);
    std::memcpy(reinterpret_cast<uint8_t*>(&t) + kBsTabOff, off, (size_t)n * (kBsK + mo) * 4);
    t.flags = a.flags ? a.flags + s0 : nullptr;
    t.nstripes = n;
    if (!bs_tiles(len, n, &tps, &nt)) return hipErrorInvalidValue;
    const hipError_t e = launch_rep<1>(nd, ne, t, r, tps, nt, st);
    if (e != hipSuccess) return e;
    t.zw = nullptr;  // the first launch zeroed them
    t.nzw = 0;
  }
  return hipSuccess;
}

hipError_t launch_bs_tab(int k, int m, const dev::GfArgs& a, const uint8_t* const* rows, unsigned ns, uint64_t len,
                         hipStream_t st, bool* ok) {
  *ok = false;
  uint32_t tps, nt;
  if (k != 16 || (m != 20 && m != 22) || !bs_tiles(len, ns, &tps, &nt) || !rows || ns == 0)
    return hipErrorInvalidValue;
  const size_t nrows = (size_t)ns * (k + m);
  uintptr_t lo;
  if (!bs_rows_base(rows, nrows, &lo)) return hipSuccess;  // not ok: the caller keeps its route
  BsDevTables* ring = dev_tables();
  if (!ring) return hipSuccess;
  std::lock_guard<std::mutex> lk(ring->mu);
  BsDevTable* dt = dev_table_reserve(*ring, nrows);
  if (!dt) return hipSuccess;  // not ok: every table in flight, the caller keeps its route
  bs_row_offsets(rows, nrows, lo, dt->host);
  std::atomic_thread_fence(std::memory_order_release);  // the table before the launch that reads it
  *ok = true;
  static thread_local dev::GfArgs t;
  std::memcpy(&t, &a, sizeof(dev::GfArgs));
  t.sstride = 0;
  t.tab = 1;
  t.nstripes = ns;
  const BsTabArgs tb{reinterpret_cast<const uint8_t*>(lo), dt->dev};
  const hipError_t e = m == 22 ? launch_net<dev::BsEc16p20l2, 22, 2>(t, tps, nt, st, tb)
                               : launch_net<dev::BsEc16p20l2, 20, 2>(t, tps, nt, st, tb);
  return e != hipSuccess ? e : dev_table_fence(dt, st);
}

}  // namespace cfsec
