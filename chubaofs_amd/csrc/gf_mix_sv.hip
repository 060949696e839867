// gf_mix_sv.hip -- the mixed-plan launch that stores, compares and checksums: Reconstruct + Verify of
// many items in one launch, and crc32.ChecksumIEEE of every row of every item out of the same pass.
//
// blobnode repairs a tasklet bid by bid: Reconstruct, then Verify, and a CRC32 of every shard around
// them (blobnode/work_shard_recover.go:708-771, 654-685, 335-342).  The bids are whatever blobs lived
// on the broken disk, mostly small and each of its own size, so the launch groups pay a product launch
// per erasure pattern and a checksum launch per length.  Here the whole tasklet is gf_mix_crc.hip's
// launch -- one workgroup per 4 KiB tile of one item, the item read from a table in device memory
// (gf_mix_sv.hpp), the checksums from the registers the product holds -- with Verify in it:
//
//   output rows [0, nstore)  are stored, and checksummed from the accumulator, as in gf_mix_crc.hip;
//   output rows [nstore, m)  are compared: the lane loads the shard's own 16 bytes at the offset it
//                            codes (the re-coded last chunk at len - 16 and ld_tail for rows under 16
//                            bytes included), compares them with the accumulator and checksums WHAT IT
//                            LOADED -- the contract is the checksum of the shard as it stands in
//                            memory, so a corrupt survivor gives the corrupt shard's CRC together
//                            with the raised Verify word.
//
// A mismatch in any lane raises the item's Verify word with dev::set_flag, a system-scope store of 1
// (gf_device.hpp says why no read-modify-write: the word may be pinned host memory), once per wave that
// saw one.  The word's address is a number in the table.
//
// Passes, ragged ends and bounds are gf_mix_crc.hip's: items with more than kMixPassRows outputs take
// further passes and re-read the inputs in each (checksummed in the first only); the split between
// stored and compared rows may fall inside a pass (mc, ns and r0 are the same in every lane of the
// workgroup); no access leaves [row, row + len) of any row.
#include <hip/hip_runtime.h>

#include "gf_crc.hpp"
#include "gf_mix_lane.hpp"
#include "gf_mix_sv.hpp"
#include "kernels.hpp"

namespace cfsec {
namespace {

using namespace mixdev;

// Rows [0, mc) of a pass (mc <= M; tables at stride kMixPassRows) over this lane's chunk: rows [0, ns)
// stored, rows [ns, mc) compared, and the wave's shares of the checksums of the inputs (CIN) and of
// those rows.  Every lane of the wave runs this (the shares are reduced over the wave): a lane past the
// row's end holds zeros.  Returns non-zero when a compared row differs in this lane's bytes.
template <int M, bool CIN, bool NTL>
__device__ __forceinline__ uint32_t mixsv_pass(int k, int mc, int ns, const uint64_t* in, const uint64_t* out,
                                               const u32x4* tab01, const uint32_t* tab2, const LaneCrc& lc,
                                               uint64_t off, uint64_t len) {
  constexpr int MT = kMixPassRows, G = 4;
  if (off - (uint64_t)lc.lane * dev::kLaneBytes >= len) {  // the whole wave lies past the row's end
    if (lc.lane == 0) {
      if constexpr (CIN)
        for (int c = 0; c < k; ++c) lc.red[c] = 0u;
      for (int r = 0; r < mc; ++r) lc.red[kInSlots + r] = 0u;
    }
    return 0u;
  }
  u32x4 acc[M];
#pragma unroll
  for (int r = 0; r < M; ++r) acc[r] = u32x4{0u, 0u, 0u, 0u};
  const bool big = len >= (uint64_t)dev::kLaneBytes;  // the same in every lane
  const bool live = big ? off < len : off == 0;
  // the row's ragged end: the chunk at len - 16 instead, and its bytes from `over` on for the checksum
  const uint64_t loff = !big || off + dev::kLaneBytes <= len ? off : len - dev::kLaneBytes;
  const uint32_t over = live ? (uint32_t)(off - loff) : 0u;
  const auto piece = [&](u32x4 v) { return over ? dev::shr_bytes(v, over) : v; };
  for (int c0 = 0; c0 < k; c0 += G) {
    u32x4 x[G];
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (c0 + g < k) {
        x[g] = u32x4{0u, 0u, 0u, 0u};
        if (big) {
          if (live) x[g] = dev::ld16<NTL>(row_ptr(in[c0 + g]) + loff);
        } else if (live) {
          x[g] = dev::ld_tail(row_ptr(in[c0 + g]), (size_t)len);
        }
      }
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (c0 + g < k) {
        dev::mac_row<M>(acc, x[g], tab01 + (c0 + g) * MT, tab2 + (c0 + g) * MT);
        if constexpr (CIN) lc.share(c0 + g, piece(x[g]));
      }
  }
  // the compared rows' own bytes, requested before the stored rows' stores and checksums
  u32x4 y[M];
#pragma unroll
  for (int r = 0; r < M; ++r) {
    y[r] = u32x4{0u, 0u, 0u, 0u};
    if (r >= ns && r < mc) {
      if (big) {
        if (live) y[r] = dev::ld16<true>(row_ptr(out[r]) + loff);
      } else if (live) {
        y[r] = dev::ld_tail(row_ptr(out[r]), (size_t)len);
      }
    }
  }
  uint32_t diff = 0u;
#pragma unroll
  for (int r = 0; r < M; ++r)
    if (r < ns) {
      if (big) {
        if (live) dev::st16_out<true>(row_ptr(out[r]) + loff, acc[r]);
      } else if (live) {
        dev::st_tail(row_ptr(out[r]), acc[r], (size_t)len);
      }
      lc.share(kInSlots + r, piece(acc[r]));
    } else if (r < mc) {
      // a lane that is not live holds zeros in both; bytes past a short row's end are zero in both
      const u32x4 d = y[r] ^ acc[r];
      diff |= d.x | d.y | d.z | d.w;
      lc.share(kInSlots + r, piece(y[r]));  // the shard as it stands, not the product
    }
  return diff;
}

__global__ __launch_bounds__(256) void gf_mix_sv_kernel(const uint8_t* __restrict__ table, uint32_t ntiles) {
  __shared__ u32x4 tab01[dev::kMaxK * kMixPassRows];
  __shared__ uint32_t tab2[dev::kMaxK * kMixPassRows];
  __shared__ uint32_t ct[crcdev::kFiveTabWords];
  __shared__ uint32_t red[4][kRedRows];
  const uint32_t tile = blockIdx.x, tid = threadIdx.x;
  if (tile >= ntiles) return;
  const MixCrcHead* h = reinterpret_cast<const MixCrcHead*>(table);
  const uint32_t idx = reinterpret_cast<const uint32_t*>(table + h->map_off)[tile];
  const MixSvItem* it = reinterpret_cast<const MixSvItem*>(table + h->items_off) + idx;
  const int k = (int)it->k, m = (int)it->m, nstore = (int)it->nstore;
  const uint64_t len = it->len;
  const uint64_t* in = reinterpret_cast<const uint64_t*>(table + h->rows_off) + it->rows;
  const uint64_t* out = in + k;
  const uint32_t* word = reinterpret_cast<const uint32_t*>(table + h->words_off) + it->rows;
  const uint8_t* coef = table + it->coef;
  const uint32_t q = tile - it->tile0;
  const uint64_t off = (uint64_t)q * kMixTile + (uint64_t)tid * dev::kLaneBytes;

  const global_u32* tabs = (const global_u32*)h->tabs;
  for (int i = (int)tid; i < crcdev::kFiveTabWords; i += 256) ct[i] = tabs[crcdev::kFiveTabBase + i];
  LaneCrc lc;
  lc.ct = ct;
  lc.red = red[tid >> 6];
  lc.lane = tid & 63u;
  lc.col[0] = tabs[crcdev::kShiftBase + tid];
#pragma unroll
  for (int i = 1; i < 32; ++i) lc.col[i] = (lc.col[i - 1] >> 1) ^ ((lc.col[i - 1] & 1u) ? crcdev::kPoly : 0u);
  // from this tile's end to the row's end, and the conditioning word, the row's first tile's to add:
  // the same in every lane
  uint32_t g = it->gend;
  for (uint32_t e = it->ntiles - 1 - q, p = 0; e && p < (uint32_t)kMixCrcPow; e >>= 1, ++p)
    if (e & 1u) g = crcdev::mulmod(g, h->xpow2[p]);
  const uint32_t fin = q == 0 ? it->fin : 0u;
  global_u32* const crc = (global_u32*)h->crc;

  uint32_t diff = 0u;
  int r0 = 0;
  do {
    const int mc = m - r0 < kMixPassRows ? m - r0 : kMixPassRows;
    const int ns = nstore <= r0 ? 0 : nstore - r0 < mc ? nstore - r0 : mc;  // stored rows of this pass
    if (r0) __syncthreads();  // the previous pass has read its tables and its shares
    dev::build_tables<kMixPassRows>(k, mc, coef + r0 * k, tab01, tab2);
    __syncthreads();
    if (m <= kMixPassRows) {  // one pass: every input byte is read once
      if (m <= 1) diff |= mixsv_pass<1, true, true>(k, mc, ns, in, out, tab01, tab2, lc, off, len);
      else if (m == 2) diff |= mixsv_pass<2, true, true>(k, mc, ns, in, out, tab01, tab2, lc, off, len);
      else diff |= mixsv_pass<kMixPassRows, true, true>(k, mc, ns, in, out, tab01, tab2, lc, off, len);
    } else if (r0 == 0) {
      diff |= mixsv_pass<kMixPassRows, true, false>(k, mc, ns, in, out, tab01, tab2, lc, off, len);
    } else {
      diff |= mixsv_pass<kMixPassRows, false, false>(k, mc, ns, in, out + r0, tab01, tab2, lc, off, len);
    }
    __syncthreads();
    // one atomic per (tile, row): thread t has the pass's row slot t
    const int slot = (int)tid;
    const bool valid = slot < kInSlots ? (r0 == 0 && slot < k) : slot - kInSlots < mc;
    if (slot < kRedRows && valid) {
      const int p = slot < kInSlots ? slot : k + r0 + slot - kInSlots;  // the row's place in row[] and word[]
      const uint32_t v = red[0][slot] ^ red[1][slot] ^ red[2][slot] ^ red[3][slot];
      atomicXor((uint32_t*)(crc + word[p]), crcdev::mulmod(g, v) ^ fin);
    }
    r0 += kMixPassRows;
  } while (r0 < m);
  // Verify: one store per wave that saw a mismatch
  if (__any((int)(diff != 0u)) && lc.lane == 0u) dev::set_flag((uint32_t*)(global_u32*)it->flag, 0u);
}

}  // namespace

hipError_t launch_mix_sv(const uint8_t* table, uint32_t ntiles, hipStream_t stream) {
  if (!table || ntiles == 0 || ntiles > kMixMaxTiles) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf_mix_sv_kernel, dim3(ntiles), dim3(dev::kThreads), 0, stream, table, ntiles);
  return hipGetLastError();
}

}  // namespace cfsec
