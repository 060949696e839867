// gf_mix_crc.hip -- the mixed-plan launch with checksums: store-only GF(2^8) products of many items in
// one launch, and crc32.ChecksumIEEE of every row of every item out of the same pass.
//
// access ends every put with Encode and the CRC32 of every shard (access/stream_put.go:125-143,
// 249-253).  A blob smaller than the blob size is one stripe of its own shard size, so a batch gathered
// across requests is mostly small stripes, each of its own length: the fused product + checksum kernels
// (gf_crc.hpp) take one length per launch, and the separate pass takes a launch per length.  Here the
// whole batch is gf_mix.hip's launch -- one workgroup per 4 KiB tile of one item, the item read from a
// table in device memory (gf_mix_crc.hpp) -- and each workgroup also checksums its tile of every row
// from the registers the product holds: the k inputs as they are loaded, the outputs as they are stored.
//
// The checksum is crc32block_objects.hip's per-tile form on gf_crc.hpp's pieces: per lane the raw CRC of
// its 16 bytes (the 5-bit conflict-free tables in LDS, crc_step5's data words), moved from the piece's
// end to the tile's end (x^(8 * 16 * (255 - lane)), the per-lane shift constant of the table block, as
// 32 columns kept in registers: one row's move is 32 selects), XOR-reduced over the wave, the four
// waves' words XOR-ed and moved from the tile's end to the row's end (MixCrcItem::gend times a power of
// x^(8 * 4096)), and one atomicXor per (tile, row) into the row's word, which the batch call zeroed.
// The row's first tile adds MixCrcItem::fin.  XOR commutes: the tiles' order does not matter.
//
// Ragged ends.  The product codes a row's last partial chunk as gf_mix.hip does, by coding the row's
// last full 16 bytes at len - 16 again; a checksum must see every byte once and at its own place, so
// the lane holding the row's end checksums what it loaded (or computed) shifted down by the overlap,
// zeros in above: bytes [off, len) at the piece's start.  The zeros between the row's end and the tile's
// end are what gend (a negative power of x) takes out.  Rows shorter than 16 bytes are lane 0's
// ld_tail / st_tail, zero-padded the same way.  No access leaves [row, row + len); outputs are written
// with the compiler's own stores (st16_out, st_tail).
//
// Items with more than kMixPassRows outputs take further passes, as in gf_mix.hip; the inputs are
// checksummed in the first pass only, each output in the pass that produces it.  An item with no output
// rows (an engine with no parity shards) is one pass that checksums its inputs.
#include <hip/hip_runtime.h>

#include "gf_crc.hpp"
#include "gf_mix_crc.hpp"
#include "gf_mix_lane.hpp"
#include "kernels.hpp"

namespace cfsec {
namespace {

using namespace mixdev;  // row_ptr, crc_piece, LaneCrc: shared with gf_mix_sv.hip

// Rows [0, mc) of a pass (mc <= M; tables at stride kMixPassRows) over this lane's chunk, and the
// wave's shares of the checksums of the inputs (CIN) and of those rows.  Every lane of the wave runs
// this (the shares are reduced over the wave): a lane past the row's end holds zeros.
template <int M, bool CIN, bool NTL>
__device__ __forceinline__ void mixcrc_pass(int k, int mc, const uint64_t* in, const uint64_t* out, const u32x4* tab01,
                                            const uint32_t* tab2, const LaneCrc& lc, uint64_t off, uint64_t len) {
  constexpr int MT = kMixPassRows, G = 4;
  if (off - (uint64_t)lc.lane * dev::kLaneBytes >= len) {  // the whole wave lies past the row's end
    if (lc.lane == 0) {
      if constexpr (CIN)
        for (int c = 0; c < k; ++c) lc.red[c] = 0u;
      for (int r = 0; r < mc; ++r) lc.red[kInSlots + r] = 0u;
    }
    return;
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
#pragma unroll
  for (int r = 0; r < M; ++r)
    if (r < mc) {
      if (big) {
        if (live) dev::st16_out<true>(row_ptr(out[r]) + loff, acc[r]);
      } else if (live) {
        dev::st_tail(row_ptr(out[r]), acc[r], (size_t)len);
      }
      lc.share(kInSlots + r, piece(acc[r]));
    }
}

__global__ __launch_bounds__(256) void gf_mix_crc_kernel(const uint8_t* __restrict__ table, uint32_t ntiles) {
  __shared__ u32x4 tab01[dev::kMaxK * kMixPassRows];
  __shared__ uint32_t tab2[dev::kMaxK * kMixPassRows];
  __shared__ uint32_t ct[crcdev::kFiveTabWords];
  __shared__ uint32_t red[4][kRedRows];
  const uint32_t tile = blockIdx.x, tid = threadIdx.x;
  if (tile >= ntiles) return;
  const MixCrcHead* h = reinterpret_cast<const MixCrcHead*>(table);
  const uint32_t idx = reinterpret_cast<const uint32_t*>(table + h->map_off)[tile];
  const MixCrcItem* it = reinterpret_cast<const MixCrcItem*>(table + h->items_off) + idx;
  const int k = (int)it->k, m = (int)it->m;
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

  int r0 = 0;
  do {
    const int mc = m - r0 < kMixPassRows ? m - r0 : kMixPassRows;
    if (r0) __syncthreads();  // the previous pass has read its tables and its shares
    dev::build_tables<kMixPassRows>(k, mc, coef + r0 * k, tab01, tab2);
    __syncthreads();
    if (m <= kMixPassRows) {  // one pass: every input byte is read once
      if (m <= 1) mixcrc_pass<1, true, true>(k, mc, in, out, tab01, tab2, lc, off, len);
      else if (m == 2) mixcrc_pass<2, true, true>(k, mc, in, out, tab01, tab2, lc, off, len);
      else mixcrc_pass<kMixPassRows, true, true>(k, mc, in, out, tab01, tab2, lc, off, len);
    } else if (r0 == 0) {
      mixcrc_pass<kMixPassRows, true, false>(k, mc, in, out, tab01, tab2, lc, off, len);
    } else {
      mixcrc_pass<kMixPassRows, false, false>(k, mc, in, out + r0, tab01, tab2, lc, off, len);
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
}

}  // namespace

hipError_t launch_mix_crc(const uint8_t* table, uint32_t ntiles, hipStream_t stream) {
  if (!table || ntiles == 0 || ntiles > kMixMaxTiles) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf_mix_crc_kernel, dim3(ntiles), dim3(dev::kThreads), 0, stream, table, ntiles);
  return hipGetLastError();
}

}  // namespace cfsec
