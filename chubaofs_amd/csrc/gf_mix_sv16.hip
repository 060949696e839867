// gf_mix_sv16.hip -- the mixed-plan repair launch of the 16 + 20 code: Reconstruct + Verify of many
// items of EC16P20 / EC16P20L2's global stripe in one launch, and crc32.ChecksumIEEE of every row of
// every item out of the same pass, from one read of the item's 16 inputs.
//
// gf_mix_sv.hip would run such an item as 5-6 passes of 4 output rows, each pass reading the 16 inputs
// again: 16 products per output row.  The item's Dy16Plan (engine.hpp) describes the cheaper product
// repair_dy16 (gf_dyadic16.hpp) computes per launch group: the nd <= 4 missing data rows from their
// decode rows, then all 20 parity rows and the extra rows from the 16 data rows through the 16x16
// dyadic block (dev::dy16_rows).  Here that body is driven from an item table (gf_mix_sv16.hpp), with
// gf_mix_sv.hip's launch shape, ragged ends and checksums.  Per 4 KiB tile, once:
//
//   1. the 16 inputs are loaded in data-row slot order and checksummed from the loaded pieces, before
//      any accumulator is live;
//   2. the missing data rows come from the decode rows (coefficients in slot order; one instantiation
//      of the product per nd, the switch on a value every lane of the launch tile shares), are stored,
//      checksummed from the accumulator, and replace the stand-ins in their slots through
//      repair_dy16<SLOTS>'s uniform branch;
//   3. dy16_rows<1, 2> hands every parity and extra row to put(): a row whose pstore bit is set is
//      stored and checksummed from the product; one whose pcmp bit is set is loaded, compared, and
//      checksummed from WHAT WAS LOADED (the shard as it stands in memory: a corrupt survivor gives the
//      corrupt shard's word together with the raised Verify word); a row with neither bit is dropped.
//      One instantiation, E = 2: an EC16P20 item (e = 0) has zero tables and empty mask bits there;
//   4. one atomicXor per (tile, row) into the row's word, one dev::set_flag per wave that saw a
//      difference.
//
// The tables are built once per workgroup behind one barrier; nothing between the steps waits for
// another wave.  No access leaves [row, row + len) of any row: a lane loads, stores and compares only
// when `live`, at loff + 16 <= len (rows of at least 16 bytes) or bytes [0, len) (shorter rows, lane 0).
#include <hip/hip_runtime.h>

#include "gf_crc.hpp"
#include "gf_dyadic16.hpp"
#include "gf_mix_lane.hpp"
#include "gf_mix_sv16.hpp"
#include "kernels.hpp"

// Registers (compiler's resource-usage remarks, gfx950): 256 VGPRs, 0 AGPRs, no scratch, 2 waves per
// SIMD as built.  PIN = 0 (no scheduling barriers in dy16_rows) lets the scheduler run the checksums of
// many finished rows abreast: 256 VGPRs + 256 AGPRs and 536 bytes of scratch.  WPE = 3 (168 VGPRs): 340
// bytes of scratch.  Neither is taken.
#ifndef CFSEC_MIX16_PIN
#define CFSEC_MIX16_PIN 1  // dy16_rows' scheduling barriers
#endif
#ifndef CFSEC_MIX16_WPE
#define CFSEC_MIX16_WPE 2  // waves per SIMD the register allocation aims at
#endif

namespace cfsec {
namespace {

using namespace mixdev;

constexpr int kIn = kMixSv16In, kE = kMixSv16Extra;
constexpr int kRed16 = kIn + kMixSv16MaxOut;            // a wave's shares: inputs at [0, 16), outputs from 16
constexpr int kNDY = dev::kDy16Leaves + 36 + kIn * kE;  // build_dy16_tables<1, 2>'s slots
constexpr int kNT = kNDY + kIn * 4;                     // then decode row j, column c at kNDY + 4 c + j

// rec[0 .. ND) = the decode rows times the 16 input chunks
template <int ND>
__device__ __forceinline__ void decode_rows(uint32_t (&rec)[4][4], const uint32_t (&x)[kIn][4], const u32x4* tab01,
                                            const uint32_t* tab2) {
  auto& r = reinterpret_cast<uint32_t(&)[ND][4]>(rec);
#pragma unroll
  for (int c = 0; c < kIn; ++c) dev::mac_row_k<ND>(r, x[c], tab01 + kNDY + 4 * c, tab2 + kNDY + 4 * c);
}

__device__ __forceinline__ u32x4 vec(const uint32_t (&v)[4]) { return u32x4{v[0], v[1], v[2], v[3]}; }

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CFSEC_MIX16_WPE, 8))) void gf_mix_sv16_kernel(
    const uint8_t* __restrict__ table, uint32_t ntiles) {
  __shared__ u32x4 tab01[kNT];
  __shared__ uint32_t tab2[kNT];
  __shared__ uint32_t ct[crcdev::kFiveTabWords];
  __shared__ uint32_t red[4][kRed16];
  const uint32_t tile = blockIdx.x, tid = threadIdx.x;
  if (tile >= ntiles) return;
  const MixCrcHead* h = reinterpret_cast<const MixCrcHead*>(table);
  const uint32_t idx = reinterpret_cast<const uint32_t*>(table + h->map_off)[tile];
  const MixSv16Item* it = reinterpret_cast<const MixSv16Item*>(table + h->items_off) + idx;
  const int nd = (int)it->nd, e = (int)it->e;
  const uint64_t len = it->len;
  const uint64_t* in = reinterpret_cast<const uint64_t*>(table + h->rows_off) + it->rows;
  const uint64_t* out = in + kIn;
  const uint32_t* word = reinterpret_cast<const uint32_t*>(table + h->words_off) + it->rows;
  const uint8_t* coef = table + it->coef;
  const uint32_t q = tile - it->tile0;
  const uint64_t off = (uint64_t)q * kMixTile + (uint64_t)tid * dev::kLaneBytes;
  const uint32_t pstore = it->pstore, pcmp = it->pcmp;

  // the tables, once: the 16x16 block's leaves and the 4x4 row block (build_dy16_tables<1, 0>), the
  // extra rows (zero where the item has none), the decode rows (zero past nd)
  dev::build_dy16_tables<1, 0>(coef, tab01, tab2);
  for (int i = (int)tid; i < kIn * kE + kIn * 4; i += 256) {
    uint32_t cf = 0u;
    if (i < kIn * kE) {
      const int c = i / kE, x = i % kE;  // slot c * E + x, as build_dy16_tables<1, 2>
      if (x < e) cf = coef[(20 + x) * kIn + c];
    } else {
      const int j = (i - kIn * kE) & 3, c = (i - kIn * kE) >> 2;
      if (j < nd) cf = coef[(20 + e + j) * kIn + c];
    }
    dev::coef_tables(cf, tab01[dev::kDy16Leaves + 36 + i], tab2[dev::kDy16Leaves + 36 + i]);
  }
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
  for (uint32_t t = it->ntiles - 1 - q, p = 0; t && p < (uint32_t)kMixCrcPow; t >>= 1, ++p)
    if (t & 1u) g = crcdev::mulmod(g, h->xpow2[p]);
  const uint32_t fin = q == 0 ? it->fin : 0u;
  global_u32* const crc = (global_u32*)h->crc;
  __syncthreads();

  uint32_t diff = 0u;
  if (off - (uint64_t)lc.lane * dev::kLaneBytes >= len) {  // the whole wave lies past the row's end
    if (lc.lane < (uint32_t)kRed16) lc.red[lc.lane] = 0u;
  } else {
    const bool big = len >= (uint64_t)dev::kLaneBytes;  // the same in every lane
    const bool live = big ? off < len : off == 0;
    // the row's ragged end: the chunk at len - 16 instead, and its bytes from `over` on for the checksum
    const uint64_t loff = !big || off + dev::kLaneBytes <= len ? off : len - dev::kLaneBytes;
    const uint32_t over = live ? (uint32_t)(off - loff) : 0u;
    const auto piece = [&](u32x4 v) { return over ? dev::shr_bytes(v, over) : v; };
    const auto load = [&](uint64_t row) {  // a lane that is not live holds zeros
      u32x4 v{0u, 0u, 0u, 0u};
      if (big) {
        if (live) v = dev::ld16<true>(row_ptr(row) + loff);
      } else if (live) {
        v = dev::ld_tail(row_ptr(row), (size_t)len);
      }
      return v;
    };
    const auto store = [&](uint64_t row, u32x4 v) {
      if (big) {
        if (live) dev::st16_out<true>(row_ptr(row) + loff, v);
      } else if (live) {
        dev::st_tail(row_ptr(row), v, (size_t)len);
      }
    };
    // 1. the inputs, in slot order, and their checksums
    uint32_t x[kIn][4];
#pragma unroll
    for (int c = 0; c < kIn; ++c) {
      const u32x4 v = load(in[c]);
      x[c][0] = v.x, x[c][1] = v.y, x[c][2] = v.z, x[c][3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < kIn; ++c) lc.share(c, piece(vec(x[c])));
    // 2. the missing data rows
    if (nd > 0) {
      uint32_t rec[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int w = 0; w < 4; ++w) rec[j][w] = 0u;
      switch (nd) {
        case 1: decode_rows<1>(rec, x, tab01, tab2); break;
        case 2: decode_rows<2>(rec, x, tab01, tab2); break;
        case 3: decode_rows<3>(rec, x, tab01, tab2); break;
        default: decode_rows<4>(rec, x, tab01, tab2); break;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nd) {
          store(out[j], vec(rec[j]));
          lc.share(kIn + j, piece(vec(rec[j])));
        }
      // missing row j replaces the stand-in in its slot: a uniform branch (the asm keeps it one)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t m = j < nd ? (uint32_t)it->src[j] : 0xFFu;
#pragma unroll
        for (int i = 0; i < kIn; ++i) {
          if (m == (uint32_t)i) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int w = 0; w < 4; ++w) x[i][w] = rec[j][w];
          }
        }
      }
    }
    // 3. every parity and extra row from the 16 data chunks
    const uint64_t* pout = out + nd;
    const int pslot = kIn + nd;
    dev::dy16_rows<1, kE, (bool)CFSEC_MIX16_PIN, 4>(x, tab01, tab2, [&](int r, const uint32_t (&v)[4]) {
      if ((pstore >> r) & 1u) {
        store(pout[r], vec(v));
        lc.share(pslot + r, piece(vec(v)));
      } else if ((pcmp >> r) & 1u) {
        // a lane that is not live holds zeros in both; bytes past a short row's end are zero in both
        const u32x4 y = load(pout[r]);
        const u32x4 d = y ^ vec(v);
        diff |= d.x | d.y | d.z | d.w;
        lc.share(pslot + r, piece(y));  // the shard as it stands, not the product
      }
    });
  }
  __syncthreads();
  // 4. one atomic per (tile, row): thread t has row slot t = the row's place in row[] and word[]
  if (tid < (uint32_t)(kIn + nd + 20 + e)) {
    const uint32_t w = word[tid];
    if (w != kMixNoWord) {
      const uint32_t v = red[0][tid] ^ red[1][tid] ^ red[2][tid] ^ red[3][tid];
      atomicXor((uint32_t*)(crc + w), crcdev::mulmod(g, v) ^ fin);
    }
  }
  // Verify: one store per wave that saw a mismatch
  if (__any((int)(diff != 0u)) && lc.lane == 0u) dev::set_flag((uint32_t*)(global_u32*)it->flag, 0u);
}

}  // namespace

hipError_t launch_mix_sv16(const uint8_t* table, uint32_t ntiles, hipStream_t stream) {
  if (!table || ntiles == 0 || ntiles > kMixMaxTiles) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf_mix_sv16_kernel, dim3(ntiles), dim3(dev::kThreads), 0, stream, table, ntiles);
  return hipGetLastError();
}

}  // namespace cfsec
