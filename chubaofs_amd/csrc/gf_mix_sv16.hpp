// gf_mix_sv16.hpp -- the item table of the mixed-plan repair launch of the 16 + 20 code (gf_mix_sv16.hip),
// shared by the host packer (pack_mix_sv16, batch.cpp) and the kernel.
//
// The launch is gf_mix_sv.hip's -- Reconstruct + Verify of many items and every row's
// crc32.ChecksumIEEE out of one pass -- for items whose plan carries a Dy16Plan (engine.hpp): the
// nd <= 4 missing data rows from their decode rows, then all 20 parity rows and the e extra rows
// (EC16P20L2's two local parities) from the 16 data rows through the 16x16 dyadic block
// (gf_dyadic16.hpp), each parity row stored, compared or dropped by the plan's masks.  The table, in
// this order:
//
//   MixCrcHead                    as gf_mix_crc.hpp
//   MixSv16Item item[nitems]      below
//   uint64_t    row[]             per item the 16 input row addresses in data-row slot order (slot i =
//                                 data row i when present, else the parity standing in for a missing
//                                 row), then the nd + 20 + e addresses of Dy16Plan::rows (0 for a parity
//                                 row that is neither stored nor compared: it is never touched)
//   uint32_t    word[]            the checksum word of every row, parallel to row[]; kMixNoWord for an
//                                 output row that is neither stored nor compared (a stand-in already
//                                 checksummed as an input, or a row past e)
//   uint32_t    tile_item[ntiles] the item of every launch tile
//   uint8_t     coef[]            per plan (20 + e + nd) x 16 coefficient rows, each plan 16-byte
//                                 aligned: Dy16Plan::coef with the decode rows' columns in slot order
#pragma once
#include <cstdint>

#include "gf_mix_crc.hpp"

namespace cfsec {

constexpr uint32_t kMixNoWord = 0xFFFFFFFFu;
constexpr int kMixSv16In = 16;                 // input rows of an item
constexpr int kMixSv16MaxOut = 4 + 20 + 2;     // output rows at most: nd + 20 + e
constexpr int kMixSv16Extra = 2;               // extra rows the kernel computes (dropped where e == 0)

struct MixSv16Item {
  uint64_t len;    // bytes per row
  uint64_t flag;   // address of the item's Verify word (a 1 is stored there on a mismatch)
  uint32_t coef;   // byte offset of the plan's coefficient rows from the table's base
  uint32_t rows;   // index of the item's first row address in row[], of its first word in word[]
  uint32_t tile0;  // the item's first launch tile
  uint32_t ntiles;
  uint32_t fin;    // as MixCrcItem
  uint32_t gend;   // as MixCrcItem
  uint32_t pstore, pcmp;  // parity rows (bits 0..19) and extra rows (20..) stored / compared
  uint8_t nd, e;   // missing data rows (<= 4), extra rows (0 or 2)
  uint8_t pad[2];
  uint8_t src[4];  // src[j], j < nd: the data row (= input slot) of missing row j
};
static_assert(sizeof(MixSv16Item) == 56, "table records");

}  // namespace cfsec
