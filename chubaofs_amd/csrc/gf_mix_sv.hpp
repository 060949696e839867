// gf_mix_sv.hpp -- the item table of the mixed-plan launch that stores, compares and checksums
// (gf_mix_sv.hip), shared by the host packer (pack_mix_sv, batch.cpp) and the kernel.
//
// The launch is gf_mix_crc.hip's with Verify in it: blobnode's repair tasklet runs Reconstruct, then
// Verify, per bid, and checksums every shard around them (blobnode/work_shard_recover.go:708-771,
// 654-685, 335-342).  Of an item's m output rows the first nstore are stored, the rest compared with
// the shards' own bytes; a mismatch raises the item's Verify word.  Every row -- k inputs, stored and
// compared outputs -- gets its crc32.ChecksumIEEE as it stands in memory.  The table is
// gf_mix_crc.hpp's, in the same order, with MixSvItem records:
//
//   MixCrcHead                    as gf_mix_crc.hpp
//   MixSvItem  item[nitems]       as MixCrcItem, plus nstore and the address of the item's Verify word
//   uint64_t   row[]              per item k input row addresses, then m output row addresses
//   uint32_t   word[]             the checksum word of every row, parallel to row[]
//   uint32_t   tile_item[ntiles]  the item of every launch tile
//   uint8_t    coef[]             per plan m x k coefficient rows, row-major, each plan 16-byte aligned
#pragma once
#include <cstdint>

#include "gf_mix_crc.hpp"

namespace cfsec {

struct MixSvItem {
  uint64_t len;     // bytes per row
  uint32_t k, m;    // input rows (<= kLaunchMaxRows), output rows (>= 1)
  uint32_t coef;    // byte offset of the m x k coefficient rows from the table's base
  uint32_t rows;    // index of the item's first row address in row[], of its first word in word[]
  uint32_t tile0;   // the item's first launch tile
  uint32_t ntiles;
  uint32_t fin;     // as MixCrcItem
  uint32_t gend;    // as MixCrcItem
  uint32_t nstore;  // output rows [0, nstore) are stored, [nstore, m) compared
  uint32_t pad;
  uint64_t flag;    // address of the item's Verify word (a 1 is stored there on a mismatch); unused
                    // when nothing is compared
};
static_assert(sizeof(MixSvItem) == 56, "table records");

}  // namespace cfsec
