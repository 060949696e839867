// gf_mix_crc.hpp -- the item table of the mixed-plan launch with checksums (gf_mix_crc.hip), shared by
// the host packer (pack_mix_crc, batch.cpp) and the kernel.
//
// The launch is gf_mix.hip's -- store-only products of many items, one workgroup per 4 KiB tile of one
// item, everything about an item read from this table -- and on top of the product every row of an
// item, its k inputs and its m outputs, gets its crc32.ChecksumIEEE: access checksums every shard of a
// blob right after Encode (access/stream_put.go:249-253).  The table, in this order:
//
//   MixCrcHead                    counts, the byte offsets of the arrays below, the device addresses of
//                                 the CRC table block and of the call's checksum words, x^(8 * 4096 * 2^q)
//   MixCrcItem item[nitems]       as MixItem, plus the two length-dependent words of the item
//   uint64_t   row[]              per item k input row addresses, then m output row addresses
//   uint32_t   word[]             the checksum word of every row, parallel to row[]
//   uint32_t   tile_item[ntiles]  the item of every launch tile
//   uint8_t    coef[]             per plan m x k coefficient rows, row-major, each plan 16-byte aligned
//
// A row's word is the XOR of one share per tile -- the tile's raw (zero-preset) CRC moved to the row's
// end -- and of MixCrcItem::fin, XOR-ed in by the row's first tile: the order of the tiles does not
// matter, and the words start at zero (the batch call zeroes them).
#pragma once
#include <cstdint>

#include "gf_mix.hpp"

namespace cfsec {

constexpr int kMixCrcPow = 24;  // kMixMaxTiles = 2^24 tiles at most between a tile and its row's end

struct MixCrcHead {
  uint32_t nitems, ntiles;
  uint32_t items_off, rows_off, words_off, map_off, coef_off;  // bytes from the table's base
  uint32_t bytes;                                              // the whole table
  uint32_t nplans, pad[3];
  uint64_t tabs;              // device address of the CRC table block (crc_device_tables)
  uint64_t crc;                // device address of checksum word 0
  uint32_t xpow2[kMixCrcPow];  // x^(8 * 4096 * 2^q) mod P
};
struct MixCrcItem {
  uint64_t len;    // bytes per row
  uint32_t k, m;   // input rows (<= kLaunchMaxRows), output rows (0: checksums only)
  uint32_t coef;   // byte offset of the m x k coefficient rows from the table's base
  uint32_t rows;   // index of the item's first row address in row[], of its first word in word[]
  uint32_t tile0;  // the item's first launch tile
  uint32_t ntiles;
  uint32_t fin;    // shift(~0, len) ^ ~0: turns the raw CRC of len bytes into crc32.ChecksumIEEE
  uint32_t gend;   // x^(8 (len - 4096 ntiles)): from the end of the item's last tile back to the row's end
  uint32_t pad[2];
};
static_assert(sizeof(MixCrcHead) == 160 && sizeof(MixCrcItem) == 48, "table records");

}  // namespace cfsec
