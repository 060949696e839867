// gf_mix.hpp -- the item table of the mixed-plan launch (gf_mix.hip), shared by the host packer
// (pack_mix, batch.cpp) and the kernel.
//
// A mixed launch codes store-only products of many items -- each with its own rows, length, input and
// output count and coefficient rows -- in one launch: nothing about an item is in the kernel argument
// block, which holds the table's device address and the tile count.  The table, in this order:
//
//   MixHead                       counts and the byte offsets of the four arrays below
//   MixItem  item[nitems]         length, k, m, where its row addresses and coefficient rows are,
//                                 its first launch tile
//   uint64_t row[]                per item k input row addresses, then m output row addresses
//   uint32_t tile_item[ntiles]    the item of every launch tile (its index within the item is
//                                 tile - item.tile0)
//   uint8_t  coef[]               per plan m x k coefficient rows, row-major, each plan 16-byte aligned;
//                                 items that share a plan share one copy
//
// A tile is kMixTile bytes of every row of one item (256 lanes x 16 bytes), one workgroup.
#pragma once
#include <cstdint>

namespace cfsec {

constexpr uint32_t kMixTile = 4096;
constexpr int kMixPassRows = 4;  // output rows per pass over a tile

struct MixHead {
  uint32_t nitems, ntiles;
  uint32_t items_off, rows_off, map_off, coef_off;  // bytes from the table's base
  uint32_t bytes;                                   // the whole table
  uint32_t nplans;
};
struct MixItem {
  uint64_t len;    // bytes per row
  uint32_t k, m;   // input rows (<= kLaunchMaxRows), output rows
  uint32_t coef;   // byte offset of the m x k coefficient rows from the table's base
  uint32_t rows;   // index of the item's first row address in row[]
  uint32_t tile0;  // the item's first launch tile
  uint32_t ntiles;
};
static_assert(sizeof(MixHead) == 32 && sizeof(MixItem) == 32, "table records are 32 bytes");

}  // namespace cfsec
