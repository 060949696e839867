// crc32block_objects.hpp -- the object table of the mixed-size crc32block launch
// (crc32block_objects.hip), shared by the host packer (pack_blk_objects, blk_objects.cpp) and the kernel.
//
// One launch checks, decodes or encodes many framed objects, each with its own payload size, range and
// alignment: nothing about an object is in the kernel argument block, which holds the table's device
// address and the work-item count, so the object count is not bounded by it.  A work item is one block
// of one object (one workgroup pass).  The table, in this order:
//
//   BlkHead                      counts, the mode, P, what every full block shares, array offsets
//   BlkObject object[nobjects]   addresses, size, range, first block and block count of the launch, first
//                                work item, and the constants crc32block.hip's BlockArgs holds once per
//                                launch: the last block's payload length, its fin, the tile-end factors,
//                                whole_fin, xlast
//   uint32_t  map[nitems]        the object of every work item (its block is b0 + item - item0)
//
// The tile-end factor x^(8(plen + h - tiles * 4096)) takes a block's reduced Horner sum from the end of
// its last tile back to the end of its payload.  h is the misalignment the pieces are cut at:
//   check    16-byte boundaries of the source: h = (src + 4) mod 16, one value for every block of the
//            object (block_len is a multiple of 4096), so the factor is one word per payload length
//   encode   4096-byte boundaries of the destination: h = (dst + 4) mod 4096, again one per object
//   decode   4096-byte boundaries of the destination, whose payloads sit P = block_len - 4 apart: h of
//            launch block w is (D + w * P) mod 4096 and h mod 16 takes four values, w mod 4; the words are
//            x^(8(plen + (h mod 16) - tiles * 4096)) for those four, the kernel multiplies by
//            x^(8 * 16 * (h / 16)) from the shift table (as crc32block.hip's gc4k)
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/cfsec.h"

namespace cfsec {

constexpr int kBlkCheck = 0, kBlkDecode = 1, kBlkEncode = 2;
constexpr uint32_t kBlkMaxItems = 1u << 26;  // work items of one table (4 TiB of 64 KiB blocks)

struct BlkHead {
  uint32_t nobjects, nitems;
  uint32_t mode, P;              // kBlk*; payload bytes of a full block
  uint32_t objs_off, map_off;    // bytes from the table's base
  uint32_t bytes;                // the whole table
  uint32_t fin_full;             // shift(~0, P) ^ ~0: a full block's ChecksumIEEE from its raw CRC
  // set by the launcher, not the packer: the device CRC table block, and the launch's result words --
  // [nobjects] first mismatching launch block (preset ~0), then [nobjects] whole-object checksums (preset 0)
  uint64_t tabs, words;
  uint32_t xpow2[32];            // x^(8 P 2^i): moves a block's raw CRC over 2^i full blocks
};
struct BlkObject {
  uint64_t src;                  // check, decode: the framed object's byte 0; encode: the payload
  uint64_t dst;                  // decode: where payload byte 0 would go (the caller's dst - from);
                                 // encode: the framed object's byte 0; check: 0
  uint64_t size, lo, hi;         // payload bytes; the payload range copied (decode), [0, size) otherwise
  uint32_t b0, nb;               // first block of the launch, blocks in the launch
  uint32_t item0, nblk;          // the object's first work item; blocks in the object
  uint32_t last_len, fin_last;   // payload of the last block; shift(~0, last_len) ^ ~0
  uint32_t whole, whole_fin;     // 1: accumulate the whole-object checksum; shift(~0, size) ^ ~0
  uint32_t xlast, h;             // x^(8 last_len); check, encode: the alignment term
  uint32_t g[2][4][2];           // tile-end factors [full, last block][w mod 4][extra tile]; check and
                                 // encode use [.][0][0] alone
};
static_assert(sizeof(BlkHead) == 176 && sizeof(BlkObject) == 144, "table records keep 8-byte alignment");

// What one object asks of a launch, from its numbers alone (no address is dereferenced): the status the
// single call would return before it touches the device, the blocks [b0, b0 + nb) it touches, and the
// framed bytes [f0, f1) they occupy.  nb == 0 with CFSEC_OK: nothing to launch.
struct BlkSpan {
  int status = CFSEC_OK;
  int64_t b0 = 0, nb = 0, nblk = 0, f0 = 0, f1 = 0;
  int64_t in_bytes = 0, out_bytes = 0;  // read from src + (encode ? 0 : f0), written at dst
  bool whole = false;                   // the call returns this object's whole-payload checksum
};
BlkSpan blk_object_span(int mode, const cfsec_blk_object& o, int64_t block_len);

// The object table of one launch, packed from objects o[0 .. n) in order.  status[i] is decided for every
// object taken; the ones that need a launch (CFSEC_OK so far, nb > 0) go into the table, index[j] = the
// caller's index of table object j.  Objects are taken while the work items stay below kBlkMaxItems;
// `taken` says how many were.  dst == nullptr, or cap below the bytes needed: nothing is written (the
// sizing pass).  Host arithmetic only: no device call, no address is dereferenced.
struct BlkPack {
  size_t bytes = 0;  // the table's size
  uint32_t objects = 0, items = 0;
  size_t taken = 0;
  std::vector<int> status;
  std::vector<uint32_t> index;
};
BlkPack pack_blk_objects(int mode, const cfsec_blk_object* o, size_t n, int64_t block_len, uint8_t* dst, size_t cap);

}  // namespace cfsec
