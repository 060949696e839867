// blk_objects.cpp -- the host plan of the mixed-size crc32block launch (crc32block_objects.hpp): each
// object's status and launch range, and the object table.  Host arithmetic only: no HIP call, no
// address is dereferenced (tests/test_blk_objects_plan.py drives it on a machine without a device).
#include <algorithm>
#include <cstring>

#include "crc32block_objects.hpp"
#include "crc_pow.hpp"

namespace cfsec {

namespace {

constexpr uint32_t kBlkMaxObjects = 1u << 22;  // with kBlkMaxItems: a table stays below 2^32 bytes
constexpr int64_t kTileBytes = 4096;

uint32_t xpow8(int64_t n) { return crc_xpow8(n); }  // x^(8 n), 0 <= n < 2^40 (crc_pow.hpp)
uint32_t shift_ones(uint32_t xlen) { return crc_shift_ones_of(xlen); }
// x^(8(len + h - tiles * 4096)) with tiles = ceil((len + h) / 4096) + extra
uint32_t tile_end_factor(int64_t len, int64_t h, int extra) {
  const int64_t tiles = (len + h + kTileBytes - 1) / kTileBytes + extra;
  return crc_pow_tables().neg[tiles * kTileBytes - len - h];
}

}  // namespace

BlkSpan blk_object_span(int mode, const cfsec_blk_object& o, int64_t block_len) {
  BlkSpan s;
  const int64_t P = block_len - 4;
  const bool encode = mode == kBlkEncode;
  if (o.size < 0 || o.size >= (int64_t(1) << 40) || (!encode && (o.from < 0 || o.from > o.to || o.to > o.size))) {
    s.status = CFSEC_ERR_INVALID_ARG;
    return s;
  }
  s.nblk = (o.size + P - 1) / P;
  s.nb = s.nblk;
  if (!encode) {
    // Decoder.Reader: from the block holding `from` through the block holding to - 1; from == to reads
    // (and checks) the block it has to skip into, none on a block boundary (capi.cpp blocks_touched)
    s.b0 = o.from / P;
    const int64_t b1 = o.from < o.to ? (o.to - 1) / P : (o.from % P ? s.b0 : s.b0 - 1);
    s.nb = b1 - s.b0 + 1;
  }
  if (s.nb <= 0) {
    s.b0 = s.nb = 0;
    return s;
  }
  s.f0 = s.b0 * block_len;
  s.f1 = std::min(o.size + 4 * s.nblk, (s.b0 + s.nb) * block_len);
  s.in_bytes = encode ? o.size : s.f1 - s.f0;
  s.out_bytes = encode ? s.f1 : mode == kBlkDecode ? o.to - o.from : 0;
  s.whole = encode || (o.from == 0 && o.to == o.size);
  if (!o.src || (s.out_bytes > 0 && !o.dst) || s.nblk > (int64_t)kBlkMaxItems)
    s.status = CFSEC_ERR_INVALID_ARG;
  else if (!encode && o.src_len < s.f1)
    s.status = CFSEC_ERR_SHORT_DATA;
  return s;
}

BlkPack pack_blk_objects(int mode, const cfsec_blk_object* o, size_t n, int64_t block_len, uint8_t* dst, size_t cap) {
  BlkPack pk;
  const int64_t P = block_len - 4;
  std::vector<BlkSpan> spans;
  uint64_t items = 0;
  for (size_t i = 0; i < n; ++i) {
    const BlkSpan s = blk_object_span(mode, o[i], block_len);
    if (s.status == CFSEC_OK && s.nb > 0) {
      if (items + (uint64_t)s.nb > kBlkMaxItems || pk.index.size() == kBlkMaxObjects) break;
      pk.index.push_back((uint32_t)i);
      spans.push_back(s);
      items += (uint64_t)s.nb;
    }
    pk.status.push_back(s.status);
    pk.taken = i + 1;
  }
  pk.objects = (uint32_t)pk.index.size();
  pk.items = (uint32_t)items;
  if (!pk.objects) return pk;
  const size_t objs_off = sizeof(BlkHead), map_off = objs_off + sizeof(BlkObject) * pk.objects;
  pk.bytes = (map_off + 4 * (size_t)pk.items + 15) / 16 * 16;
  if (!dst || cap < pk.bytes) return pk;

  std::memset(dst, 0, pk.bytes);
  BlkHead h{};
  h.nobjects = pk.objects, h.nitems = pk.items;
  h.mode = (uint32_t)mode, h.P = (uint32_t)P;
  h.objs_off = (uint32_t)objs_off, h.map_off = (uint32_t)map_off, h.bytes = (uint32_t)pk.bytes;
  h.xpow2[0] = xpow8(P);
  h.fin_full = shift_ones(h.xpow2[0]);
  for (int i = 1; i < 32; ++i) h.xpow2[i] = crc_mulmod(h.xpow2[i - 1], h.xpow2[i - 1]);
  std::memcpy(dst, &h, sizeof h);
  uint32_t item0 = 0;
  for (uint32_t j = 0; j < pk.objects; ++j) {
    const cfsec_blk_object& c = o[pk.index[j]];
    const BlkSpan& s = spans[j];
    BlkObject r{};
    r.src = (uint64_t)reinterpret_cast<uintptr_t>(c.src);
    r.size = (uint64_t)c.size;
    r.lo = 0, r.hi = (uint64_t)c.size;
    r.b0 = (uint32_t)s.b0, r.nb = (uint32_t)s.nb;
    r.item0 = item0, r.nblk = (uint32_t)s.nblk;
    const int64_t lens[2] = {P, c.size - (s.nblk - 1) * P};
    r.last_len = (uint32_t)lens[1];
    r.xlast = xpow8(lens[1]);
    r.fin_last = shift_ones(r.xlast);
    r.whole = s.whole ? 1u : 0u;
    if (s.whole) r.whole_fin = shift_ones(xpow8(c.size));
    if (mode == kBlkDecode) {
      r.lo = (uint64_t)c.from, r.hi = (uint64_t)c.to;
      r.dst = (uint64_t)reinterpret_cast<uintptr_t>(c.dst) - (uint64_t)c.from;
      const uint64_t d0 = r.dst + (uint64_t)(s.b0 * P);  // where payload byte 0 of block b0 belongs
      for (int i = 0; i < 2; ++i)
        for (int w = 0; w < 4; ++w)
          for (int dt = 0; dt < 2; ++dt) r.g[i][w][dt] = tile_end_factor(lens[i], (int64_t)((d0 + (uint64_t)(w * P)) & 15u), dt);
    } else {
      if (mode == kBlkEncode) r.dst = (uint64_t)reinterpret_cast<uintptr_t>(c.dst);
      r.h = (uint32_t)(((mode == kBlkEncode ? r.dst : r.src) + 4) & (mode == kBlkEncode ? 4095u : 15u));
      for (int i = 0; i < 2; ++i) r.g[i][0][0] = tile_end_factor(lens[i], r.h, 0);
    }
    std::memcpy(dst + objs_off + sizeof(BlkObject) * j, &r, sizeof r);
    uint32_t* map = reinterpret_cast<uint32_t*>(dst + map_off);
    for (uint32_t w = 0; w < r.nb; ++w) map[item0 + w] = j;
    item0 += r.nb;
  }
  return pk;
}

}  // namespace cfsec
