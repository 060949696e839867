// blk_objects_driver.cpp -- asks libcfsec.so's pack_blk_objects (crc32block_objects.hpp) for
// tests/test_blk_objects_plan.py: the object table of a mixed-size crc32block launch, decoded back into
// text.  Host only: the addresses are numbers the test made up, never dereferenced; nothing is launched.
//
// Input (stdin), one case after another:
//   blk <mode: 0 check, 1 decode, 2 encode> <block_len> <n>
//   then n lines:  <src> <src_len> <dst> <size> <from> <to>
// Output per case:
//   pack <objects> <items> <bytes> <bytes the sizing pass gave> <taken>
//   status <n statuses>
//   index <the caller's index of every table object>
//   head <mode> <P> <fin_full> <xpow2[0 .. 32)>                                   (when objects > 0)
//   obj <src> <dst> <size> <lo> <hi> <b0> <nb> <item0> <nblk> <last_len> <fin_last> <whole> <whole_fin>
//       <xlast> <h> | <g[2][4][2]>                                                (per table object)
//   map <object of every work item>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "crc32block_objects.hpp"

using namespace cfsec;

int main() {
  std::string what;
  while (std::cin >> what) {
    if (what != "blk") return 1;
    int mode;
    int64_t block_len;
    size_t n;
    std::cin >> mode >> block_len >> n;
    std::vector<cfsec_blk_object> o(n);
    for (size_t i = 0; i < n; ++i) {
      uint64_t src, dst;
      std::cin >> src >> o[i].src_len >> dst >> o[i].size >> o[i].from >> o[i].to;
      o[i].src = reinterpret_cast<const uint8_t*>((uintptr_t)src);
      o[i].dst = reinterpret_cast<uint8_t*>((uintptr_t)dst);
    }
    const BlkPack sz = pack_blk_objects(mode, o.data(), n, block_len, nullptr, 0);
    std::vector<uint32_t> words((sz.bytes + 64) / 4 + 1, 0xEEEEEEEEu);  // 4-byte aligned
    uint8_t* buf = reinterpret_cast<uint8_t*>(words.data());
    const size_t room = sz.bytes + 64;
    if (sz.bytes > 0) {  // a buffer one byte short: nothing written
      const BlkPack none = pack_blk_objects(mode, o.data(), n, block_len, buf, sz.bytes - 1);
      for (size_t i = 0; i < room; ++i)
        if (buf[i] != 0xEE) return 3;
      if (none.bytes != sz.bytes || none.objects != sz.objects || none.items != sz.items) return 3;
    }
    const BlkPack pk = pack_blk_objects(mode, o.data(), n, block_len, buf, sz.bytes);
    for (size_t i = sz.bytes; i < room; ++i)
      if (buf[i] != 0xEE) return 4;  // wrote past the size it reported
    if (pk.status != sz.status || pk.index != sz.index || pk.items != sz.items || pk.taken != sz.taken) return 5;
    std::cout << "pack " << pk.objects << " " << pk.items << " " << pk.bytes << " " << sz.bytes << " " << pk.taken << "\n";
    std::cout << "status";
    for (int s : pk.status) std::cout << " " << s;
    std::cout << "\nindex";
    for (uint32_t i : pk.index) std::cout << " " << i;
    std::cout << "\n";
    if (!pk.objects) continue;
    BlkHead h;
    std::memcpy(&h, buf, sizeof h);
    if (h.nobjects != pk.objects || h.nitems != pk.items || h.bytes != pk.bytes || h.tabs || h.words) return 6;
    if (h.objs_off < sizeof h || h.map_off < h.objs_off + sizeof(BlkObject) * h.nobjects ||
        h.map_off + 4 * (size_t)h.nitems > h.bytes)
      return 6;
    std::cout << "head " << h.mode << " " << h.P << " " << h.fin_full;
    for (int i = 0; i < 32; ++i) std::cout << " " << h.xpow2[i];
    std::cout << "\n";
    for (uint32_t j = 0; j < h.nobjects; ++j) {
      BlkObject r;
      std::memcpy(&r, buf + h.objs_off + sizeof r * j, sizeof r);
      std::cout << "obj " << r.src << " " << r.dst << " " << r.size << " " << r.lo << " " << r.hi << " " << r.b0 << " "
                << r.nb << " " << r.item0 << " " << r.nblk << " " << r.last_len << " " << r.fin_last << " " << r.whole
                << " " << r.whole_fin << " " << r.xlast << " " << r.h << " |";
      for (int i = 0; i < 16; ++i) std::cout << " " << (&r.g[0][0][0])[i];
      std::cout << "\n";
    }
    std::cout << "map";
    const uint32_t* map = reinterpret_cast<const uint32_t*>(buf + h.map_off);
    for (uint32_t t = 0; t < h.nitems; ++t) std::cout << " " << map[t];
    std::cout << "\n";
  }
  return 0;
}
