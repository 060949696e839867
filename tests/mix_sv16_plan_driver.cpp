// mix_sv16_plan_driver.cpp -- asks libcfsec.so's pack_mix_sv16 (engine.hpp) for tests/test_mix_sv16_plan.py:
// the item table of the mixed-plan repair launch of the 16 + 20 code (gf_mix_sv16.hpp), decoded back into
// text.  Host only: the row addresses, the Verify word addresses, the table-block address and the word
// address are numbers the test made up, never dereferenced; nothing is launched.
//
// Input (stdin), one case after another:
//   mixsv16 <max_len> <nwords> <tabs> <crc> <nplans> <ntasks>
//   then nplans lines:  <k> <m> <nstore> <dy16: 0|1> <k input shard indices> <m output shard indices>
//                       and, with dy16 = 1:  <nd> <e> <pstore> <pcmp> <16 src> <nd + 20 + e row indices>
//                                            <(20 + e + nd) * 16 coefficient bytes>
//   then ntasks lines:  <plan index> <len> <crc mode> <owner> <crc_word> <remap: 0|1> <split> <flag addr>
//                       <k input addrs> <m output addrs>
// Output per case:
//   pack <items> <tiles> <plans> <bytes> <bytes the sizing pass gave>
//   left <indices of the tasks not packed>
//   head <tabs> <crc> <the 24 powers x^(8 * 4096 * 2^q)>
//   item <len> <coef offset> <tile0> <ntiles> <fin> <gend> <flag addr> <nd> <e> <pstore> <pcmp> <src[0..4)> |
//        <16 + nd + 20 + e row addrs> | <as many words> | <(20 + e + nd) * 16 coefficient bytes>   (per item)
//   map <item of every launch tile>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <list>
#include <memory>
#include <string>
#include <vector>

#include "engine.hpp"
#include "gf_mix_sv16.hpp"

using namespace cfsec;

int main() {
  std::string what;
  while (std::cin >> what) {
    if (what != "mixsv16") return 1;
    size_t max_len, nwords, nplans, ntasks;
    uint64_t tabs, crc;
    std::cin >> max_len >> nwords >> tabs >> crc >> nplans >> ntasks;
    std::vector<std::unique_ptr<StripePlan>> plans;
    for (size_t p = 0; p < nplans; ++p) {
      size_t k, m;
      int nstore, dy;
      std::cin >> k >> m >> nstore >> dy;
      plans.emplace_back(new StripePlan());
      StripePlan& pl = *plans.back();
      pl.in.assign(k, 0);
      pl.out.assign(m, 0);
      for (int& c : pl.in) std::cin >> c;
      for (int& r : pl.out) std::cin >> r;
      pl.nstore = nstore;
      if (dy) {
        auto d = std::make_shared<Dy16Plan>();
        std::cin >> d->nd >> d->e >> d->pstore >> d->pcmp;
        for (int i = 0; i < 16; ++i) {
          int v;
          std::cin >> v;
          d->src[i] = (uint8_t)v;
        }
        d->rows.assign((size_t)(d->nd + 20 + d->e), 0);
        for (int& r : d->rows) std::cin >> r;
        d->coef = Matrix(20 + d->e + d->nd, 16);
        for (uint8_t& b : d->coef.v) {
          int v;
          std::cin >> v;
          b = (uint8_t)v;
        }
        pl.dy16 = std::move(d);
      }
    }
    std::vector<StripeTask> tasks(ntasks);
    std::vector<uint64_t> flags(ntasks);
    std::list<std::vector<uint8_t*>> addrs;
    std::vector<uint8_t* const*> rows;
    std::vector<int> identity(64);
    for (int i = 0; i < 64; ++i) identity[i] = i;
    for (size_t i = 0; i < ntasks; ++i) {
      size_t p;
      int remap;
      std::cin >> p >> tasks[i].len >> tasks[i].crc >> tasks[i].owner >> tasks[i].crc_word >> remap >> tasks[i].split >>
          flags[i];
      tasks[i].plan = plans[p].get();
      if (remap) tasks[i].crc_map = identity.data();
      addrs.emplace_back();
      for (size_t r = 0; r < plans[p]->in.size() + plans[p]->out.size(); ++r) {
        uint64_t a;
        std::cin >> a;
        addrs.back().push_back(reinterpret_cast<uint8_t*>((uintptr_t)a));
      }
      rows.push_back(addrs.back().data());
    }
    std::vector<const StripeTask*> tp;
    for (const StripeTask& t : tasks) tp.push_back(&t);
    const auto pack = [&](uint8_t* dst, size_t cap) {
      return pack_mix_sv16(tp.data(), rows.data(), flags.data(), ntasks, max_len, nwords, tabs, crc, nullptr, dst, cap);
    };
    const MixPack sz = pack(nullptr, 0);
    std::vector<uint8_t> buf(sz.bytes + 64, 0xEE);
    if (sz.bytes > 0) {  // a buffer one byte short: nothing written
      const MixPack none = pack(buf.data(), sz.bytes - 1);
      for (uint8_t b : buf)
        if (b != 0xEE) return 3;
      if (none.bytes != sz.bytes) return 3;
    }
    const MixPack pk = pack(buf.data(), sz.bytes);
    for (size_t i = sz.bytes; i < buf.size(); ++i)
      if (buf[i] != 0xEE) return 4;  // wrote past the size it reported
    std::cout << "pack " << pk.items << " " << pk.tiles << " " << pk.plans << " " << pk.bytes << " " << sz.bytes << "\n";
    std::cout << "left";
    for (size_t i : pk.left) std::cout << " " << i;
    std::cout << "\n";
    if (pk.items) {
      MixCrcHead h;
      std::memcpy(&h, buf.data(), sizeof h);
      if (h.nitems != pk.items || h.ntiles != pk.tiles || h.nplans != pk.plans || h.bytes != pk.bytes) return 5;
      std::cout << "head " << h.tabs << " " << h.crc;
      for (uint32_t x : h.xpow2) std::cout << " " << x;
      std::cout << "\n";
      const uint8_t* item = buf.data() + h.items_off;
      const uint8_t* row = buf.data() + h.rows_off;
      const uint8_t* word = buf.data() + h.words_off;
      const uint8_t* map = buf.data() + h.map_off;
      if (h.rows_off != h.items_off + h.nitems * sizeof(MixSv16Item)) return 7;
      for (uint32_t j = 0; j < h.nitems; ++j) {
        MixSv16Item it;
        std::memcpy(&it, item + (size_t)j * sizeof it, sizeof it);
        const uint32_t nrows = 16u + it.nd + 20u + it.e, ncoef = (20u + it.e + it.nd) * 16u;
        if (it.coef < h.coef_off || it.coef + (size_t)ncoef > h.bytes) return 6;
        std::cout << "item " << it.len << " " << it.coef << " " << it.tile0 << " " << it.ntiles << " " << it.fin << " "
                  << it.gend << " " << it.flag << " " << (int)it.nd << " " << (int)it.e << " " << it.pstore << " "
                  << it.pcmp;
        for (int q = 0; q < 4; ++q) std::cout << " " << (int)it.src[q];
        std::cout << " |";
        for (uint32_t r = 0; r < nrows; ++r) {
          uint64_t a;
          std::memcpy(&a, row + (size_t)(it.rows + r) * 8, 8);
          std::cout << " " << a;
        }
        std::cout << " |";
        for (uint32_t r = 0; r < nrows; ++r) {
          uint32_t w;
          std::memcpy(&w, word + (size_t)(it.rows + r) * 4, 4);
          std::cout << " " << w;
        }
        std::cout << " |";
        for (uint32_t c = 0; c < ncoef; ++c) std::cout << " " << (int)buf[it.coef + c];
        std::cout << "\n";
      }
      std::cout << "map";
      for (uint32_t t = 0; t < h.ntiles; ++t) {
        uint32_t v;
        std::memcpy(&v, map + (size_t)t * 4, 4);
        std::cout << " " << v;
      }
      std::cout << "\n";
    }
  }
  return 0;
}
