// mix_plan_driver.cpp -- asks libcfsec.so's pack_mix (engine.hpp) for tests/test_mix_plan.py: the item
// table of a mixed-plan launch (gf_mix.hpp), decoded back into text.  Host only: the row addresses are
// numbers the test made up, never dereferenced; nothing is launched.
//
// Input (stdin), one case after another:
//   mix <max_len> <nplans> <ntasks>
//   then nplans lines:  <k> <m> <nstore> <dy16: 0|1> <m * k coefficient bytes>
//   then ntasks lines:  <plan index> <len> <crc> <k input addrs> <m output addrs>
// Output per case:
//   pack <items> <tiles> <plans> <bytes> <bytes the sizing pass gave>
//   left <indices of the tasks not packed>
//   item <len> <k> <m> <coef offset> <tile0> <ntiles> | <k + m row addrs> | <m * k coefficient bytes>   (per item)
//   map <item of every launch tile>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <list>
#include <memory>
#include <string>
#include <vector>

#include "engine.hpp"
#include "gf_mix.hpp"

using namespace cfsec;

int main() {
  std::string what;
  while (std::cin >> what) {
    if (what != "mix") return 1;
    size_t max_len, nplans, ntasks;
    std::cin >> max_len >> nplans >> ntasks;
    std::vector<std::unique_ptr<StripePlan>> plans;
    for (size_t p = 0; p < nplans; ++p) {
      size_t k, m;
      int nstore, dy;
      std::cin >> k >> m >> nstore >> dy;
      plans.emplace_back(new StripePlan());
      StripePlan& pl = *plans.back();
      pl.in.assign(k, 0);
      pl.out.assign(m, 0);
      pl.nstore = nstore;
      pl.rows = Matrix((int)m, (int)k);
      for (size_t i = 0; i < m * k; ++i) {
        int v;
        std::cin >> v;
        pl.rows.v[i] = (uint8_t)v;
      }
      if (dy) pl.dy16 = std::make_shared<Dy16Plan>();
    }
    std::vector<StripeTask> tasks(ntasks);
    std::list<std::vector<uint8_t*>> addrs;
    std::vector<uint8_t* const*> rows;
    for (size_t i = 0; i < ntasks; ++i) {
      size_t p;
      std::cin >> p >> tasks[i].len >> tasks[i].crc;
      tasks[i].plan = plans[p].get();
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
    const MixPack sz = pack_mix(tp.data(), rows.data(), ntasks, max_len, nullptr, 0);
    std::vector<uint8_t> buf(sz.bytes + 64, 0xEE);
    if (sz.bytes > 0) {  // a buffer one byte short: nothing written
      const MixPack none = pack_mix(tp.data(), rows.data(), ntasks, max_len, buf.data(), sz.bytes - 1);
      for (uint8_t b : buf)
        if (b != 0xEE) return 3;
      if (none.bytes != sz.bytes) return 3;
    }
    const MixPack pk = pack_mix(tp.data(), rows.data(), ntasks, max_len, buf.data(), sz.bytes);
    for (size_t i = sz.bytes; i < buf.size(); ++i)
      if (buf[i] != 0xEE) return 4;  // wrote past the size it reported
    std::cout << "pack " << pk.items << " " << pk.tiles << " " << pk.plans << " " << pk.bytes << " " << sz.bytes << "\n";
    std::cout << "left";
    for (size_t i : pk.left) std::cout << " " << i;
    std::cout << "\n";
    if (pk.items) {
      MixHead h;
      std::memcpy(&h, buf.data(), sizeof h);
      if (h.nitems != pk.items || h.ntiles != pk.tiles || h.nplans != pk.plans || h.bytes != pk.bytes) return 5;
      const MixItem* item = reinterpret_cast<const MixItem*>(buf.data() + h.items_off);
      const uint64_t* row = reinterpret_cast<const uint64_t*>(buf.data() + h.rows_off);
      const uint32_t* map = reinterpret_cast<const uint32_t*>(buf.data() + h.map_off);
      for (uint32_t j = 0; j < h.nitems; ++j) {
        const MixItem& it = item[j];
        if (it.coef < h.coef_off || it.coef + (size_t)it.k * it.m > h.bytes) return 6;
        std::cout << "item " << it.len << " " << it.k << " " << it.m << " " << it.coef << " " << it.tile0 << " "
                  << it.ntiles << " |";
        for (uint32_t r = 0; r < it.k + it.m; ++r) std::cout << " " << row[it.rows + r];
        std::cout << " |";
        for (uint32_t c = 0; c < it.k * it.m; ++c) std::cout << " " << (int)buf[it.coef + c];
        std::cout << "\n";
      }
      std::cout << "map";
      for (uint32_t t = 0; t < h.ntiles; ++t) std::cout << " " << map[t];
      std::cout << "\n";
    }
  }
  return 0;
}
