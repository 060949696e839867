// batch_runs_driver.cpp -- asks libcfsec.so's two pieces of batch host arithmetic (engine.hpp) for
// tests/test_batch_runs.py: the run splitter of a launch group (split_runs) and the staged-chunk packer
// (pack_chunk).  Host only: the addresses are numbers the test made up, never dereferenced; nothing is
// launched.
//
// Input (stdin), one case after another:
//   runs <k> <m> <mo> <nt>      then nt lines:  <len> <k in addrs> <m out addrs> <mo hout addrs>
//   pack <lane_bytes> <n>       then n lines:   <len> <nin> <nout> <nstore>
// Output, one line per case:
//   runs: "t0 t1" of every run, in order
//   pack: for every chunk "| i0 i1" followed by its row offsets
#include <cstdint>
#include <iostream>
#include <list>
#include <string>
#include <vector>

#include "engine.hpp"

using namespace cfsec;

int main() {
  std::string what;
  while (std::cin >> what) {
    if (what == "runs") {
      size_t k, m, mo, nt;
      std::cin >> k >> m >> mo >> nt;
      std::vector<const uint8_t*> in, out, hout;
      std::vector<uint64_t> lens(nt);
      const auto read = [](std::vector<const uint8_t*>* v, size_t n) {
        for (size_t i = 0; i < n; ++i) {
          uint64_t a;
          std::cin >> a;
          v->push_back(reinterpret_cast<const uint8_t*>((uintptr_t)a));
        }
      };
      for (size_t t = 0; t < nt; ++t) {
        std::cin >> lens[t];
        read(&in, k);
        read(&out, m);
        read(&hout, mo);
      }
      for (const auto& r : split_runs(in.data(), k, out.data(), m, hout.data(), mo, lens.data(), nt))
        std::cout << r.first << " " << r.second << " ";
      std::cout << "\n";
    } else if (what == "pack") {
      size_t lane_bytes, n;
      std::cin >> lane_bytes >> n;
      std::list<StripePlan> plans;
      std::vector<StripeTask> tasks(n);
      for (size_t i = 0; i < n; ++i) {
        size_t nin, nout;
        plans.emplace_back();
        std::cin >> tasks[i].len >> nin >> nout >> plans.back().nstore;
        plans.back().in.assign(nin, 0);
        plans.back().out.assign(nout, 0);
        tasks[i].plan = &plans.back();
      }
      std::vector<const StripeTask*> p;
      for (const StripeTask& t : tasks) p.push_back(&t);
      std::vector<size_t> off;
      for (size_t i0 = 0; i0 < n;) {
        const size_t i1 = pack_chunk(p.data(), n, i0, lane_bytes, &off);
        std::cout << "| " << i0 << " " << i1;
        for (size_t o : off) std::cout << " " << o;
        std::cout << " ";
        if (i1 <= i0) return 2;  // no progress: not the packer's contract
        i0 = i1;
      }
      std::cout << "\n";
    } else {
      return 1;
    }
  }
  return 0;
}
