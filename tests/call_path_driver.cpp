// call_path_driver.cpp -- asks libcfsec.so which way a single-stripe call takes (single_call_path,
// engine.hpp) for tests/test_call_path.py.  Host only: no device is touched, nothing is launched.
//
// Input (stdin), one case per line:  <host> <rows_aliasable> <stage_usable> <moved_bytes> <nin> <mode>
//   mode: store | verify
// Output, one line per case: in_place | pinned_in_place | small_stage | pipeline | staged_whole
// A first line "small_pageable" answers RSEngine::kSmallPageable.
#include <iostream>
#include <string>

#include "engine.hpp"

using namespace cfsec;

int main() {
  std::string first;
  while (std::cin >> first) {
    if (first == "small_pageable") {
      std::cout << RSEngine::kSmallPageable << "\n";
      continue;
    }
    int aliasable, usable, nin;
    size_t moved;
    std::string mode;
    std::cin >> aliasable >> usable >> moved >> nin >> mode;
    if (!std::cin || (mode != "store" && mode != "verify")) return 1;
    const MatVecMode m = mode == "verify" ? MatVecMode::kVerify : MatVecMode::kStore;
    switch (single_call_path(first != "0", aliasable != 0, usable != 0, moved, nin, m)) {
      case CallPath::kInPlace: std::cout << "in_place\n"; break;
      case CallPath::kPinnedInPlace: std::cout << "pinned_in_place\n"; break;
      case CallPath::kSmallStage: std::cout << "small_stage\n"; break;
      case CallPath::kPipeline: std::cout << "pipeline\n"; break;
      case CallPath::kStagedWhole: std::cout << "staged_whole\n"; break;
    }
  }
  return 0;
}
