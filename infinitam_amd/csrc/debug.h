// debug.h -- the switches of include/itm_debug.h (itm_debug_set / itm_debug_get) as the library reads them: one table, indexed by key.
// Plain C++, host only.
#pragma once

#include "../../include/itm_debug.h"

namespace itm {

struct DebugSwitches {
  int value[ITM_DEBUG_KEY_COUNT] = {};
  constexpr DebugSwitches() {
    constexpr struct { int key, value; } defaults[] = {{ITM_DEBUG_EXCHANGE_CORRUPT_WORD, -1}};      // every other key starts at 0
    for (const auto& d : defaults) value[d.key] = d.value;
  }
  static constexpr bool known(int key) { return key > 0 && key < ITM_DEBUG_KEY_COUNT && !(key >= 21 && key <= 23); }
};
extern DebugSwitches g_debug;      // debug.hip

inline int debug_value(int key) { return g_debug.value[key]; }

}  // namespace itm
