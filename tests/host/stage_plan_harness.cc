// stage_plan_harness.cc — headtrackr_amd/csrc/ht_stage_plan.h (the arithmetic of a staged table) as a shared object for tests/test_stage_plan_cpu.py:
// compiled with g++, no HIP, called through ctypes.
#include <stdint.h>

#include "ht_stage_plan.h"

extern "C" int stage_slots(void) { return HT_STAGE_SLOTS; }
extern "C" uint64_t stage_capacity(uint64_t cap, uint64_t need, uint64_t minimum) { return ht_stage_capacity(cap, need, minimum); }
extern "C" int stage_next_slot(int slot) { return ht_stage_next_slot(slot); }
