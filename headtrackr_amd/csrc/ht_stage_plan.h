// ht_stage_plan.h — the arithmetic of a staged table (HtStagedTable, ht_internal.h): how large the table is after a reservation and which
// pinned slot a call takes.  Without HIP, so the CPU suite compiles and calls it (tests/host/stage_plan_harness.cc).
#pragma once

#include <stddef.h>

constexpr int HT_STAGE_SLOTS = 4;  // pinned slots per table: a call waits for the copy of the call HT_STAGE_SLOTS before it, practically never

// bytes the table holds after a reservation of `need`: what it has when that is enough (no reallocation), otherwise need, but at least the
// table's minimum — so that the first short list does not make every longer one reallocate
inline size_t ht_stage_capacity(size_t cap, size_t need, size_t minimum) { return cap >= need ? cap : need > minimum ? need : minimum; }

// the slot behind `slot`: the slots take turns
inline int ht_stage_next_slot(int slot) { return (slot + 1) % HT_STAGE_SLOTS; }
