"""The arithmetic of the staged tables (headtrackr_amd/csrc/ht_stage_plan.h: the capacity after a reservation, the slot a call takes) without a
device: the header is compiled with g++ into tests/host/stage_plan_harness.cc and called through ctypes.  The expectations are the scheme
as the four tables had it before it was written once — allocate max(need, minimum) when need exceeds the capacity, never shrink, slots in
turn —, and that ht_internal.h's HtStagedTable, and nothing else in the library, goes through these two functions."""
import ctypes as C
import os
import re
import subprocess

import pytest
from conftest import ROOT

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
DESC, CROP_DESC = 104, 120  # bytes of a draw-list and of a crop descriptor


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stage_plan") / "stage_plan.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "host", "stage_plan_harness.cc"), "-o", so])
    L = C.CDLL(so)
    L.stage_capacity.restype = C.c_uint64
    L.stage_capacity.argtypes = [C.c_uint64] * 3
    return L


def test_capacity_is_the_minimum_first_then_the_longest_list_and_never_shrinks(plan):
    for per, minimum in ((DESC, 64 * DESC), (CROP_DESC, 64 * CROP_DESC), (4, 6 * 17)):
        cap, reallocations = 0, 0
        for n in (3, 1, 64, 65, 3, 64, 65, 66, 4000, 65535, 1):
            new = plan.stage_capacity(cap, n * per, minimum)
            assert new == (cap if cap >= n * per else max(n * per, minimum)) and new >= cap and new >= n * per and new >= minimum, (per, n, cap, new)
            reallocations += new != cap
            cap = new
        # the first call and every list longer than all before it (and than the minimum): a list no longer than one before it reallocates nothing
        assert reallocations == (5 if minimum == 64 * per else 6) and cap == 65535 * per
    assert plan.stage_capacity(0, 1, 0) == 1 and plan.stage_capacity(7, 7, 100) == 7 and plan.stage_capacity(7, 8, 100) == 100
    assert plan.stage_capacity(0, 2 ** 40, 64) == 2 ** 40  # bytes are size_t: no 32-bit product


def test_slots_take_turns(plan):
    n = plan.stage_slots()
    assert n == 4
    seen, slot = [], 0
    for _ in range(3 * n):
        seen.append(slot)
        slot = plan.stage_next_slot(slot)
        assert 0 <= slot < n
    assert seen == list(range(n)) * 3  # a slot comes round again only after the other three


def test_the_scheme_exists_once():
    """ht_internal.h's four functions are the only place that allocates, stages and frees a table; the four users keep an instance each,
    with their minimum capacity and their allocation message"""
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc"))}
    internal = text["ht_internal.h"]
    assert '#include "ht_stage_plan.h"' in internal and internal.count("ht_stage_capacity(") == 1 and internal.count("ht_stage_next_slot(") == 1
    assert "hip" not in text["ht_stage_plan.h"].split("#pragma once")[1].lower()  # behind its header comment: no HIP
    for fn in ("ht_stage_reserve", "ht_stage_take", "ht_stage_commit", "ht_stage_free"):
        assert len(re.findall(r"^inline \w+ %s\(" % fn, internal, re.M)) == 1, fn
    assert sum(t.count("hipEventDisableTiming") for f, t in text.items() if f in ("ht_draw_list.hip", "ht_cs_pairs.hip", "ht_crop.hip", "ht_align.hip", "ht_ingest.hip")) == 0
    assert re.search(r"HtStagedTable dl_tab;", internal) and re.search(r"HtStagedTable csp_tab;", internal) and re.search(r"HtFaceCalls crop, align;", internal)
    users = {"ht_draw_list.hip": ("&c->dl_tab", "64 * sizeof(HtDrawDesc)", "allocation of the descriptor table failed"),
             "ht_cs_pairs.hip": ("&c->csp_tab", "(size_t)c->cs_streams * (2 * sizeof(CspEntry) / 4 + 1)", "allocation of the pair table failed"),
             "ht_face_calls.hip": ("&s.tab", "64 * sizeof(HtCropDesc)", '": allocation of the " + fam.word + " table failed"')}
    for f, (table, minimum, message) in users.items():
        assert text[f].count("ht_stage_reserve(c, " + table) == 1 and text[f].count("ht_stage_take(c, " + table) == 1 and text[f].count("ht_stage_commit(c, " + table) == 1, f
        assert minimum in text[f] and message in text[f], f
    assert sum(t.count("ht_stage_reserve(") for t in text.values()) == 1 + len(users)
    assert '{"crop", sizeof(ht_crop_record), &ht_ctx::crop,' in text["ht_face_calls.hip"] and '{"align", sizeof(ht_align_record), &ht_ctx::align,' in text["ht_face_calls.hip"]
