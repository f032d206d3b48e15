"""The N-API shim (csrc/ht_napi.cc) behind its first two checks, without a GPU: linked against the recording C-ABI stub
(tests/js/abi_stub.cc) instead of the library, it is driven through tests/js/addon_calls.js — full calls, optional arguments omitted,
every argument of the wrong type, every boundary at its last accepted and first rejected value, dead contexts, freed buffers, every
failing C-ABI call — and must reproduce tests/golden/addon_calls.json call by call: thrown constructor and message, result digest and
the C-ABI calls made.  The golden was recorded from the shim before its argument handling was consolidated."""
import json

import pytest

import addon_stub

pytestmark = pytest.mark.skipif(not addon_stub.available(), reason="node / node_api.h / g++ not installed")


@pytest.fixture(scope="module")
def calls(tmp_path_factory):
    return addon_stub.run(addon_stub.NAPI_SRC, tmp_path_factory.mktemp("addon_stub"))


def test_addon_transcript_equals_the_recorded_one(calls):
    with open(addon_stub.GOLDEN) as f:
        golden = json.load(f)
    got = calls["transcript"]
    assert len(golden) > 900
    for i, (g, e) in enumerate(zip(golden, got)):
        assert e == g, (i, g["call"])
    assert len(got) == len(golden)


def test_device_ranges_that_used_to_wrap_are_refused(calls):
    """n * stride = 2^64 (or a byte offset of 1e30 converted to size_t) passed the range checks that multiplied before they compared and
    reached the C-ABI call with a range outside the buffer; every check now goes through frames_fit, which divides first.  The pairs form
    never could: a pair list is capped at 2^23 pairs."""
    assert len(calls["overflow"]) == 5
    for e in calls["overflow"]:
        assert e["ok"], (e["call"], e.get("threw"), e.get("message"), e["log"])
