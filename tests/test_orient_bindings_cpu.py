"""The orientation of a feed in the binding layers, without a GPU.  The JavaScript facade on tests/js/mock_addon_422.js
(tests/js/orient_cpu.js): ccv.drawFrames videos and ccv.DeviceBatch sources pack `orientation` into the format number, format | k << 8, and
refuse anything but an integer 0..7.  The N-API shim (csrc/ht_napi.cc) linked against the recording C-ABI stubs, the pattern of
tests/addon_stub.py (tests/js/orient_addon.js): a frame is sized and laid out by the bare format and the number reaches the C ABI whole.
(The Python layer's packing is in tests/test_orient_cpu.py.)  On the parent commit the facade ignores `orientation` and the shim sizes an
oriented YUYV frame as 4:2:0: both tests fail."""
import json
import os
import subprocess

import pytest

import addon_stub
from conftest import ROOT

JS = os.path.join(ROOT, "tests", "js")
RGBA, NV12, I420, YUYV, UYVY = 16, 0, 1, 4, 5


def O(k):  # noqa: E743
    return k << 8


@pytest.mark.skipif(addon_stub.NODE is None, reason="node is missing on this machine")
def test_facade_packs_the_orientation_into_the_format_number():
    r = subprocess.run([addon_stub.NODE, os.path.join(JS, "orient_cpu.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["yuv"] == [NV12 | O(5), I420 | O(1), YUYV | O(7), UYVY | O(2), NV12, I420]
    assert out["lists"] == [[YUYV | O(3), RGBA | O(6), NV12 | O(4), I420]]
    thrown = dict(out["thrown"])
    assert len(thrown) == 8
    for what, msg in thrown.items():
        assert msg is not None and msg.startswith("RangeError: ") and "orientation" in msg, (what, msg)
    assert "0..7" in thrown["drawFrames orientation 8"] and "0..7" in thrown["DeviceBatch orientation -1"]
    # the sizes drawFilterFactors asks about: 6 x 4 sources, the one under an odd orientation (3) as 4 x 6
    assert out["factors"] == [4, 6, 6, 4, 6, 4, 6, 4]


@pytest.mark.skipif(not addon_stub.available(), reason="node / g++ / node_api.h not installed")
def test_shim_lays_an_oriented_frame_out_by_its_bare_format(tmp_path):
    addon = str(tmp_path / "addon_orient.node")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "/usr/include/node", "-I", os.path.join(ROOT, "include"), "-DNAPI_VERSION=7",
                           "-DNODE_GYP_MODULE_NAME=headtrackr_hip", addon_stub.NAPI_SRC, os.path.join(JS, "abi_stub.cc"), os.path.join(JS, "draw_list_stub.cc"),
                           os.path.join(JS, "ingest_422_stub.cc"), "-o", addon])
    log, dl_log = str(tmp_path / "yuv.log"), str(tmp_path / "dl.log")
    r = subprocess.run([addon_stub.NODE, os.path.join(JS, "orient_addon.js"), addon], capture_output=True, text=True, timeout=120, env=dict(os.environ, HT_422_STUB_LOG=log, HT_DL_STUB_LOG=dl_log))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    W, H, F = 23, 7, 4 * 12 * 7
    calls = [json.loads(ln) for ln in open(log)]
    # (the stub's own "bytes" sizes a frame by the number it is given and knows no orientation: not looked at.  That the SHIM sizes an
    # oriented YUYV frame as 4:2:2 is the pair below: 2 F bytes pass, 2 F - 1 — more than two 4:2:0 frames — throw)
    host = [(c["n"], c["format"], c["rect"]) for c in calls if c["fn"] == "ht_draw_frames_yuv"]
    assert host == [(2, YUYV | O(5), None), (1, I420 | O(3), [0, 0, 7, 23])]
    assert 2 * F - 1 > 2 * (W * H + 2 * 12 * 4)
    dev = [(c["n"], c["format"], c["u"], c["v"], c["stride"]) for c in calls if c["fn"] == "ht_draw_frames_yuv_device"]
    assert dev == [(3, UYVY | O(7), None, None, F), (1, NV12 | O(1), W * H, None, 0), (1, I420 | O(6), W * H, W * H + 12 * 4, 0)]
    lists = [json.loads(ln) for ln in open(dl_log)]
    assert len(lists) == 1 and lists[0]["n"] == 4
    got = [(e["p0"], e["p1"], e["p2"], e["format"], e["rect"]) for e in lists[0]["entries"]]
    assert got == [(0, None, None, YUYV | O(1), [0, 0, 7, 23]), (3 - 8, W * H, W * H + 12 * 4, I420 | O(4), [0, 0, 0, 0]), (4 - 8, None, None, RGBA | O(3), [0, 0, 0, 0]),
                   (9 - 8, 15, None, NV12 | O(2), [0, 0, 0, 0])]
    thrown = dict(out["thrown"])
    assert set(thrown) == {"host form: oriented yuyv one byte short", "device form: oriented uyvy misaligned offset", "device form: oriented yuyv one byte beyond",
                           "list entry: oriented rgba one byte beyond", "list entry: oriented yuyv misaligned offset"}
    for what, msg in thrown.items():
        assert msg is not None and msg.startswith("RangeError: "), (what, msg)
    for what in ("device form: oriented uyvy misaligned offset", "list entry: oriented yuyv misaligned offset"):
        assert "multiple of 4" in thrown[what], thrown[what]
