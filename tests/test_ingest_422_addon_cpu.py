"""The N-API shim (csrc/ht_napi.cc) with the packed 4:2:2 formats, linked against recording C-ABI stubs (tests/js/abi_stub.cc,
tests/js/draw_list_stub.cc, tests/js/ingest_422_stub.cc) and driven by tests/js/ingest_422_addon.js: no GPU.  A 4:2:2 frame is 4 cw h bytes
(a buffer that exactly fits passes, one byte short throws); its one plane reaches the C ABI as y / p0 with u, v / p1, p2 NULL and pitches 0;
an offset that is no multiple of 4 throws a RangeError with a message; 4:2:0 is sized and laid out as before."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")


@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_shim_sizes_and_lays_out_packed_422_frames(tmp_path):
    addon = str(tmp_path / "addon_422.node")
    js = os.path.join(ROOT, "tests", "js")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "/usr/include/node", "-I", os.path.join(ROOT, "include"), "-DNAPI_VERSION=7",
                           "-DNODE_GYP_MODULE_NAME=headtrackr_hip", os.path.join(CSRC, "ht_napi.cc"), os.path.join(js, "abi_stub.cc"), os.path.join(js, "draw_list_stub.cc"),
                           os.path.join(js, "ingest_422_stub.cc"), "-o", addon])
    log, dl_log = str(tmp_path / "yuv.log"), str(tmp_path / "dl.log")
    r = subprocess.run([NODE, os.path.join(js, "ingest_422_addon.js"), addon], capture_output=True, text=True, timeout=120, env=dict(os.environ, HT_422_STUB_LOG=log, HT_DL_STUB_LOG=dl_log))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["consts"] == [4, 5, 0, 1, 16]
    W, H, F = 23, 7, 4 * 12 * 7
    pattern = lambda n: sum((i * 7 + 3) & 255 for i in range(n))  # noqa: E731  (the bytes ingest_422_addon.js fills its buffers with)
    calls = [json.loads(ln) for ln in open(log)]
    host = [c for c in calls if c["fn"] == "ht_draw_frames_yuv"]
    assert host == [
        dict(fn="ht_draw_frames_yuv", ctx=True, n=2, size=[W, H], format=4, matrix=1, stride=0, bytes=2 * F, sum=pattern(2 * F), rect=None),
        dict(fn="ht_draw_frames_yuv", ctx=True, n=1, size=[W, H], format=5, matrix=3, stride=0, bytes=F, sum=pattern(F), rect=[1, 1, 21, 5]),
        dict(fn="ht_draw_frames_yuv", ctx=True, n=1, size=[1, 1], format=1, matrix=0, stride=0, bytes=3, sum=pattern(3), rect=None)]
    dev = [c for c in calls if c["fn"] == "ht_draw_frames_yuv_device"]
    common = dict(fn="ht_draw_frames_yuv_device", ctx=True, y_set=True, pitch=[0, 0], size=[W, H])
    assert dev == [
        dict(common, n=3, u=None, v=None, stride=F, format=4, matrix=2, dst=True, dst_stride=0, rect=None),
        dict(common, n=2, u=None, v=None, stride=F + 8, format=5, matrix=0, dst=False, dst_stride=0, rect=[0, 0, 2, 2]),
        dict(common, n=1, u=W * H, v=None, stride=0, format=0, matrix=0, dst=True, dst_stride=0, rect=None)]
    lists = [json.loads(ln) for ln in open(dl_log)]
    whole = [0, 0, 0, 0]
    E_YUYV = dict(p1=None, p2=None, pitch=[0, 0], size=[W, H], format=4, matrix=1, rect=whole)
    E_UYVY = dict(p1=None, p2=None, pitch=[0, 0], size=[W, H], format=5, matrix=2, rect=[3, 1, 20, 6])
    E_NV12 = dict(p0=1, p1=15, p2=None, pitch=[0, 0], size=[5, 3], format=0, matrix=0, rect=whole)
    assert len(lists) == 2 and lists[0]["n"] == 4 and lists[0]["dst"] is None
    assert lists[0]["entries"] == [dict(E_YUYV, p0=0), E_NV12, dict(E_UYVY, p0=2 * F), dict(E_YUYV, p0=0)]
    assert lists[1]["n"] == 2 and lists[1]["entries"] == [dict(E_UYVY, p0=0), dict(E_YUYV, p0=-2 * F)]
    thrown = dict(out["thrown"])
    assert set(thrown) == {"host form one byte short", "host form: a 4:2:0-sized buffer is too short for 4:2:2", "device form one byte beyond", "device form misaligned offset",
                           "device form: stride with a gap beyond", "list entry one byte beyond", "list entry misaligned offset"}
    for what, msg in thrown.items():
        assert msg is not None and msg.startswith("RangeError: "), (what, msg)
    for what in ("device form misaligned offset", "list entry misaligned offset"):
        assert "multiple of 4" in thrown[what] and "YUYV / UYVY" in thrown[what], thrown[what]
