"""The packed 4:2:2 formats in the JavaScript layer, on tests/js/mock_addon_422.js (no GPU): tests/js/ingest_422_cpu.js draws through
ccv.drawFrames and ccv.DeviceBatch; the canvases' CRC-32 are compared with tests/yuv422_cases.py here."""
import json
import os
import shutil
import subprocess

import pytest

import ingest_cases as ic
import yuv422_cases as y4
import yuv_cases as yc
from conftest import ROOT

NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node is missing on this machine")
def test_facade_draws_packed_422_frames_on_the_mock_addon(tmp_path):
    (sw, sh), (w, h) = (23, 23), (40, 30)
    videos, want = [], []
    for k, (fmt, matrix, rect) in enumerate(((y4.YUYV, 0, None), (y4.UYVY, 3, None), (y4.YUYV, 1, (1, 1, 21, 21)), (y4.UYVY, 2, (5, 3, 2, 2)))):
        frame = y4.raw_noise(sw, sh, fmt, 60 + k) if k & 1 else y4.from_rgb_frames("noise", sw, sh, 1, fmt, matrix, seed=60 + k)[0]
        assert frame.nbytes == y4.frame_bytes(sw, sh) == 4 * 12 * 23
        name = str(tmp_path / f"video_{k}.bin")
        frame.tofile(name)
        videos.append(dict(file=name, format=y4.FORMAT_NAMES[fmt], matrix=yc.MATRIX_NAMES[matrix], rect=list(rect) if rect else None))
        want.append(ic.crc(y4.expected(frame, sw, sh, fmt, matrix, rect, w, h)))
    (tmp_path / "job.json").write_text(json.dumps(dict(w=w, h=h, sw=sw, sh=sh, videos=videos)))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "ingest_422_cpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["crc"] == want and out["batch_checks"] == 2 and out["refusals"] >= 9
