"""Builds an ht_napi.cc together with tests/js/abi_stub.cc (the recording stand-in for the C ABI) into a temporary .node and runs
tests/js/addon_calls.js on it.  Shared by tests/test_addon_calls_cpu.py and tests/golden/make_addon_calls_golden.py.  The flags are
build.build_addon's, with the stub in place of -lheadtrackr_hip; the product addon (headtrackr_amd/js/headtrackr_hip.node) is never written."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
NODE_API = "/usr/include/node/node_api.h"
GOLDEN = os.path.join(ROOT, "tests", "golden", "addon_calls.json")
NAPI_SRC = os.path.join(ROOT, "headtrackr_amd", "csrc", "ht_napi.cc")


def available():
    return NODE is not None and shutil.which("g++") is not None and os.path.exists(NAPI_SRC) and os.path.exists(NODE_API)


def build(napi_src, out_dir):
    out = os.path.join(str(out_dir), "addon_stub.node")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "/usr/include/node", "-I", os.path.join(ROOT, "include"), "-DNAPI_VERSION=7",
                           "-DNODE_GYP_MODULE_NAME=headtrackr_hip", napi_src, os.path.join(ROOT, "tests", "js", "abi_stub.cc"), "-o", out])
    return out


def run(napi_src, out_dir):
    """-> {"transcript": [...], "overflow": [...]} of tests/js/addon_calls.js on napi_src + stub"""
    addon = build(napi_src, out_dir)
    log, res = os.path.join(str(out_dir), "stub.log"), os.path.join(str(out_dir), "calls.json")
    if os.path.exists(log):
        os.unlink(log)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "addon_calls.js"), addon, res], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HT_STUB_LOG=log))
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    with open(res) as f:
        return json.load(f)


def dump(transcript, path):
    """one entry per line: a change shows up as that call's line in a diff"""
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in transcript) + "\n]\n")
