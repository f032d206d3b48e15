"""CPU-side checks of the context core: the frame registry (headtrackr_amd/csrc/ht_frame_registry.h — which live context has frames bound
where, and the ht_device_alloc buffers that outlived their owner) against a Python restatement, plain and under AddressSanitizer + UBSan;
its threaded mode under ThreadSanitizer (bindings published by their owners' threads while another thread retires buffers and sweeps);
and where the text of the frame calls and of the detect step lives.  Stand-alone programs, run directly.  No compute calls (no GPU here)."""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT
from headtrackr_amd import build

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")
FLAGS = {"plain": ["-O2"], "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-O1", "-g", "-fsanitize=thread"]}
A, B = 0x100000, 0x900000  # two buffers
N = 4096                   # ... of this many bytes


def _build_harness(tmp_path_factory, kind):
    exe = str(tmp_path_factory.mktemp("frame_registry") / ("frame_registry_harness_" + kind))
    subprocess.check_call(["g++", "-std=c++17", *FLAGS[kind], "-Wall", "-Werror", "-pthread", "-I", CSRC, os.path.join(ROOT, "tests", "host", "frame_registry_harness.cc"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build_harness(tmp_path_factory, "plain")


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """the same program with AddressSanitizer + UBSan linked in: a stand-alone executable, run directly"""
    return _build_harness(tmp_path_factory, "san")


@pytest.fixture(scope="module")
def harness_tsan(tmp_path_factory):
    """the same program with ThreadSanitizer linked in: a stand-alone executable, run directly"""
    return _build_harness(tmp_path_factory, "tsan")


def run(exe, tmp_path, script):
    path = str(tmp_path / "script.txt")
    with open(path, "w") as f:
        f.write("".join(" ".join(str(v) for v in op) + "\n" for op in script))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(script)
    return out


class Model:
    """the Python restatement: slots {number: [device, address]}, orphans in the order they were made"""

    def __init__(self):
        self.slots, self.orphans = {}, []

    def bound(self, skip, device, p, nbytes):
        return any(s != skip and d == device and a and p <= a < p + nbytes for s, (d, a) in self.slots.items())

    def sweep(self):
        gone = [o for o in self.orphans if not self.bound(None, o[2], o[0], o[1])]
        self.orphans = [o for o in self.orphans if o not in gone]
        return [o + [1] for o in gone]

    def step(self, op):
        release, answer = [], -1
        if op[0] == "add":
            self.slots[op[1]] = [op[2], 0]
        elif op[0] == "remove":
            del self.slots[op[1]]
        elif op[0] == "publish":
            self.slots[op[1]][1] = op[2]
        elif op[0] == "retire":
            for p, nbytes in zip(op[3::2], op[4::2]):
                if self.bound(None, op[1], p, nbytes):
                    self.orphans.append([p, nbytes, op[1]])
                else:
                    release.append([p, nbytes, op[1], 0])
            release += self.sweep()  # the owner's own buffers first, then older orphans that have become free
        elif op[0] == "sweep":
            release = self.sweep()
        elif op[0] == "query":
            answer = int(self.bound(op[1], op[2], op[3], op[4]))
        return dict(op=op[0], answer=answer, release=release, orphans=[list(o) for o in self.orphans])


def scripts():
    """-> {name: (script, {step index: the release list or answer the case is about})}"""
    s = {}
    # the owner (slot 0) is retired while a binder (slot 1) is inside: the buffer becomes an orphan; the binder moves away: the sweep releases it
    s["orphan, then the binder moves away"] = ([
        ("add", 0, 0), ("add", 1, 0), ("publish", 0, A), ("publish", 1, A + 64), ("remove", 0), ("retire", 0, 2, A, N, B, N), ("sweep",),
        ("publish", 1, B + N), ("sweep",), ("sweep",)],
        {5: [[B, N, 0, 0]], 6: [], 8: [[A, N, 0, 1]], 9: []})
    # two binders: only the last one leaving releases; unbinding counts as leaving
    s["two binders"] = ([
        ("add", 0, 0), ("add", 1, 0), ("add", 2, 0), ("publish", 1, A), ("publish", 2, A + N - 4), ("remove", 0), ("retire", 0, 1, A, N),
        ("publish", 1, B), ("sweep",), ("publish", 2, 0), ("sweep",)],
        {6: [], 8: [], 10: [[A, N, 0, 1]]})
    # a binding at the first byte, at the last byte and one past the end of a buffer; one before its start
    s["edges"] = ([
        ("add", 1, 0), ("publish", 1, A), ("query", -1, 0, A, N), ("publish", 1, A + N - 1), ("query", -1, 0, A, N), ("publish", 1, A + N), ("query", -1, 0, A, N),
        ("publish", 1, A - 1), ("query", -1, 0, A, N), ("publish", 1, A + N - 1), ("retire", 0, 1, A, N), ("publish", 1, A + N), ("sweep",),
        ("query", -1, 0, A, 0), ("publish", 1, 0), ("query", -1, 0, 0, N)],
        {2: 1, 4: 1, 6: 0, 8: 0, 10: [], 12: [[A, N, 0, 1]], 13: 0, 15: 0})
    # the same address on another device does not count
    s["another device"] = ([
        ("add", 1, 1), ("publish", 1, A + 8), ("query", -1, 0, A, N), ("query", -1, 1, A, N), ("retire", 0, 1, A, N), ("retire", 1, 1, A, N), ("remove", 1), ("sweep",)],
        {2: 0, 3: 1, 4: [[A, N, 0, 0]], 5: [], 7: [[A, N, 1, 1]]})
    # ht_device_free's question leaves the asking context out: bound inside its own buffer it may free it, another one inside forbids it
    s["except"] = ([
        ("add", 0, 0), ("add", 1, 0), ("publish", 0, A + 16), ("query", 0, 0, A, N), ("query", -1, 0, A, N), ("query", 1, 0, A, N), ("publish", 1, A + 32),
        ("query", 0, 0, A, N), ("query", 1, 0, A, N)],
        {3: 0, 4: 1, 5: 1, 7: 1, 8: 1})
    # a retire finds older orphans releasable: they follow the owner's own buffers, in the order they were orphaned
    s["retire sweeps"] = ([
        ("add", 0, 0), ("add", 1, 0), ("add", 2, 0), ("publish", 2, A), ("remove", 0), ("retire", 0, 1, A, N), ("publish", 2, B + 4), ("remove", 1),
        ("retire", 0, 2, B, N, B + N, N), ("publish", 2, 0), ("remove", 2), ("retire", 0, 1, 3 * B, N)],
        {5: [], 8: [[B + N, N, 0, 0], [A, N, 0, 1]], 11: [[3 * B, N, 0, 0], [B, N, 0, 1]]})
    return s


@pytest.mark.parametrize("name", list(scripts()))
def test_registry_matches_the_restatement(harness, tmp_path, name):
    script, about = scripts()[name]
    got, model = run(harness, tmp_path, script), Model()
    for i, (op, g) in enumerate(zip(script, got)):
        assert g == model.step(list(op)), (name, i, op, g)
        if i in about:  # the case is the case it was written as
            assert (g["answer"] if op[0] == "query" else g["release"]) == about[i], (name, i, op, g)


def test_registry_under_the_sanitizers(harness, harness_san, tmp_path):
    for name, (script, _) in scripts().items():
        assert run(harness_san, tmp_path, script) == run(harness, tmp_path, script), name


def test_bindings_published_while_another_thread_sweeps_are_no_race(harness_tsan):
    """two threads move their bindings among four buffers 4000 times each and sweep behind every move, a third retires the buffers and
    sweeps; under ThreadSanitizer: no report (empty stderr, status 0), and every retired buffer was released exactly once"""
    r = subprocess.run([harness_tsan, "--threads", "4000"], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr[-3000:])
    got = json.loads(r.stdout)
    assert got["retired"] == got["released"] == 2000 and got["twice"] == got["never"] == got["unknown"] == got["orphans_left"] == 0, got


def function_bodies(text):
    """{name: body} of the functions defined at column 0 of a file of this project's layout (the closing brace at column 0)"""
    return {m.group(1): m.group(2) for m in re.finditer(r"^[\w\"][^\n;{}]*?\b(\w+)\([^;{}]*\)(?: const)? \{(?:  //[^\n]*)?\n(.*?)^\}", text, re.M | re.S)}


def test_where_the_context_core_lives():
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc", ".cc"))}
    everything = "".join(text.values())
    registry, frames, step, ctx = text["ht_frame_registry.h"], text["ht_frames.hip"], text["ht_detect_step.hip"], text["ht_context.hip"]
    assert "#include <hip" not in registry and "ht_internal.h" not in registry.split("#pragma once")[1] and "hip" not in registry.split("#pragma once")[1].lower()
    # the two files are compiled as part of ht_context.hip; the list of translation units is what it was
    assert ctx.count('#include "ht_frames.hip"') == 1 and ctx.count('#include "ht_detect_step.hip"') == 1
    assert sum(t.count('#include "ht_frames.hip"') + t.count('#include "ht_detect_step.hip"') for t in text.values()) == 2
    assert build.HIP_SOURCES == ["ht_context.hip", "ht_pyramid.hip", "ht_scan.hip", "ht_camshift.hip", "ht_backproject.hip", "ht_allgather.hip"]
    assert "__global__" not in frames and "__global__" not in step and "__global__" not in ctx
    # ONE writer of the binding: a member d_frames, frame_stride or nframes is assigned in one function of ht_frames.hip and nowhere else
    assign = r"(?:->|\.)\s*(?:d_frames|frame_stride|nframes)\s*=(?!=)"
    for f, t in text.items():
        if f != "ht_frames.hip":
            t = re.sub(r"\bg->(frames|frame_stride|nframes)\b|\bka\.frame_stride\b|\bd\.frame_stride\b", "", t)  # a graph's key; kernel arguments; the addon's own record
            assert not re.search(assign, t), (f, re.search(assign, t).group(0))
        assert not re.search(r"\bd_frames\s*=\s*(?:nullptr|NULL|0)\s*[,;)]", t.replace("const uint8_t *d_frames = nullptr;", "")), f  # (the member's initialiser)
    writers = [name for name, body in function_bodies(frames).items() if re.search(assign, body)]
    assert writers == ["ht_frames_set"] and len(re.findall(assign, frames)) == 3
    assert "HtFrameRegistry::publish(&c->frame_slot, frames)" in function_bodies(frames)["ht_frames_set"] and everything.count("HtFrameRegistry::publish(") == 1
    # what carried arguments through the context, and the old bookkeeping, are gone
    for gone in ("collect_best_follows", "h_sort_deferred", "requeue_flags = ", "->requeue_flags", "g_orphans", "bound_by_live_context", "g_live", "HtOrphan"):
        assert gone not in everything, gone
    assert not re.search(r"\brequeue_flags\b", text["ht_internal.h"])
    # one device-wide synchronisation, in release_buffers, which ht_destroy and the sweep share; the sweeps are where they were
    assert (ctx + frames + step).count("hipDeviceSynchronize") == 1 and "hipDeviceSynchronize" in function_bodies(ctx)["release_buffers"]
    assert ctx.count("release_buffers(") == 2 and frames.count("release_buffers(") == 1 and everything.count("release_buffers(") == 3
    sweeping = sorted(name for name, body in function_bodies(frames).items() if "sweep_orphans(c)" in body)
    assert sweeping == ["ht_bind_frames_device", "ht_device_free", "ht_frames_bind_own"] and "ht_frames_bind_own(c, n)" in function_bodies(frames)["ht_swap_frames"]
    assert everything.count("g_frames.sweep()") == 1 and everything.count("g_frames.retire(") == 1 and everything.count("g_frames.bound_inside(") == 1
    # every entry point that moved is defined once, in its file
    moved = {"ht_frames.hip": ("ht_upload_frames", "ht_upload_frames_async", "ht_swap_frames", "ht_bind_frames_device", "ht_frames_bound", "ht_frames_enqueued", "ht_host_alloc",
                               "ht_host_free", "ht_device_alloc", "ht_device_free", "ht_device_upload", "ht_device_download"),
             "ht_detect_step.hip": ("ht_detect_enqueue", "ht_detect_collect", "ht_detect_collect_best", "ht_detect_collect_best_requeue", "ht_detect_batch",
                                    "ht_whitebalance_batch", "ht_detect_whitebalance", "ht_graph_launches")}
    for f, names in moved.items():
        for fn in names:
            pat = r'^extern "C" \w+ %s\(' % fn
            assert len(re.findall(pat, text[f], re.M)) == 1 and sum(len(re.findall(pat, t, re.M)) for t in text.values()) == 1, fn
    for fn in ("ht_frames_own_reserve", "ht_frames_bind_own", "ht_frames_set"):
        assert len(re.findall(r"^\w+ %s\([^;]*\) \{" % fn, frames, re.M)) == 1, fn
    # the collect calls are thin callers of one body; the shared head is used by both collects; the graph cache's entry is dropped in one place
    bodies = function_bodies(step)
    for inner, callers in (("detect_collect", ("ht_detect_collect", "detect_collect_best")), ("detect_collect_best", ("ht_detect_collect_best", "ht_detect_collect_best_requeue"))):
        assert sorted(name for name, body in bodies.items() if re.search(r"(?<!\w)%s\(c, " % inner, body)) == sorted(callers), inner
    assert everything.count("ht_detect_fetch(c, ") == 2 and "ht_detect_fetch(c, " in text["ht_group.hip"] and "ht_detect_fetch(c, " in bodies["detect_collect"]
    assert everything.count("ht_detect_mark_collected(") == 2  # defined, called by the fetch
    assert everything.count("hipGraphExecDestroy(") == 1 and step.count("graph_drop(") == 3
    assert "1 << 30" in bodies["graph_capture"] and step.count("ht_capture_mark(c, true)") == 1 and step.count("ht_capture_mark(c, false)") == 2
    assert "hipMemsetAsync" not in bodies["detect_enqueue_body"] and "hipMemsetAsync" not in bodies["graph_capture"] and "NEVER captured" in step
    assert step.count("a counting sort by frame") == 1  # the comment that stood twice
