#!/usr/bin/env python3
"""tools/gpu_group.py [output file] | --publish FILE — (no argument: profiles/group_device.txt and its section of profiles/README.md) — what moving the grouping and the best-face selection onto the
device costs and saves, measured in ONE process with the two routes taking turns:

  1. device time of the k_grp_* launches (ht_profile / ht_kernel_times, HIP events) for a 256 x 320x240 and a 128 x 1280x720 batch of the
     benchmark's frame mix: grp_bucket = count + scan + scatter, grp_frames = one workgroup per frame;
  2. wall clock per step of the three-context C2 loop (256 x 320x240, the benchmark's run_steps) on the device route
     (ht_detect_best_enqueue / ht_detect_best_collect_requeue) and on the host route (ht_detect_collect_best_requeue), alternating blocks;
  3. the process's CPU time per step (user + system, all threads: the host route's worker pool included) for both routes.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from headtrackr_amd import native, synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

DEPTH, BLOCK_STEPS, BLOCKS, WARM = 3, 400, 6, 60
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def kernel_times(w, h, n, reps=20):
    frames = torch.from_numpy(synth.mixed_batch(n, w, h, seed0=1234)).cuda()
    c = Context()
    try:
        c.set_geometry(w, h, n)
        c.bind_device(frames.data_ptr(), n)
        for _ in range(3):
            c.detect_enqueue()
            c.detect_best_enqueue(1, 0)
            best, hits = c.detect_best_collect()
        c.profile(True)
        c.kernel_times(reset=True)
        for _ in range(reps):
            c.detect_enqueue()
            c.detect_best_enqueue(1, 0)
            c.detect_best_collect()
        kt = c.kernel_times(reset=True)
        c.profile(False)
        grp = {k: v["ms"] / reps * 1e3 for k, v in kt.items() if k.startswith("grp_")}
        rest = sum(v["ms"] for k, v in kt.items() if not k.startswith("grp_")) / reps * 1e3
        say(f"{n} x {w}x{h}: {hits} raw hits, {int((best['neighbors'] > 0).sum())} frames with a face; device us per batch: "
            + ", ".join(f"{k} {v:.1f}" for k, v in sorted(grp.items())) + f"; all other kernels of the batch {rest:.1f}")
        return grp
    finally:
        c.close()
        del frames


def loop(ctxs, k, device_route, bufs):
    """the benchmark's run_steps: k batches, DEPTH in flight, every collect re-enqueues its context while batches remain"""
    started = min(len(ctxs), k)
    for i in range(started):
        ctxs[i].detect_enqueue()
        if device_route:
            ctxs[i].detect_best_enqueue(1, 0)
    for i in range(k):
        cx = ctxs[i % len(ctxs)]
        more = started < k
        if device_route:
            out = cx.detect_best_collect_requeue(bufs[i % len(ctxs)]) if more else cx.detect_best_collect(bufs[i % len(ctxs)])
        else:
            out = cx.detect_collect_best_requeue(1, bufs[i % len(ctxs)]) if more else cx.detect_collect_best(1, bufs[i % len(ctxs)])
        if more:
            started += 1
    return out


def c2_loop():
    w, h, n = 320, 240, 256
    frames = torch.from_numpy(synth.mixed_batch(n, w, h, seed0=1234)).cuda()
    routes = {}
    for name in ("host", "device"):
        ctxs = []
        for _ in range(DEPTH):
            c = Context()
            c.set_geometry(w, h, n)
            c.bind_device(frames.data_ptr(), n)
            ctxs.append(c)
        routes[name] = (ctxs, [np.zeros(n, dtype=native.RECT_DTYPE) for _ in range(DEPTH)])
    ref = {}
    for name, (ctxs, bufs) in routes.items():
        best, hits = loop(ctxs, WARM, name == "device", bufs)
        ref[name] = (best.tobytes(), hits)
    say(f"C2 loop, {n} x {w}x{h}, {DEPTH} contexts in flight: both routes return the same bytes: {ref['host'] == ref['device']} ({ref['host'][1]} raw hits)")
    wall = {"host": [], "device": []}
    cpu = {"host": [], "device": []}
    for b in range(BLOCKS):
        for name in (("host", "device") if b % 2 == 0 else ("device", "host")):  # alternated: both routes see the same machine state
            ctxs, bufs = routes[name]
            torch.cuda.synchronize()
            t0, c0 = time.perf_counter(), time.process_time()
            loop(ctxs, BLOCK_STEPS, name == "device", bufs)
            t1, c1 = time.perf_counter(), time.process_time()
            wall[name].append((t1 - t0) / BLOCK_STEPS * 1e3)
            cpu[name].append((c1 - c0) / BLOCK_STEPS * 1e3)
    for name in ("host", "device"):
        say(f"  {name:6s} route: wall ms/step per block {[round(v, 4) for v in wall[name]]} median {np.median(wall[name]):.4f} "
            f"spread {max(wall[name]) - min(wall[name]):.4f}; process CPU ms/step median {np.median(cpu[name]):.4f} {[round(v, 4) for v in cpu[name]]}")
    for ctxs, _ in routes.values():
        for c in ctxs:
            c.close()
    return wall, cpu


def publish(text):
    """profiles/group_device.txt + its section of profiles/README.md"""
    with open(os.path.join(ROOT, "profiles", "group_device.txt"), "w") as f:
        f.write(text)
    with open(os.path.join(ROOT, "profiles", "README.md"), "a") as f:
        f.write("\n## group_device.txt (tools/gpu_group.py)\n\n```\n" + text + "```\n")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--publish":  # a result file written elsewhere (another machine) into profiles/
        publish(open(sys.argv[2]).read())
        return
    out = sys.argv[1] if len(sys.argv) > 1 else None
    say("device grouping (ht_group.hip): k_grp_* device time, and the C2 loop on the device route against the host route")
    say(f"GPU: {torch.cuda.get_device_name(0)}; blocks of {BLOCK_STEPS} steps, {BLOCKS} per route, alternated")
    g2 = kernel_times(320, 240, 256)
    g4 = kernel_times(1280, 720, 128)
    wall, cpu = c2_loop()
    worst = max(max(g2.values()), max(g4.values()))
    say(f"expectation (each of the two grouping scopes <= 10 us of device time; the longest measured: {worst:.1f} us): {'holds' if worst <= 10 else 'REFUTED'}")
    hw, dw = float(np.median(wall["host"])), float(np.median(wall["device"]))
    spread = max(max(v) - min(v) for v in wall.values())
    say(f"expectation (device-route step no slower than the host route beyond the spread between blocks of one route, {spread:.4f} ms): "
        f"{'holds' if dw <= hw + spread else 'REFUTED'} (device {dw:.4f} ms, host {hw:.4f} ms per step)")
    hc, dc = float(np.median(cpu["host"])), float(np.median(cpu["device"]))
    say(f"expectation (host CPU time per batch falls): {'holds' if dc < hc else 'REFUTED'} (device route {dc:.4f} ms, host route {hc:.4f} ms of process CPU time per step)")
    text = "\n".join(lines) + "\n"
    if out is None:
        publish(text)
    else:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
