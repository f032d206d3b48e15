"""Every refusal of the frame calls and the detect-step calls as one ordered script.  replay() makes each call on real contexts and returns
{"canvas": [W, H], "cases": {"call/case": [status, ht_last_error text, ht_frames_bound() afterwards]}}; tests/golden/frame_call_refusals.json
is that table as the library answered it BEFORE these calls moved out of csrc/ht_context.hip (into ht_frames.hip and ht_detect_step.hip),
and tests/test_gpu_frame_layouts.py replays it on the built library and compares for equality.  A case named "a+b" holds two faults that
are adjacent in the call's check order; the answer is the earlier check's, which is what pins the order.  A call that answers with a bare
status leaves ht_last_error as the case before it left it: that text is part of the record, the script's order is fixed.

Contexts: `fresh` never gets a geometry; `c` has one (W x H, MAX_BATCH frames); `other` has the same and binds inside c's buffer.  The only
kernels that run are one 2-frame detect batch with HT_DETECT_WHITEBALANCE at the end (ht_detect_whitebalance needs a collected one)."""
import ctypes as C

import numpy as np

from headtrackr_amd import native, synth
from headtrackr_amd.api import Context
from headtrackr_amd.native import HIT_DTYPE, RECT_DTYPE
from hipmem import DeviceArray

W, H, MAX_BATCH = 320, 240, 2
FB = W * H * 4
WB = native.HT_DETECT_WHITEBALANCE


def replay():
    fresh, c, other = Context(), Context(), Context()
    L = c._lib
    host = np.ascontiguousarray(np.stack([synth.face_frame(W, H, [(100, 60, 96)]), synth.face_frame(W, H, [(40, 30, 120)])]))
    foreign = DeviceArray(np.zeros(64, dtype=np.uint8))  # device memory no context allocated
    hp, out = host.ctypes.data, {}
    dbl = np.zeros(8, dtype=np.float64)
    rects = np.zeros(MAX_BATCH, dtype=RECT_DTYPE)
    hits = np.zeros(1 << 10, dtype=HIT_DTYPE)
    counts = np.zeros(8, dtype=np.uint32)
    total = C.c_uint32(0)

    def rec(key, ctx, status):
        assert key not in out, key
        out[key] = [int(status), L.ht_last_error(ctx._h).decode(), int(L.ht_frames_bound(ctx._h))]

    try:
        c.set_geometry(W, H, MAX_BATCH)
        other.set_geometry(W, H, MAX_BATCH)
        buf, spare = C.c_void_p(), C.c_void_p()
        assert L.ht_device_alloc(c._h, 2 * FB, C.byref(buf)) == 0 and L.ht_device_alloc(c._h, FB, C.byref(spare)) == 0
        d = buf.value

        # ---- the two uploads: geometry, then pointer / count / stride in ONE check
        for f, call in (("ht_upload_frames", L.ht_upload_frames), ("ht_upload_frames_async", L.ht_upload_frames_async)):
            rec(f + "/no geometry", fresh, call(fresh._h, hp, 2, FB))
            rec(f + "/no geometry+NULL frames", fresh, call(fresh._h, None, 2, FB))
            rec(f + "/no geometry+n = 0", fresh, call(fresh._h, hp, 0, FB))
            rec(f + "/NULL frames", c, call(c._h, None, 2, FB))
            rec(f + "/n = 0", c, call(c._h, hp, 0, FB))
            rec(f + "/n < 0", c, call(c._h, hp, -1, FB))
            rec(f + "/n above the batch capacity", c, call(c._h, hp, MAX_BATCH + 1, FB))
            rec(f + "/stride smaller than a frame", c, call(c._h, hp, 2, FB - 1))
            rec(f + "/stride 0", c, call(c._h, hp, 1, 0))
            rec(f + "/NULL frames+stride", c, call(c._h, None, 2, FB - 4))
            rec(f + "/count+stride", c, call(c._h, hp, MAX_BATCH + 1, FB - 4))

        # ---- ht_swap_frames
        rec("ht_swap_frames/no geometry", fresh, L.ht_swap_frames(fresh._h))
        rec("ht_swap_frames/nothing pending", c, L.ht_swap_frames(c._h))

        # ---- ht_bind_frames_device: geometry, then pointer / count / stride / both alignments in ONE check
        f, call = "ht_bind_frames_device", L.ht_bind_frames_device
        rec(f + "/no geometry", fresh, call(fresh._h, d, 2, FB))
        rec(f + "/no geometry+NULL frames", fresh, call(fresh._h, None, 2, FB))
        rec(f + "/no geometry+misaligned pointer", fresh, call(fresh._h, d + 2, 2, FB))
        rec(f + "/NULL frames", c, call(c._h, None, 2, FB))
        rec(f + "/n = 0", c, call(c._h, d, 0, FB))
        rec(f + "/n < 0", c, call(c._h, d, -2, FB))
        rec(f + "/n above the batch capacity", c, call(c._h, d, MAX_BATCH + 1, FB))
        rec(f + "/stride smaller than a frame", c, call(c._h, d, 2, FB - 4))
        rec(f + "/stride not a multiple of 4", c, call(c._h, d, 1, FB + 2))
        rec(f + "/misaligned pointer", c, call(c._h, d + 1, 1, FB))
        rec(f + "/count+stride", c, call(c._h, d, 0, FB - 4))
        rec(f + "/stride+pointer", c, call(c._h, d + 2, 1, FB + 2))

        # ---- nothing bound, nothing enqueued (c has a geometry, fresh has none)
        for name, ctx in (("no geometry", fresh), ("nothing bound", c)):
            rec("ht_detect_enqueue/" + name, ctx, L.ht_detect_enqueue(ctx._h, 0))
            rec("ht_detect_enqueue/" + name + ", with whitebalance", ctx, L.ht_detect_enqueue(ctx._h, WB))
            rec("ht_whitebalance_batch/" + name, ctx, L.ht_whitebalance_batch(ctx._h, dbl.ctypes.data, 1))
            rec("ht_whitebalance_batch/" + name + "+NULL out", ctx, L.ht_whitebalance_batch(ctx._h, None, 1))
            rec("ht_detect_collect/" + name + ": nothing enqueued", ctx, L.ht_detect_collect(ctx._h, hits.ctypes.data, 16, counts.ctypes.data, C.byref(total)))
            rec("ht_detect_collect/" + name + ": nothing enqueued+NULL hits", ctx, L.ht_detect_collect(ctx._h, None, 0, None, None))
            rec("ht_detect_collect_best/" + name + ": nothing enqueued", ctx, L.ht_detect_collect_best(ctx._h, 1, rects.ctypes.data, C.byref(total)))
            rec("ht_detect_collect_best/" + name + ": NULL best+nothing enqueued", ctx, L.ht_detect_collect_best(ctx._h, 1, None, C.byref(total)))
            rec("ht_detect_collect_best_requeue/" + name + ": nothing enqueued", ctx, L.ht_detect_collect_best_requeue(ctx._h, 1, rects.ctypes.data, None, 0))
            rec("ht_detect_collect_best_requeue/" + name + ": NULL best+nothing enqueued", ctx, L.ht_detect_collect_best_requeue(ctx._h, 1, None, None, 0))
            rec("ht_detect_whitebalance/" + name + ": nothing collected", ctx, L.ht_detect_whitebalance(ctx._h, dbl.ctypes.data, 1))
            rec("ht_detect_whitebalance/" + name + ": nothing collected+n = 0", ctx, L.ht_detect_whitebalance(ctx._h, dbl.ctypes.data, 0))
            rec("ht_detect_whitebalance/" + name + ": NULL out+nothing collected", ctx, L.ht_detect_whitebalance(ctx._h, None, 1))

        # ---- the allocation calls
        p = C.c_void_p()
        rec("ht_device_alloc/0 bytes", c, L.ht_device_alloc(c._h, 0, C.byref(p)))
        rec("ht_device_alloc/NULL out", c, L.ht_device_alloc(c._h, 64, None))
        rec("ht_host_alloc/0 bytes", c, L.ht_host_alloc(0, C.byref(p)))
        rec("ht_host_alloc/NULL out", c, L.ht_host_alloc(64, None))
        rec("ht_device_upload/NULL destination", c, L.ht_device_upload(c._h, None, hp, 16))
        rec("ht_device_upload/NULL source", c, L.ht_device_upload(c._h, d, None, 16))
        rec("ht_device_upload/0 bytes", c, L.ht_device_upload(c._h, d, hp, 0))
        rec("ht_device_download/NULL destination", c, L.ht_device_download(c._h, None, d, 16))
        rec("ht_device_download/NULL source", c, L.ht_device_download(c._h, hp, None, 16))
        rec("ht_device_download/0 bytes", c, L.ht_device_download(c._h, hp, d, 0))

        # ---- ht_device_free: NULL is fine; the pointer has to be this context's; nobody ELSE may be bound inside it
        f, call = "ht_device_free", L.ht_device_free
        rec(f + "/NULL pointer", c, call(c._h, None))
        rec(f + "/a pointer no context allocated", c, call(c._h, foreign.ptr))
        rec(f + "/inside a buffer, not its start", c, call(c._h, d + FB))
        rec(f + "/another context's buffer", other, call(other._h, d))
        assert L.ht_bind_frames_device(other._h, d, 2, FB) == 0
        rec(f + "/another context bound at its first byte", c, call(c._h, d))
        rec(f + "/another context's buffer+that context bound inside it", other, call(other._h, d))
        assert L.ht_bind_frames_device(other._h, d + FB, 1, FB) == 0
        rec(f + "/another context bound at its last frame", c, call(c._h, d))
        assert L.ht_bind_frames_device(c._h, d, 2, FB) == 0
        rec(f + "/the owner and another context bound inside it", c, call(c._h, d))
        assert L.ht_bind_frames_device(other._h, spare.value, 1, FB) == 0
        rec(f + "/another context bound inside ANOTHER buffer of the owner", c, call(c._h, spare.value))
        rec(f + "/only the owner bound inside it: freed, the owner unbound", c, call(c._h, d))
        rec("ht_detect_enqueue/unbound by ht_device_free", c, L.ht_detect_enqueue(c._h, 0))
        rec("ht_whitebalance_batch/unbound by ht_device_free", c, L.ht_whitebalance_batch(c._h, dbl.ctypes.data, 1))
        rec(f + "/freed twice", c, call(c._h, d))

        # ---- bound frames: ht_whitebalance_batch's count; an upload pending, then a geometry that drops it
        assert L.ht_upload_frames(c._h, hp, 2, FB) == 0
        rec("ht_whitebalance_batch/n = 0", c, L.ht_whitebalance_batch(c._h, dbl.ctypes.data, 0))
        rec("ht_whitebalance_batch/n above the bound frames", c, L.ht_whitebalance_batch(c._h, dbl.ctypes.data, 3))
        rec("ht_whitebalance_batch/NULL out+n = 0", c, L.ht_whitebalance_batch(c._h, None, 0))
        assert L.ht_upload_frames(c._h, hp, 1, FB) == 0
        rec("ht_whitebalance_batch/n above the bound frames, below the capacity", c, L.ht_whitebalance_batch(c._h, dbl.ctypes.data, 2))

        # ---- one batch with and one without the whitebalance sums: what ht_detect_whitebalance refuses afterwards
        assert L.ht_upload_frames(c._h, hp, 2, FB) == 0
        assert L.ht_detect_enqueue(c._h, WB) == 0
        rec("ht_detect_whitebalance/enqueued with the flag, not collected yet", c, L.ht_detect_whitebalance(c._h, dbl.ctypes.data, 1))
        assert L.ht_detect_collect(c._h, hits.ctypes.data, 1 << 10, counts.ctypes.data, C.byref(total)) == 0 and total.value > 0
        rec("ht_detect_whitebalance/n = 0", c, L.ht_detect_whitebalance(c._h, dbl.ctypes.data, 0))
        rec("ht_detect_whitebalance/n above the collected batch", c, L.ht_detect_whitebalance(c._h, dbl.ctypes.data, 3))
        rec("ht_detect_whitebalance/NULL out+n above the collected batch", c, L.ht_detect_whitebalance(c._h, None, 3))
        rec("ht_detect_collect/collected already", c, L.ht_detect_collect(c._h, hits.ctypes.data, 1 << 10, counts.ctypes.data, C.byref(total)))
        rec("ht_detect_collect_best/collected already", c, L.ht_detect_collect_best(c._h, 1, rects.ctypes.data, C.byref(total)))
        rec("ht_detect_collect_best_requeue/collected already", c, L.ht_detect_collect_best_requeue(c._h, 1, rects.ctypes.data, None, 0))
        assert L.ht_detect_enqueue(c._h, 0) == 0
        assert L.ht_detect_collect(c._h, hits.ctypes.data, 1 << 10, counts.ctypes.data, C.byref(total)) == 0
        rec("ht_detect_whitebalance/the batch collected last had no flag", c, L.ht_detect_whitebalance(c._h, dbl.ctypes.data, 1))
        rec("ht_detect_whitebalance/no flag+n above the collected batch", c, L.ht_detect_whitebalance(c._h, dbl.ctypes.data, 3))

        # ---- ht_detect_batch: its parts' refusals, in their order (geometry, upload)
        f = "ht_detect_batch"

        def batch(ctx, ptr, n, w, h, stride):
            return L.ht_detect_batch(ctx._h, ptr, n, w, h, stride, 0, hits.ctypes.data, 1 << 10, counts.ctypes.data, C.byref(total))

        rec(f + "/zero width", fresh, batch(fresh, hp, 1, 0, H, FB))
        rec(f + "/zero width+NULL frames", fresh, batch(fresh, None, 1, 0, H, FB))
        rec(f + "/n = 0 on a context without geometry", fresh, batch(fresh, hp, 0, W, H, FB))
        rec(f + "/NULL frames", c, batch(c, None, 1, W, H, FB))
        rec(f + "/n = 0", c, batch(c, hp, 0, W, H, FB))
        rec(f + "/stride smaller than a frame", c, batch(c, hp, 1, W, H, FB - 4))
        rec("ht_swap_frames/nothing pending after all of it", c, L.ht_swap_frames(c._h))
        return {"canvas": [W, H], "cases": out}
    finally:
        other.close()
        fresh.close()
        c.close()
        foreign.free()
