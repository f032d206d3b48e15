"""Run by tests/test_gpu_patch_tensor.py::test_into_a_torch_tensor in a process of its own: torch is imported FIRST (it brings a HIP runtime
of its own and cannot initialise behind another), then the library.  The pairs scene is tracked as the other tests track it (precondition:
the oracle's objects); empty_patches(n, 24, 24, fmt, "cuda") for f16 CHW and bf16 HWC is filled through the crop and the align wrapper;
after synchronize() the tensor's bits must be the restatement's.  A wrong-dtype, non-contiguous or short tensor is refused and nothing is
written.  Prints "OK 4 tensors" at the end; any failure is an exception."""
import os
import sys

import torch  # noqa: I001  (first: see above)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import align_cases as al  # noqa: E402
import crop_cases as cr  # noqa: E402
import patch_tensor_cases as pt  # noqa: E402
from headtrackr_amd import torch_patches as tp  # noqa: E402
from headtrackr_amd.api import Context, PatchFormat  # noqa: E402
from test_gpu_align import objects_agree  # noqa: E402
from test_gpu_crop import CROP_LIST, canvas_source, oracle_step, start_pairs  # noqa: E402

W, H = cr.CANVAS
n, P, Q = len(CROP_LIST), 24, 24
a, b = cr.pairs_scene()
c = Context()
c.set_geometry(W, H, 2)
c.upload(np.stack([a.frames[0], b.frames[0]]))
pairs = start_pairs(c)
c.upload(np.stack([a.frames[1], b.frames[1]]))
got = c.camshift_track_pairs(pairs)
objs = oracle_step(1)
objects_agree(got, [objs[s] for s, _f in pairs], "pairs scene, step 1")
sources = [canvas_source(a.frames[1]), canvas_source(b.frames[1])]
done = 0
for kind, into in (("crop", tp.crop_pairs_into), ("align", tp.align_pairs_into)):
    if kind == "crop":
        obj = [cr.obj_of(objs[s]) if s in objs else (0.0, 0.0, 0.0, 0.0) for s, _f in CROP_LIST]
        patches = [cr.patch(sources[f], o, W, H, None, 256, 0, P, Q) for o, (_s, f) in zip(obj, CROP_LIST)]
    else:
        obj = [al.obj_of(objs[s]) if s in objs else al.NO_OBJECT for s, _f in CROP_LIST]
        patches = [al.patch(sources[f], o, W, H, None, 256, 0, P, Q) for o, (_s, f) in zip(obj, CROP_LIST)]
    assert any(p.any() for p in patches)
    for fmt in (("f16", "chw", "rgb"), ("bf16", "hwc", "rgb")):
        pair = pt.PAIRS["imagenet"]
        pf = PatchFormat(*fmt, scale=pair[0], bias=pair[1])
        t = tp.empty_patches(n, P, Q, pf, "cuda")
        assert tuple(t.shape) == ((n, 3, Q, P) if fmt[1] == "chw" else (n, Q, P, 3)) and t.is_cuda and t.dtype == (torch.float16 if fmt[0] == "f16" else torch.bfloat16)
        t.view(torch.int16).fill_(0x5A5A)
        torch.cuda.synchronize()
        into(c, t, CROP_LIST, pf)
        c.synchronize()
        bits = t.cpu().view(torch.int16).numpy().reshape(n, -1)
        for i, p in enumerate(patches):
            want = pt.f(p, fmt, pair)
            assert np.array_equal(bits[i].view(np.uint8), want), f"{kind} {fmt} entry {i}: {(bits[i].view(np.uint8) != want).sum()} bytes differ"
        # refusals: nothing is written
        t.view(torch.int16).fill_(0x5A5A)
        wide = tp.empty_patches(n, 2 * P, Q, pf, "cuda")
        wide.view(torch.int16).fill_(0x5A5A)
        torch.cuda.synchronize()
        halves = wide[..., :P] if fmt[1] == "chw" else wide[:, :, :P, :]
        for bad, exc in ((t.float(), TypeError), (halves, ValueError), (t[:n - 1], ValueError)):
            try:
                into(c, bad, CROP_LIST, pf)
            except exc:
                pass
            else:
                raise AssertionError(f"{kind} {fmt}: a tensor of shape {tuple(bad.shape)}, {bad.dtype}, contiguous {bad.is_contiguous()} was accepted")
        c.synchronize()
        torch.cuda.synchronize()
        assert bool((t.view(torch.int16) == 0x5A5A).all()) and bool((wide.view(torch.int16) == 0x5A5A).all())
        done += 1
c.close()
print(f"OK {done} tensors")
