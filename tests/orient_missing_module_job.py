"""Run by tests/test_gpu_orient.py::test_without_the_module_only_the_oriented_calls_fail in a process of its own, with HEADTRACKR_HIP_LIB
naming a COPY of the library in a directory that holds no libheadtrackr_hip_orient.hsaco: a plain draw_list works and is right; an oriented
one is HT_ERR_STATE with the module's path — in the copy's directory — in ht_last_error, writes nothing and leaves the context usable.
Prints "OK missing module" at the end; any failure is an exception."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import draw_list_cases as dl  # noqa: E402
import orient_cases as oc  # noqa: E402
from headtrackr_amd import native  # noqa: E402
from headtrackr_amd.api import Context, HtError  # noqa: E402
from hipmem import DeviceArray  # noqa: E402
from test_gpu_ingest import d2h  # noqa: E402

HT_ERR_STATE = -6
lib_dir = os.path.dirname(os.environ["HEADTRACKR_HIP_LIB"])
assert native.LIB_PATH == os.environ["HEADTRACKR_HIP_LIB"] and not os.path.exists(os.path.join(lib_dir, "libheadtrackr_hip_orient.hsaco"))
dw, dh = 40, 30
src = oc.source(dl.RGBA, 23, 23, seed=5)
arr = DeviceArray(src.plane_buffers()[0])
dst = DeviceArray(np.full(dw * dh * 4, dl.GUARD, dtype=np.uint8))
c = Context()
c.set_geometry(dw, dh, 1)
try:
    c.draw_list([oc.entry(src, [arr.ptr], 1)], dst=dst.ptr)
    raise AssertionError("the oriented draw went through without its module")
except HtError as e:
    assert e.status == HT_ERR_STATE, (e.status, str(e))
    assert os.path.join(lib_dir, "libheadtrackr_hip_orient.hsaco") in str(e), str(e)
c.synchronize()
assert (d2h(dst.ptr, dst.nbytes) == dl.GUARD).all()
c.draw_list([src.entry([arr.ptr])], dst=dst.ptr)  # the plain list: as before
c.synchronize()
assert np.array_equal(d2h(dst.ptr, dst.nbytes).reshape(dh, dw, 4), src.expected(None, dw, dh))
c.close()
arr.free()
dst.free()
print("OK missing module")
