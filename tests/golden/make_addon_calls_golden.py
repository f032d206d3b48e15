#!/usr/bin/env python3
"""Records tests/golden/addon_calls.json: the transcript of tests/js/addon_calls.js on a given ht_napi.cc linked against the recording
C-ABI stub (tests/js/abi_stub.cc).  Needs g++, node and node_api.h; no GPU, no library.

    git show <commit>:headtrackr_amd/csrc/ht_napi.cc > /tmp/ht_napi_before.cc
    python tests/golden/make_addon_calls_golden.py /tmp/ht_napi_before.cc [out.json]

The committed file was recorded from the shim as it was BEFORE its argument handling was consolidated (the parent of the commit that added
this recorder) and is not re-recorded from a later shim: it is what holds a refactor of that file in place.  The overflow cases of the script
are not part of it (the recorded shim let them through); their outcomes on the given file are printed.  Test infrastructure only."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import addon_stub  # noqa: E402


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else addon_stub.GOLDEN
    with tempfile.TemporaryDirectory() as td:
        res = addon_stub.run(os.path.abspath(sys.argv[1]), td)
    addon_stub.dump(res["transcript"], out)
    print("wrote", out, os.path.getsize(out), "bytes,", len(res["transcript"]), "calls")
    for e in res["overflow"]:
        print("overflow case", "refused" if e["ok"] else "NOT refused", e["call"], "->", e.get("threw", "returned"), e.get("message", ""), e["log"])


if __name__ == "__main__":
    main()
