#!/usr/bin/env python3
"""Regenerates tests/golden/detect_variants.json: the unmodified reference JS (needs /root/reference and node) at intervals other than 5 and
with cascades whose window is not 24x24 — ccv.detect_objects takes both as arguments (ccv.js:109).

    python tests/golden/make_detect_variants_golden.py

The cases are GOLDEN_CASES of tests/detect_variant_cases.py: frames from headtrackr_amd.synth, written as raw RGBA to a temp dir; the custom
cascades from that module's builder, handed to oracle/ref_harness.js as objects in the shape of headtrackr.cascade (`cascade` of a case).
Stored per case: the generator spec, interval, the cascade's name, the level count, every pyramid canvas in creation order as (w, h, CRC32),
the raw and the grouped rects and the input's CRC; once per file: the custom cascades in the reference's JSON shape.  No frame, no plane and
no reference text is stored.  Test infrastructure only; the other golden files are not touched."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detect_variant_cases as dv  # noqa: E402
from headtrackr_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "detect_variants.json")


def main():
    cascades = {c["cascade"]: dv.cascade_to_json(dv.golden_cascade(c["cascade"])) for c in dv.GOLDEN_CASES if c["cascade"]}
    with tempfile.TemporaryDirectory() as td:
        job = {"cases": []}
        for k, c in enumerate(dv.GOLDEN_CASES):
            fn = f"f{k}.raw"
            synth.make(c["gen"], c["w"], c["h"]).tofile(os.path.join(td, fn))
            j = dict(name=c["name"], kind="detect", w=c["w"], h=c["h"], gen=c["gen"], frame=fn, interval=c["interval"], ops=["gray", "pyramid", "raw", "grouped"])
            if c["cascade"]:
                j["cascade"] = cascades[c["cascade"]]
            job["cases"].append(j)
        jf, of = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        with open(jf, "w") as f:
            json.dump(job, f)
        subprocess.check_call(["node", os.path.join(ROOT, "oracle", "ref_harness.js"), jf, of])
        with open(of) as f:
            res = json.load(f)
    for r, c in zip(res["cases"], dv.GOLDEN_CASES):
        assert r["name"] == c["name"]
        r["interval"], r["cascade"] = c["interval"], c["cascade"]
        # ccv.js:117-147 creates n - 1 slot-0 canvases and 3 (n - 2 next) variants: n from the count
        nxt, m = c["interval"] + 1, len(r["pyramid"])
        n = (m + 1 + 6 * nxt) // 4
        assert (n - 1) + 3 * (n - 2 * nxt) == m and n > 2 * nxt, (c["name"], m)
        r["nlevels"] = n
        assert len(r["raw"]) > 0, c["name"]  # what the cases were chosen for: the reference finds something
    res["cascades"] = cascades
    with open(OUT, "w") as f:
        json.dump(res, f, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
