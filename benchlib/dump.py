"""bench.py --dump-outputs DIR: what the timed path returned to its caller in the last timed step, as DIR/<name>.npy.

Record arrays (best faces, camshift track objects) become float64 tables, one row per frame / stream and one column per
field in the dtype's order (the padding field `reserved` dropped); the inputs are seeded, so two builds given the same
arguments can be compared file by file."""
import os

import numpy as np

CAP_BYTES = 64 * 1024 * 1024


def table(rec):
    """structured array -> float64 [n, fields] (every field of the ABI's records is exact in binary64)"""
    rec = np.asarray(rec)
    if rec.dtype.names is None:
        return np.atleast_1d(rec.astype(np.float64))
    names = [n for n in rec.dtype.names if n != "reserved"]
    return np.stack([rec[n].astype(np.float64) for n in names], axis=-1).reshape(len(rec), len(names))


def write(directory, outputs):
    """outputs: {name: array} -> directory/<name>.npy (float64), at most CAP_BYTES in all"""
    arrays = {k: table(v) for k, v in outputs.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > CAP_BYTES:
        raise SystemExit(f"--dump-outputs: {total} B of outputs exceed the {CAP_BYTES} B cap")
    os.makedirs(directory, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(directory, f"{k}.npy"), a)
