#!/usr/bin/env python3
"""Stored dosage rows -> 2-bit hard-call rows and filter counts on the device (sgx_quantize_packed), N = 430 000.

    python tools/ds_quant_speed.py [--n N] [--n-file F] [--rows M] [--reps R] [--chunk-mb C] [--host-rows H] [--out FILE]

The rows of a dosage-only file as the null-model fit's marker loader hands them over: M rows stored as dPackedReal8U,
dPackedReal16U and dFloat32, read from pinned host buffers (sgx_host_alloc) and written to pinned buffers, with the
file's N samples as they are and with a selection of N out of F = 487 000.  Per class and form: rows a second of the
whole call (upload, kernel, rows and counts back), the bytes over the link and their rate; beside them the rows a
second of the numpy statement of the same rule (gds.quantize_dosage_2bit, H rows) and the ratio, and that the two
agree (packed rows and integer counts exactly; ds_sum exactly for the integer classes).  Writes
profiles/ds_quant_speed.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLASSES = {"dPackedReal8U": (np.dtype(np.uint8), 0xFF, 1 / 127), "dPackedReal16U": (np.dtype("<u2"), 0xFFFF, 1e-4),
           "dFloat32": (np.dtype("<f4"), None, 1.0)}


def fill(raw, cls, rng):
    """Imputed-looking rows: hard calls, blurred where they are not 0, 0.5 % missing; 16 distinct rows, repeated."""
    dt, miss, scale = CLASSES[cls]
    base, n = min(16, raw.shape[0]), raw.shape[1]
    af = 10 ** rng.uniform(-2.0, -0.4, base)
    for j in range(base):
        g = (rng.random(n, dtype=np.float32) < af[j]).astype(np.float32) + (rng.random(n, dtype=np.float32) < af[j])
        g = np.clip(g + rng.normal(0, 0.05, n).astype(np.float32) * (g > 0), 0, 2)
        gone = rng.random(n, dtype=np.float32) < 0.005
        if miss is None:
            raw[j] = np.where(gone, np.float32(np.nan), g)
        else:
            raw[j] = np.where(gone, miss, np.rint(g / scale)).astype(dt)
    for j in range(base, raw.shape[0], base):
        raw[j:j + base] = raw[:min(base, raw.shape[0] - j)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--n-file", type=int, default=487_000)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--host-rows", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ds_quant_speed.json"))
    a = ap.parse_args()
    import torch  # noqa: F401
    from saigegds_amd import _lib
    from saigegds_amd.gds import quantize_dosage_2bit
    L = _lib.load()
    N, F, M, H = a.n, a.n_file, a.rows, min(a.host_rows, a.rows)
    nb = (N + 3) // 4
    rng = np.random.default_rng(1)
    sel = np.sort(rng.permutation(F)[:N]).astype(np.int32)          # the model's samples in the file's order
    res = {"n_samp": N, "n_file_samp": F, "n_rows": M, "reps": a.reps, "chunk_bytes": a.chunk_mb << 20,
           "host_rows": H, "classes": {}}
    with _lib.PinnedBuffer((M, nb), np.uint8) as ppk, _lib.PinnedBuffer((3, M), np.int32) as pcnt, \
            _lib.PinnedBuffer((M,), np.float64) as psum:
        for cls, (dt, miss, scale) in CLASSES.items():
            code = _lib.PACKED_CLASSES[cls]
            res["classes"][cls] = {}
            for form, nfs, s in (("all_samples", N, None), ("selection", F, sel)):
                with _lib.PinnedBuffer((M, nfs), dt) as pr:
                    raw = pr.array
                    fill(raw, cls, rng)
                    ts = []
                    for rep in range(a.reps + 1):               # the first round warms up (code objects)
                        t0 = time.perf_counter()
                        _lib.check(L.sgx_quantize_packed(raw.ctypes.data, code, nfs, scale, 0.0,
                                                         None if s is None else s.ctypes.data, N, M, 0, a.chunk_mb << 20,
                                                         ppk.array.ctypes.data, nb, pcnt.array[0].ctypes.data,
                                                         pcnt.array[1].ctypes.data, pcnt.array[2].ctypes.data,
                                                         psum.array.ctypes.data))
                        if rep:
                            ts.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    h = quantize_dosage_2bit(raw[:H], cls, scale, 0.0, sel=s)
                    t_host = time.perf_counter() - t0
                    same = bool(np.array_equal(h[0], ppk.array[:H]) and all(np.array_equal(h[1 + k], pcnt.array[k][:H]) for k in range(3)))
                    err = float(np.max(np.abs(h[4] - psum.array[:H]) / np.maximum(np.abs(h[4]), 1.0)))
                    t = min(ts)
                    link = M * nfs * dt.itemsize + M * nb
                    res["classes"][cls][form] = {
                        "raw_row_bytes": nfs * dt.itemsize, "packed_row_bytes": nb, "link_bytes": link,
                        "device_rows_per_s": M / t, "device_us_per_row": 1e6 * t / M, "link_gb_per_s": link / t / 1e9,
                        "upload_gb_per_s": M * nfs * dt.itemsize / t / 1e9,
                        "host_numpy_rows_per_s": H / t_host, "device_over_host": (M / t) / (H / t_host),
                        "rows_and_counts_equal_host": same, "ds_sum_max_rel_diff_from_host": err,
                    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
