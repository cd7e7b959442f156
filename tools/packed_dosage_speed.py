#!/usr/bin/env python3
"""Packed-real dosage rows over the link as stored (sgx_scan_packed) against float64 rows (sgx_scan_f64), N = 430 000.

    python tools/packed_dosage_speed.py [--n N] [--rows M] [--reps R] [--stats kernel_stats.csv] [--out FILE]

Both calls read pinned host buffers (sgx_host_alloc) and scan the same dosages: M rows stored as dPackedReal16U and as
dPackedReal8U, and their decoded float64 form.  Per class: wall time per variant, bytes over the link, the ratio to
the float64 call of the same run, and that the two tables are equal bit for bit.  --stats: the kernel statistics of a
run of this tool under `rocprofv3 --kernel-trace --stats -- python tools/packed_dosage_speed.py ...`; the decoder's
time is then set beside bytes moved / 6.3 TB/s (the achievable HBM rate DESIGN.md uses).  Writes
profiles/packed_dosage_speed.json; what was not measured says "not measured"."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 6.3e12
CLASSES = {"dPackedReal16U": (np.dtype("<u2"), 0xFFFF, 1e-4), "dPackedReal8U": (np.dtype(np.uint8), 0xFF, 1 / 127)}


def decoder_times(path):
    """kernel name -> (calls, total ns) of unpack_real_rows<...> from a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if "unpack_real_rows" in name:
                out[name] = (int(row.get("Calls", 0)), float(row.get("TotalDurationNs", row.get("TotalDuration(ns)", 0))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--rows", type=int, default=624)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_dosage_speed.json"))
    a = ap.parse_args()
    import torch  # noqa: F401
    from saigegds_amd import synth
    from saigegds_amd._lib import PinnedBuffer, Scanner
    from saigegds_amd.nullmod import init_nullmod
    N, M = a.n, a.rows
    mod = synth.synth_null_model(N, "binary", 0.01, n_cov=3, seed=20260)
    sm = init_nullmod(mod, np.arange(N), float("nan"), 10.0, 0.1, 0.05, float(mod.var_ratio[0]))
    rng = np.random.default_rng(1)
    af = 10 ** rng.uniform(-2.0, -0.4, M)
    res = {"n_samp": N, "n_variants": M, "reps": a.reps, "hbm_bytes_per_s": HBM_BPS, "classes": {}}
    with Scanner(sm) as sc, PinnedBuffer((M, N), np.float64) as pf:
        for cls, (dt, miss, scale) in CLASSES.items():
            with PinnedBuffer((M, N), dt) as pr:
                raw = pr.array
                for j in range(M):                      # imputed-looking rows: hard calls blurred, 0.5 % missing
                    g = (rng.random(N, dtype=np.float32) < af[j]).astype(np.float32) + (rng.random(N, dtype=np.float32) < af[j])
                    g = np.clip(g + rng.normal(0, 0.05, N).astype(np.float32) * (g > 0), 0, 2)
                    raw[j] = np.rint(g / scale).astype(dt)
                    raw[j, rng.random(N, dtype=np.float32) < 0.005] = miss
                    pf.array[j] = raw[j].astype(np.float64) * scale + 0.0
                    pf.array[j, raw[j] == miss] = np.nan
                t_pk, t_f64 = [], []
                for rep in range(a.reps + 1):           # the first round warms up (code objects, buffers)
                    t0 = time.perf_counter()
                    o1, v1 = sc.scan_packed(raw, cls, scale, 0.0)
                    t1 = time.perf_counter()
                    o2, v2 = sc.scan_f64(pf.array)
                    t2 = time.perf_counter()
                    if rep:
                        t_pk.append(t1 - t0)
                        t_f64.append(t2 - t1)
                same = bool(np.array_equal(v1, v2) and np.array_equal(np.nan_to_num(o1, nan=-7.0), np.nan_to_num(o2, nan=-7.0)))
                pk, f64 = min(t_pk), min(t_f64)
                res["classes"][cls] = {
                    "raw_row_bytes": N * dt.itemsize, "f64_row_bytes": N * 8,
                    "link_bytes_packed": M * N * dt.itemsize, "link_bytes_f64": M * N * 8,
                    "wall_us_per_variant_packed": 1e6 * pk / M, "wall_us_per_variant_f64": 1e6 * f64 / M,
                    "link_gb_per_s_packed": M * N * dt.itemsize / pk / 1e9, "link_gb_per_s_f64": M * N * 8 / f64 / 1e9,
                    "speedup_over_f64": f64 / pk, "ratio_of_row_bytes": 8 / dt.itemsize,
                    "tables_equal_bit_for_bit": same, "n_valid": int(v1.sum()),
                    "decoder_hbm_bytes_per_call": M * N * (dt.itemsize + 8),
                    "decoder_floor_us_per_call": 1e6 * M * N * (dt.itemsize + 8) / HBM_BPS,
                    "decoder_kernel": "not measured",
                }
    if a.stats:
        for name, (calls, ns) in decoder_times(a.stats).items():
            for cls, (dt, _, _) in CLASSES.items():
                if ("unsigned short" if dt.itemsize == 2 else "unsigned char") in name:
                    c = res["classes"][cls]
                    per_call = ns / max(calls, 1) * 1e-3
                    # a call of M rows is cut into chunks; the tool's calls per class: reps + 1
                    c["decoder_kernel"] = {"name": name, "launches": calls, "total_us": ns * 1e-3, "us_per_launch": per_call,
                                           "us_per_scan_call": ns * 1e-3 / (a.reps + 1),
                                           "fraction_of_hbm_rate": c["decoder_floor_us_per_call"] / (ns * 1e-3 / (a.reps + 1))}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
