#!/usr/bin/env python3
"""genotype/data rows over the link as stored (sgx_scan_dbit2) against the host decoder (sgx_decode_dbit2 + sgx_scan_2bit),
N = 430 000.

    timeout -k 10 300 python tools/dbit2_speed.py [--n N] [--n-file F] [--rows M] [--reps R] [--out FILE]
    python tools/dbit2_speed.py --merge FILE --stats kernel_stats.csv [--trace kernel_trace.csv] --reps R_OF_THE_TRACED_RUN [--out FILE]

Synthetic stored rows (hard calls, 0.5 % missing) in pinned buffers (sgx_host_alloc); in the same run, wall time of
  (a) host route, no subset:   sgx_decode_dbit2 (16 host threads, into a pinned buffer) + sgx_scan_2bit
  (b) host route, N of F samples selected (a sorted and a shuffled selection)
  (c), (d) sgx_scan_dbit2 on the same two inputs
with the tables compared bit for bit, `reps` repeats each (the first round warms up and is dropped), min / max given so
that the spread can be seen.  The link's rate of the same run: sgx_scan_2bit alone on the decoded rows.  --stats: the
kernel statistics of a second run of this tool, `timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv --
python tools/dbit2_speed.py --reps 1 --out /dev/null` (each device step under a time limit of its own, chained with
&&), merged into the first run's JSON with --merge; the decoder's time is then set beside bytes moved / 6.3 TB/s (the
achievable HBM rate DESIGN.md uses), and with --trace (that run's kernel_trace.csv) per launch, in the order of the
legs.  Writes profiles/dbit2_speed.json; what was not measured says "not measured"."""
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
LINK_BPS = 55e9           # the measured host-to-device rate of the pinned pipeline


def decoder_times(path):
    """(calls, total ns) of decode_dbit2_rows from a rocprofv3 kernel_stats.csv"""
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if "decode_dbit2_rows" in name:
                return name, int(row.get("Calls", 0)), float(row.get("TotalDurationNs", row.get("TotalDuration(ns)", 0)))
    return None


def stored_rows(out, n_file, rng):
    """hard calls as allele nibbles, two samples a byte (n_file even), MAF 1 % .. 40 %, 0.5 % missing"""
    nib = np.array([0b0000, 0b0001, 0b0101, 0b1111], dtype=np.uint8)
    base = min(out.shape[0], 96)                            # (distinct rows; the rest repeat them)
    for j in range(base, out.shape[0]):
        out[j] = 0
    for j in range(base):
        af = 10 ** rng.uniform(-2.0, -0.4)
        c = (rng.random(n_file, dtype=np.float32) < af).astype(np.uint8) + (rng.random(n_file, dtype=np.float32) < af)
        c[rng.random(n_file, dtype=np.float32) < 0.005] = 3
        x = nib[c]
        out[j] = x[0::2] | (x[1::2] << 4)
    for j in range(base, out.shape[0]):
        out[j] = out[j % base]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--n-file", type=int, default=487_000)
    ap.add_argument("--rows", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pipe-mb", type=int, default=32, help="chunk size of both routes' pipeline (2-bit rows per chunk)")
    ap.add_argument("--stats", default="")
    ap.add_argument("--merge", default="", help="a JSON this tool wrote: add --stats (of a traced run with --reps R) to it, no GPU work")
    ap.add_argument("--trace", default="", help="with --merge: the traced run's kernel_trace.csv, for the decoder's time per launch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbit2_speed.json"))
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as f:
            res = json.load(f)
        hit = decoder_times(a.stats)
        if hit:
            name, calls, ns = hit
            moved = sum(leg["decoder_hbm_bytes_per_call"] for leg in res["legs"].values()) * (a.reps + 1)
            res["decoder_kernel"] = {"name": name, "traced_run_reps": a.reps, "launches": calls, "total_us": ns * 1e-3,
                                     "us_per_launch": ns * 1e-3 / max(calls, 1), "bytes_moved": moved,
                                     "bytes_per_s": moved / (ns * 1e-9), "fraction_of_hbm_rate": moved / (ns * 1e-9) / HBM_BPS}
        if hit and a.trace:
            with open(a.trace, newline="") as f:
                rows = [r for r in csv.DictReader(f) if "decode_dbit2_rows" in r.get("Kernel_Name", "")]
            rows.sort(key=lambda r: int(r["Start_Timestamp"]))
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows]
            per_leg = len(us) // max(len(res["legs"]), 1)
            res["decoder_kernel"]["us_per_launch_by_leg"] = {
                leg: [round(x, 1) for x in us[k * per_leg:(k + 1) * per_leg]] for k, leg in enumerate(res["legs"])}
        print(json.dumps(res))
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        return
    import torch  # noqa: F401
    from saigegds_amd import synth
    from saigegds_amd._lib import PinnedBuffer, Scanner, decode_dbit2
    from saigegds_amd.nullmod import init_nullmod
    N, F, M = a.n, a.n_file, a.rows
    assert N % 2 == 0 and F % 2 == 0 and F >= N
    mod = synth.synth_null_model(N, "binary", 0.01, n_cov=3, seed=20260)
    sm = init_nullmod(mod, np.arange(N), float("nan"), 10.0, 0.1, 0.05, float(mod.var_ratio[0]))
    rng = np.random.default_rng(1)
    res = {"n_samp": N, "n_file_samp": F, "n_variants": M, "reps": a.reps, "pipe_mb": a.pipe_mb, "hbm_bytes_per_s": HBM_BPS,
           "link_bound_variants_per_s_at_55_GBps": LINK_BPS / (N / 2), "legs": {}}
    sorted_sel = np.sort(rng.permutation(F)[:N])
    inputs = {"no_subset": (N, None), "subset_sorted": (F, sorted_sel), "subset_shuffled": (F, rng.permutation(sorted_sel))}
    with Scanner(sm) as sc, PinnedBuffer((M, sc.row_stride())) as rows2:
        sc.set_option("pipe_mb", a.pipe_mb)                # several chunks per call: the copy of one under the work on another
        for leg, (nf, sel) in inputs.items():
            with PinnedBuffer((M, nf // 2)) as pr:
                stored_rows(pr.array, nf, rng)
                raw = pr.array.reshape(-1)
                t_host, t_dec, t_dev, t_link = [], [], [], []
                for rep in range(a.reps + 1):           # the first round warms up (code objects, buffers)
                    t0 = time.perf_counter()
                    decode_dbit2(raw, 0, nf, M, rows2.array, sel, 16)
                    t1 = time.perf_counter()
                    o1, v1 = sc.scan_2bit(rows2.array)
                    t2 = time.perf_counter()
                    o2, v2 = sc.scan_dbit2(raw, 0, nf, None, sel, M)
                    t3 = time.perf_counter()
                    if rep:
                        t_host.append(t2 - t0); t_dec.append(t1 - t0); t_link.append(t2 - t1); t_dev.append(t3 - t2)
                same = bool(np.array_equal(v1, v2) and np.array_equal(np.nan_to_num(o1, nan=-7.0), np.nan_to_num(o2, nan=-7.0)))
                res["legs"][leg] = {
                    "raw_row_bytes": nf // 2, "two_bit_row_bytes": sc.row_stride(),
                    "host_route_variants_per_s": [M / max(t_host), M / min(t_host)],
                    "host_decode_only_variants_per_s": [M / max(t_dec), M / min(t_dec)],
                    "host_decode_GB_per_s_of_file_bytes": M * (nf // 2) / min(t_dec) / 1e9,
                    "scan_2bit_only_variants_per_s": [M / max(t_link), M / min(t_link)],
                    "scan_2bit_link_GB_per_s": M * sc.row_stride() / min(t_link) / 1e9,
                    "device_route_variants_per_s": [M / max(t_dev), M / min(t_dev)],
                    "device_route_link_GB_per_s": M * (nf // 2) / min(t_dev) / 1e9,
                    "device_over_host": min(t_host) / min(t_dev),
                    "link_bound_variants_per_s": LINK_BPS / (nf // 2),
                    "tables_equal_bit_for_bit": same, "n_valid": int(v1.sum()),
                    "decoder_hbm_bytes_per_call": M * (nf // 2 + sc.row_stride()),
                }
        res["decoder_kernel"] = "not measured"
    if a.stats:
        hit = decoder_times(a.stats)
        if hit:
            name, calls, ns = hit
            moved = sum(leg["decoder_hbm_bytes_per_call"] for leg in res["legs"].values()) * (a.reps + 1)
            res["decoder_kernel"] = {"name": name, "launches": calls, "total_us": ns * 1e-3, "us_per_launch": ns * 1e-3 / max(calls, 1),
                                     "bytes_moved": moved, "bytes_per_s": moved / (ns * 1e-9),
                                     "fraction_of_hbm_rate": moved / (ns * 1e-9) / HBM_BPS}
    print(json.dumps(res))
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
