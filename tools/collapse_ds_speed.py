#!/usr/bin/env python3
"""Speed record of collapsing on a resident dosage block (sgx_ds_block_collapse), N = 430 000.

    timeout -k 10 900 python tools/collapse_ds_speed.py [--n N] [--rows-u8 M] [--rows-f64 M] [--out FILE]

Resident rows with an expected minor-allele count of 1 + j mod 10 in row j, no missing values, no flip: uint8 rows of
hard calls (2048 rows, 0.88 GB) and float64 rows whose carriers hold fractional dosages (1024 rows, 3.5 GB) -- both
more than the 256 MiB the last-level cache holds.  Every row is in exactly one group; groups of 8, 64 and 512
consecutive rows.  Per block type and group size, the median of 5 calls after a warm-up call (every call appends its
pseudo-rows to the block, which is sized for all six):
  the whole entry: host wall time of ``DosageBlock.collapse`` -- tables up, the collapse kernel, ds_stats_kernel and the
    single-variant scan of the new rows, results back; bytes = entries * row_bytes read + the pseudo-rows written once
    and read again by the stats and by the scan (3 * groups * row_bytes);
  the collapse kernel alone: HIP events around it (sgx_stats.ms_kernel after the call); bytes = (entries + groups) *
    row_bytes;
  each as bytes per second and as a fraction of the 8 TB/s peak; ms a call and us per group.
In the same run: sgx_collapse_2bit_dev on the 2-bit form of the uint8 rows (host wall time around call + sync, bytes =
(entries + groups) * ceil(N / 4)), and tests/collapse_ds_ref.py (numpy) on ONE group of each size.
Writes profiles/collapse_ds_speed.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8e12          # bytes / s of HBM, MI355X
SIZES = (8, 64, 512)
CALLS = 6            # a warm-up and five timed


def make_rows(n, m, dtype, seed):
    """Row j: 1 + j mod 10 expected minor alleles -- that many carriers of dosage 1 (uint8) or of a dosage in (0.5, 2)."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((m, n), dtype=dtype)
    for j in range(m):
        who = rng.choice(n, 1 + j % 10, replace=False)
        rows[j, who] = 1 if dtype == np.uint8 else rng.uniform(0.5, 2.0, who.size)
    return rows


def time_block(sc, rows, res):
    from collapse_ds_ref import collapse_ds_ref
    m, n = rows.shape
    row_bytes = rows.dtype.itemsize * n
    out = {"rows": m, "row_bytes": row_bytes, "groups_of": {}}
    with sc.dosage_block(rows.dtype, m + CALLS * (m // SIZES[0]) + 1) as blk:
        for size in SIZES:
            ng = m // size
            grp_ptr = np.arange(0, ng * size + 1, size, dtype=np.int64)
            var_idx, flip = np.arange(ng * size, dtype=np.int32), np.zeros(ng * size, dtype=np.uint8)
            blk.load(rows)
            entry, kern = [], []
            for _ in range(CALLS):
                t = time.perf_counter()
                got = blk.collapse(grp_ptr, var_idx, flip, return_rows=False)
                entry.append(time.perf_counter() - t)
                kern.append(sc.stats()["ms_kernel"] * 1e-3)
            first = blk.collapse(grp_ptr[:2], var_idx[:size], flip[:size], return_rows=True)[5][0] if size == SIZES[0] else None
            entry, kern = entry[1:], kern[1:]
            t = time.perf_counter()
            ref = collapse_ds_ref(rows, [0, size], np.arange(size), np.zeros(size, dtype=np.uint8))[0]
            t_ref = time.perf_counter() - t
            me, mk = statistics.median(entry), statistics.median(kern)
            b_entry, b_kern = (ng * size + 3 * ng) * row_bytes, (ng * size + ng) * row_bytes
            out["groups_of"][str(size)] = {
                "groups": ng, "entries": ng * size,
                "entry_ms": [x * 1e3 for x in entry], "entry_median_ms": me * 1e3, "entry_us_per_group": me * 1e6 / ng,
                "entry_bytes": b_entry, "entry_bytes_per_s": b_entry / me, "entry_fraction_of_peak": b_entry / me / PEAK,
                "kernel_ms": [x * 1e3 for x in kern], "kernel_median_ms": mk * 1e3, "kernel_us_per_group": mk * 1e6 / ng,
                "kernel_bytes": b_kern, "kernel_bytes_per_s": b_kern / mk, "kernel_fraction_of_peak": b_kern / mk / PEAK,
                "numpy_ref_us_per_group": t_ref * 1e6, "first_group_sum": float(got[1][0]), "ref_first_group_sum": float(ref.sum()),
                "first_group_equals_ref": None if first is None else bool(first.tobytes() == ref.tobytes())}
    res[str(np.dtype(rows.dtype))] = out


def time_2bit(sc, rows_u8, res):
    import torch
    from saigegds_amd.gds import pack_dosage_2bit
    m, n = rows_u8.shape
    dev = torch.device("cuda", 0)
    bpv, row_bytes = sc.row_stride(), (n + 3) // 4
    d_rows = torch.zeros((m, bpv), dtype=torch.uint8, device=dev)
    for j0 in range(0, m, 256):                                 # packed on the host a slice at a time
        d_rows[j0:j0 + 256, :row_bytes] = torch.from_numpy(pack_dosage_2bit(rows_u8[j0:j0 + 256])).to(dev)
    var_idx = torch.arange(m, dtype=torch.int32, device=dev)
    flip = torch.zeros(m, dtype=torch.uint8, device=dev)
    out = {"rows": m, "row_bytes": row_bytes, "device_stride": bpv, "groups_of": {}}
    for size in SIZES:
        ng = m // size
        grp_ptr = torch.arange(0, ng * size + 1, size, dtype=torch.int64, device=dev)
        o_rows = torch.empty((ng, bpv), dtype=torch.uint8, device=dev)
        cnt = torch.empty((ng, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        times = []
        for _ in range(CALLS):
            t = time.perf_counter()
            sc.collapse_2bit_dev(d_rows.data_ptr(), bpv, m, ng, grp_ptr.data_ptr(), var_idx.data_ptr(), flip.data_ptr(),
                                 o_rows.data_ptr(), cnt.data_ptr())
            sc.sync()
            times.append(time.perf_counter() - t)
        times = times[1:]
        med, moved = statistics.median(times), (ng * size + ng) * row_bytes
        out["groups_of"][str(size)] = {"groups": ng, "entries": ng * size, "ms": [x * 1e3 for x in times], "median_ms": med * 1e3,
                                       "us_per_group": med * 1e6 / ng, "bytes": moved, "bytes_per_s": moved / med,
                                       "fraction_of_peak": moved / med / PEAK}
    res["collapse_2bit_dev_on_the_uint8_rows"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--rows-u8", type=int, default=2048)
    ap.add_argument("--rows-f64", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collapse_ds_speed.json"))
    a = ap.parse_args()
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.nullmod import init_nullmod
    n = a.n
    mod = synth.synth_null_model(n, "binary", 0.01, n_cov=3, seed=1)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(mod.var_ratio[0]))
    res = {"n_samp": n, "peak_bytes_per_s": PEAK}
    with Scanner(sm) as sc:
        rows = make_rows(n, a.rows_u8, np.uint8, 1)
        time_block(sc, rows, res)
        time_2bit(sc, rows, res)
        rows = make_rows(n, a.rows_f64, np.float64, 2)
        time_block(sc, rows, res)
    res["note"] = ("one run on one MI355X; median of 5 calls after a warm-up; entry: host wall time of DosageBlock.collapse, bytes = "
                   "(entries + 3 groups) * row_bytes; kernel: HIP events around collapse_ds_kernel, bytes = (entries + groups) * "
                   "row_bytes; the numpy reference is timed once on one group of each size")
    print(json.dumps(res))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
