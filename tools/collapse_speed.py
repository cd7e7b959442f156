#!/usr/bin/env python3
"""Speed record of the collapse kernel (sgx_collapse_2bit_dev), N = 430 000.

    timeout -k 10 900 python tools/collapse_speed.py [--n N] [--rows M] [--out FILE]

Synthetic resident 2-bit rows (the benchmark's generator): `rows` (4096: 440 MB at the device stride, more than the
256 MiB the last-level cache holds) rows, row j with an expected minor-allele count of 1 + j mod 10, no missing
genotypes, no flip.  Every row is in exactly one group; groups of 8, 64 and 512 consecutive rows.  Per group size, the
median of 5 calls after a warm-up call, host wall time around the call + sgx_sync (the call copies the groups back and
checks them before it launches: that is in the time):
  us per group; (entries + groups) * ceil(N / 4) bytes -- one read of every entry's row, one write of every group's --
  per second, and that as a fraction of the 8 TB/s peak;
  the time of tests/collapse_ref.py (numpy) on ONE group of that size, the same rows, on the same machine.
Writes profiles/collapse_speed.json."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collapse_speed.json"))
    a = ap.parse_args()
    import torch
    from collapse_ref import collapse_ref
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.nullmod import init_nullmod
    n, m = a.n, a.rows
    dev = torch.device("cuda", 0)
    mod = synth.synth_null_model(n, "binary", 0.01, n_cov=3, seed=1)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(mod.var_ratio[0]))
    p = (1 + np.arange(m) % 10) / (2.0 * n)
    thr = np.empty((m, 3), dtype=np.uint32)
    thr[:, 0] = np.floor((1 - p) ** 2 * 4294967296.0).astype(np.uint32)
    thr[:, 1] = np.floor((1 - p * p) * 4294967296.0).astype(np.uint32)
    thr[:, 2] = 0
    row_bytes = (n + 3) // 4
    res = {"n_samp": n, "rows": m, "row_bytes": row_bytes, "peak_bytes_per_s": PEAK, "groups_of": {}}
    with Scanner(sm) as sc:
        bpv = sc.row_stride()
        rows = torch.empty((m, bpv), dtype=torch.uint8, device=dev)
        thr_d = torch.from_numpy(thr.view(np.int32)).to(dev)
        var_idx = torch.arange(m, dtype=torch.int32, device=dev)
        flip = torch.zeros(m, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        sc.synth_2bit_dev(rows.data_ptr(), bpv, m, 0, 1, thr_d.data_ptr())
        sc.sync()
        res["device_stride"] = bpv
        for size in (8, 64, 512):
            ng = m // size
            grp_ptr = torch.arange(0, ng * size + 1, size, dtype=torch.int64, device=dev)
            out = torch.empty((ng, bpv), dtype=torch.uint8, device=dev)
            cnt = torch.empty((ng, 2), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            times = []
            for _ in range(6):
                t = time.perf_counter()
                sc.collapse_2bit_dev(rows.data_ptr(), bpv, m, ng, grp_ptr.data_ptr(), var_idx.data_ptr(), flip.data_ptr(),
                                     out.data_ptr(), cnt.data_ptr())
                sc.sync()
                times.append(time.perf_counter() - t)
            times = times[1:]
            host = rows[:size, :row_bytes].cpu().numpy()
            t = time.perf_counter()
            ref_rows, ref_cnt = collapse_ref(host, n, [0, size], np.arange(size), np.zeros(size, dtype=np.uint8))
            t_ref = time.perf_counter() - t
            same = bool(np.array_equal(out[0, :row_bytes].cpu().numpy(), ref_rows[0]) and np.array_equal(cnt[0].cpu().numpy(), ref_cnt[0]))
            med, moved = statistics.median(times), (ng * size + ng) * row_bytes
            res["groups_of"][str(size)] = {
                "groups": ng, "entries": ng * size, "ms": [x * 1e3 for x in times], "median_ms": med * 1e3,
                "us_per_group": med * 1e6 / ng, "bytes": moved, "bytes_per_s": moved / med, "fraction_of_peak": moved / med / PEAK,
                "numpy_ref_us_per_group": t_ref * 1e6, "first_group_equals_ref": same,
                "first_group_counts": cnt[0].cpu().numpy().tolist()}
    res["note"] = ("one run on one MI355X; host wall time around the call + sgx_sync, median of 5 after a warm-up; bytes = "
                   "(entries + groups) * ceil(N / 4); the numpy reference is timed once on one group of each size")
    print(json.dumps(res))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
