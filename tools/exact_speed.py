#!/usr/bin/env python3
"""Speed record of the exact-p-value kernel (sgx_exact_2bit_dev), N = 430 000, cases : controls = 1 : 99.

    timeout -k 10 900 python tools/exact_speed.py [--n N] [--rows M] [--missing RATE] [--out FILE]

Synthetic resident 2-bit rows (the benchmark's generator): `rows` (50 000) rows, row j with an expected minor-allele
count of 1 + j mod 10 (allele frequency MAC / 2N), 0.1 % missing.  In one run, each the median of 5 calls after a
warm-up call, host wall time around the call + sgx_sync:
  (a) sgx_exact_2bit_dev at max_mac = 63: us per row, and row bytes / time as a fraction of the 8 TB/s peak -- the
      kernel's bound is one read of the rows;
  (b) the yardsticks on the same rows: sgx_scan_2bit_dev (the resident two-plane scan) and sgx_firth_2bit_dev.
Writes profiles/exact_speed.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12          # bytes / s of HBM, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--missing", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_speed.json"))
    a = ap.parse_args()
    import torch
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.cond import _tables
    from saigegds_amd.nullmod import init_nullmod
    n, m = a.n, a.rows
    dev = torch.device("cuda", 0)
    mod = synth.synth_null_model(n, "binary", 0.01, n_cov=a.k, seed=1)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(mod.var_ratio[0]))      # no MAC filter: a singleton is valid
    p = (1 + np.arange(m) % 10) / (2.0 * n)
    thr = np.empty((m, 3), dtype=np.uint32)
    thr[:, 0] = np.floor((1 - p) ** 2 * 4294967296.0).astype(np.uint32)
    thr[:, 1] = np.floor((1 - p * p) * 4294967296.0).astype(np.uint32)
    thr[:, 2] = np.uint32(int(a.missing * 4294967296.0))

    def timed(call, sc):
        times = []
        for _ in range(6):
            t = time.perf_counter()
            call()
            sc.sync()
            times.append(time.perf_counter() - t)
        return times[1:]

    with Scanner(sm) as sc:
        bpv = sc.row_stride()
        rows = torch.empty((m, bpv), dtype=torch.uint8, device=dev)
        out8 = torch.empty((m, 8), dtype=torch.float64, device=dev)
        valid = torch.zeros(m, dtype=torch.uint8, device=dev)
        out4 = torch.empty((m, 4), dtype=torch.float64, device=dev)
        thr_d = torch.from_numpy(thr.view(np.int32)).to(dev)
        torch.cuda.synchronize()
        sc.synth_2bit_dev(rows.data_ptr(), bpv, m, 0, 1, thr_d.data_ptr())
        sc.sync()
        t_scan = timed(lambda: sc.scan_2bit_dev(rows.data_ptr(), bpv, m, out8.data_ptr(), valid.data_ptr()), sc)
        lut = _tables(out8[:, 0], valid != 0)
        plain = torch.tensor([0.0, 1.0, 2.0, 0.0], dtype=torch.float64, device=dev).expand_as(lut)
        lut = torch.where((valid != 0)[:, None], lut, plain).contiguous()      # a row without a carrier is read like the others
        torch.cuda.synchronize()
        t_exact = timed(lambda: sc.exact_2bit_dev(rows.data_ptr(), bpv, m, lut.data_ptr(), out4.data_ptr(), 63), sc)
        o4 = out4.cpu().numpy()
        t_firth = timed(lambda: sc.firth_2bit_dev(rows.data_ptr(), bpv, m, lut.data_ptr(), out4.data_ptr()), sc)
    row_bytes = (n + 3) // 4
    done = o4[:, 3] == 1

    def record(times):
        med = statistics.median(times)
        return {"ms": [x * 1e3 for x in times], "median_ms": med * 1e3, "us_per_row": med * 1e6 / m,
                "row_bytes_per_s": m * row_bytes / med, "fraction_of_peak": m * row_bytes / med / PEAK}

    res = {"n_samp": n, "k": a.k, "cases": int(np.sum(sm.y)), "rows": m, "row_bytes": row_bytes, "device_stride": bpv,
           "missing_rate": a.missing, "peak_bytes_per_s": PEAK, "valid_rows": int((valid != 0).sum().item()),
           "exact_done": int(done.sum()), "mac_counts": np.bincount(o4[:, 2].astype(np.int64)).tolist(),
           "exact": record(t_exact), "scan_2bit": record(t_scan), "firth_2bit": record(t_firth),
           "note": ("one run on one MI355X; host wall time around the call + sgx_sync, median of 5 after a warm-up; "
                    "row_bytes = ceil(N / 4), the bytes of a row that hold samples (the device stride pads it to a "
                    "multiple of 128)")}
    print(json.dumps(res))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
