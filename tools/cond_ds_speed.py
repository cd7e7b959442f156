#!/usr/bin/env python3
"""Speed record of the conditional scan on a resident dosage block (sgx_ds_block_cond), N = 430 000, K = 3, C = 8.

    timeout -k 10 600 python tools/cond_ds_speed.py [--n N] [--unit-rows U] [--out FILE]

The counterpart of tools/cond_speed.py for dosage rows.  Per row type (uint8, float64) a block of DS_BUDGET bytes of
resident rows (hard calls with 1 % missing, 30 % of the float64 genotypes blurred; 64 distinct rows, repeated -- the
kernel's work does not depend on the values); its first C rows are the conditioning set.  In one run:
  (a) resident rows -> score / var / cov on the host: one sgx_ds_block_cond call, best of 3 after a warm-up call;
  (b) the only way to these numbers without that entry: sgx_ds_block_skat on the units {j} + C for `unit-rows` of
      the same resident rows, one call after a small warm-up call, reported per row.
(a) and (b) are compared on the rows they share.  Bounds of (a), both at VENDOR peaks, not at measured rates: the row
bytes at 8 TB/s of HBM, and 2 M N PB flops at 78.6 TFLOP/s (FP64 matrix).  Beside it sgx_cond_2bit_dev's time per row
from profiles/cond_speed.json with the ratio of the input bytes (a 2-bit row holds 4 samples a byte).
Writes profiles/cond_ds_speed.json.  A record, not a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP64_MATRIX = 78.6e12
PEAK_HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--c", type=int, default=8)
    ap.add_argument("--unit-rows", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cond_ds_speed.json"))
    a = ap.parse_args()
    import torch  # noqa: F401
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.aggregate import DS_BUDGET
    from saigegds_amd.nullmod import init_nullmod
    n, c = a.n, a.c
    mod = synth.synth_null_model(n, "binary", 0.05, n_cov=a.k, seed=1)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(mod.var_ratio[0]))
    rng = np.random.default_rng(7)
    af = rng.uniform(0.05, 0.5, 64)
    codes = rng.binomial(2, af[:, None], (64, n)).astype(np.float64)
    codes[rng.random((64, n)) < 0.01] = np.nan
    pb = 16 * ((2 * a.k + 1 + c + 15) // 16)
    twobit = None
    p2 = os.path.join(ROOT, "profiles", "cond_speed.json")
    if os.path.exists(p2):
        with open(p2) as f:
            twobit = json.load(f).get("cond_2bit_dev_us_per_row")
    res = {"n_samp": n, "k": a.k, "n_cond": c, "b_columns": pb, "budget_bytes": DS_BUDGET,
           "bounds_note": "row bytes at the vendor peak of 8 TB/s (HBM) and 2 M N PB flops at the vendor peak of 78.6 TFLOP/s "
                          "(FP64 matrix); neither is a measured rate",
           "unit_route_note": "sgx_ds_block_skat on units {j} + C from the same resident rows",
           "difference_note": "|dPhi| / sqrt(Phi_jj Phi_ll) over var and cov of the shared rows",
           "cond_2bit_dev_us_per_row": twobit}
    with Scanner(sm) as sc:
        for kind, dt in (("u8", np.uint8), ("f64", np.float64)):
            row_bytes = n * np.dtype(dt).itemsize
            m = DS_BUDGET // row_bytes
            u = min(a.unit_rows, m - c)
            if kind == "u8":
                base = np.where(np.isnan(codes), 0xFF, codes).astype(np.uint8)
            else:
                base = np.clip(codes + rng.normal(0, 0.08, codes.shape) * (rng.random(codes.shape) < 0.3), 0, 2)
            rows = np.empty((m, n), dtype=dt)
            for o in range(0, m, 64):
                rows[o:o + 64] = base[:min(64, m - o)]
            with sc.dosage_block(dt, m) as blk:
                nv, s, _ = blk.load(rows)
                del rows
                nv = nv.astype(np.float64)
                fl = s > nv
                mean = np.where(fl, 2 - s / nv, s / nv)
                fl = fl.astype(np.uint8)
                t = time.perf_counter()
                blk.cond_set(np.arange(c), fl[:c], mean[:c])
                t_set = time.perf_counter() - t
                times = []
                for _ in range(4):
                    t = time.perf_counter()
                    score, var, cov = blk.cond(fl, mean)
                    times.append(time.perf_counter() - t)
                new_s = min(times[1:])

                def units(k):
                    idx = np.concatenate([np.concatenate([[c + j], np.arange(c)]) for j in range(k)]).astype(np.int32)
                    return np.arange(0, (k + 1) * (c + 1), c + 1), idx
                ptr, idx = units(min(u, 16))
                blk.skat(ptr, idx, fl[idx], mean[idx])
                ptr, idx = units(u)
                t = time.perf_counter()
                s2, covs = blk.skat(ptr, idx, fl[idx], mean[idx])
                unit_s = time.perf_counter() - t
            worst = 0.0
            for j in range(u):
                sd = np.sqrt(np.diag(covs[j]))
                got = np.concatenate([[var[c + j]], cov[c + j]])
                worst = max(worst, float(np.max(np.abs(got - covs[j][0]) / (sd[0] * sd))))
            us = new_s * 1e6 / m
            r = {"rows": int(m), "row_bytes": int(row_bytes), "cond_set_s": t_set,
                 "cond_ms": [x * 1e3 for x in times], "cond_best_ms": new_s * 1e3, "us_per_row": us,
                 "fraction_of_hbm_bound": (m * row_bytes / PEAK_HBM) / new_s,
                 "fraction_of_matrix_pipe_bound": (2.0 * m * n * pb / PEAK_FP64_MATRIX) / new_s,
                 "unit_route_rows": int(u), "unit_route_s": unit_s, "unit_route_us_per_row": unit_s * 1e6 / u,
                 "speedup_per_row_over_unit_route": (unit_s / u) / (new_s / m),
                 "largest_difference_between_the_routes": worst,
                 "input_bytes_over_2bit": row_bytes / ((n + 3) // 4)}
            if twobit:
                r["us_per_row_over_cond_2bit_dev"] = us / twobit
            res[kind] = r
    print(json.dumps(res))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
