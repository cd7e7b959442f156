#!/usr/bin/env python3
"""Speed record of the conditional scan's device step (sgx_cond_2bit_dev), N = 430 000, K = 3, C = 8.

    timeout -k 10 600 python tools/cond_speed.py [--n N] [--rows M] [--unit-rows U] [--out FILE]

Synthetic resident 2-bit rows (the benchmark's generator).  In one run:
  (a) resident rows -> score / var / cov for `rows` (50 000) rows: sgx_cond_2bit_dev + sgx_sync, best of 3 calls after
      a warm-up call;
  (b) what the library could do for the same numbers before this entry existed: sgx_skat_2bit on the units {j} + C
      for `unit-rows` (2 000) of those rows, one call after a small warm-up call, reported per row.  That entry takes
      rows in host memory only, so its time includes their upload.
The results of (a) and (b) are compared on the rows they share.  The matrix-pipe bound of (a) is 2 M N PB flops at the
VENDOR peak of 78.6 TFLOP/s (FP64 matrix), not at a measured rate.  Writes profiles/cond_speed.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP64_MATRIX = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--c", type=int, default=8)
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--unit-rows", type=int, default=2_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cond_speed.json"))
    a = ap.parse_args()
    import torch
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.cond import _tables
    from saigegds_amd.nullmod import init_nullmod
    n, m, c, u = a.n, a.rows, a.c, min(a.unit_rows, a.rows)
    dev = torch.device("cuda", 0)
    mod = synth.synth_null_model(n, "binary", 0.05, n_cov=a.k, seed=1)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(mod.var_ratio[0]))
    with Scanner(sm) as sc:
        bpv = sc.row_stride()
        rows = torch.empty((m + c, bpv), dtype=torch.uint8, device=dev)
        thr = torch.from_numpy(synth.variant_thresholds(0, m + c, 1, miss_rate=0.005).view(np.int32)).to(dev)
        torch.cuda.synchronize()
        sc.synth_2bit_dev(rows.data_ptr(), bpv, m + c, 0, 1, thr.data_ptr())
        sc.sync()
        out8 = torch.empty((m + c, 8), dtype=torch.float64, device=dev)
        valid = torch.zeros(m + c, dtype=torch.uint8, device=dev)
        sc.scan_2bit_dev(rows.data_ptr(), bpv, m + c, out8.data_ptr(), valid.data_ptr())
        sc.sync()
        lut = _tables(out8[:, 0], valid != 0)
        torch.cuda.synchronize()
        nb = (n + 3) // 4
        host = rows[:c + u, :nb].cpu().numpy()                       # the conditioning rows first, then the rows of (b)
        hlut = lut[:c + u].cpu().numpy()
        assert np.isfinite(hlut).all()
        mac = out8[:c, 1].cpu().numpy()
        assert (mac > 0).all(), "a monomorphic conditioning row"
        t = time.perf_counter()
        s_c, phi_cc = sc.cond_set(host[:c], hlut[:c])
        t_set = time.perf_counter() - t

        # (a)
        score, var = (torch.empty(m, dtype=torch.float64, device=dev) for _ in range(2))
        cov = torch.empty((m, c), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        times = []
        for _ in range(4):
            t = time.perf_counter()
            sc.cond_2bit_dev(rows[c:].data_ptr(), bpv, m, lut[c:].data_ptr(), score.data_ptr(), var.data_ptr(), cov.data_ptr())
            sc.sync()
            times.append(time.perf_counter() - t)
        new_s = min(times[1:])
        got = (score[:u].cpu().numpy(), var[:u].cpu().numpy(), cov[:u].cpu().numpy())

        # (b)
        def units(k):
            idx = np.concatenate([np.concatenate([[c + j], np.arange(c)]) for j in range(k)]).astype(np.int32)
            return np.arange(0, (k + 1) * (c + 1), c + 1), idx
        ptr, idx = units(min(u, 32))
        sc.skat_2bit(host, ptr, idx, hlut[idx])
        ptr, idx = units(u)
        t = time.perf_counter()
        s2, covs = sc.skat_2bit(host, ptr, idx, hlut[idx])
        unit_s = time.perf_counter() - t
    worst = 0.0
    for j in range(u):
        sd = np.sqrt(np.diag(covs[j]))
        worst = max(worst, float(np.max(np.abs(np.concatenate([[got[1][j]], got[2][j]]) - covs[j][0]) / (sd[0] * sd))))
    pb = 16 * ((2 * a.k + 1 + c + 15) // 16)
    bound_s = 2.0 * m * n * pb / PEAK_FP64_MATRIX
    res = {
        "n_samp": n, "k": a.k, "n_cond": c, "rows": m, "b_columns": pb,
        "cond_set_s": t_set,
        "cond_2bit_dev_ms": [x * 1e3 for x in times], "cond_2bit_dev_best_ms": new_s * 1e3,
        "cond_2bit_dev_us_per_row": new_s * 1e6 / m,
        "matrix_pipe_bound_ms": bound_s * 1e3,
        "matrix_pipe_bound_note": "2 M N PB flops at the vendor peak of 78.6 TFLOP/s (FP64 matrix), not a measured rate",
        "fraction_of_matrix_pipe_bound": bound_s / new_s,
        "unit_route_rows": u, "unit_route_s": unit_s, "unit_route_us_per_row": unit_s * 1e6 / u,
        "unit_route_note": "sgx_skat_2bit on units {j} + C; rows in host memory, so the time includes their upload",
        "speedup_per_row": (unit_s / u) / (new_s / m),
        "largest_difference_between_the_routes": worst,
        "difference_note": "|dPhi| / sqrt(Phi_jj Phi_ll) over var and cov of the shared rows",
    }
    print(json.dumps(res))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
