#!/usr/bin/env python3
"""Score statistics and covariance of SKAT units on the device (sgx_skat_2bit), N = 430 000.

    python tools/skat_speed.py [--n N] [--sizes 16,64,256] [--units U] [--reps R] [--out FILE]

U units of m variants each (m = 16 / 64 / 256; hard calls with 1 % missing, every 7th row alt-major) against a
synthetic binary null model with three covariates.  Per m: the wall time of a whole call -- upload of the packed rows,
Gram tiles and dense sums on the matrix cores, tiles back, S and Phi on the host -- its units a second, the FP64
matrix-core work of the call (2 * 256 * 4 flop per MFMA, tiles x dwords x 4 of them) and the rate that makes.
Writes profiles/skat_speed.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--units", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skat_speed.json"))
    a = ap.parse_args()
    import torch  # noqa: F401
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    from saigegds_amd.nullmod import init_nullmod
    N = a.n
    mod = synth.synth_null_model(N, "binary", 0.05, n_cov=3, seed=20260)
    sm = init_nullmod(mod, np.arange(N), 0.0, 0.0, 1.0, 0.05, float(mod.var_ratio[0]))
    rng = np.random.default_rng(1)
    base = 16                                       # distinct rows; the units repeat them in orders of their own
    af = 10 ** rng.uniform(-2.3, -0.4, base)
    af[::7] = 1 - af[::7]
    codes = (rng.random((base, N)) < af[:, None]).astype(np.uint8) + (rng.random((base, N)) < af[:, None]).astype(np.uint8)
    codes[rng.random((base, N)) < 0.01] = 3
    ok = codes != 3
    n, s = ok.sum(axis=1), np.where(ok, codes, 0).sum(axis=1)
    mean = s / n
    lut16 = np.where((s > n)[:, None], np.stack([2 + 0 * mean, 1 + 0 * mean, 0 * mean, 2 - mean], axis=1),
                     np.stack([0 * mean, 1 + 0 * mean, 2 + 0 * mean, mean], axis=1))
    packed16 = pack_dosage_2bit(codes)
    res = {"n_samp": N, "units": a.units, "reps": a.reps, "sizes": {}}
    ndw = (N + 15) // 16
    with Scanner(sm) as sc:
        for m in (int(x) for x in a.sizes.split(",")):
            rows = a.units * m
            packed = np.ascontiguousarray(packed16[np.arange(rows) % base])
            lut = lut16[np.arange(rows) % base]
            ptr = np.arange(0, rows + 1, m)
            idx = np.arange(rows, dtype=np.int32)
            ts = []
            for rep in range(a.reps + 1):           # the first round warms up (code object, workspace)
                t0 = time.perf_counter()
                score, cov = sc.skat_2bit(packed, ptr, idx, lut)
                ts.append(time.perf_counter() - t0)
            assert np.isfinite(score).all() and all(np.isfinite(c).all() for c in cov)
            nvt = (m + 15) // 16
            tiles = a.units * (nvt * (nvt + 1) // 2 + nvt * ((2 * sm.k + 1 + 15) // 16))
            flop = tiles * ndw * 4 * 2 * 256 * 4
            t = min(ts[1:])
            res["sizes"][str(m)] = {"call_s": t, "units_per_s": a.units / t, "tiles": tiles, "packed_bytes": int(packed.nbytes),
                                    "mfma_flop": flop, "mfma_tflops_of_the_call": flop / t / 1e12}
            print(m, res["sizes"][str(m)], flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
