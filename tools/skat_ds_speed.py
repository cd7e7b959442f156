#!/usr/bin/env python3
"""Score statistics and covariance of SKAT units from a resident dosage block (sgx_ds_block_skat), N = 430 000.

    python tools/skat_ds_speed.py [--n N] [--sizes 16,64,256] [--units U] [--reps R] [--out FILE]

The counterpart of tools/skat_speed.py: U units of m variants each (m = 16 / 64 / 256) for a uint8 and a float64 block
(hard calls with 1 % missing, every 7th row alt-major, 30 % of the float64 genotypes blurred) against a synthetic binary
null model with three covariates.  Timed per m and row type: one call from the RESIDENT block -- tables up, Gram tiles
and dense sums on the matrix cores, tiles back, S and Phi on the host; the upload of the rows is not in it.  Beside
it sgx_skat_2bit's time for the same shape, whose call uploads its packed rows; a dosage row has 4 x (uint8) and 32 x
(float64) the bytes per sample of a 2-bit row.  Stated per case: the bytes of the entries' rows, each read at least
once, and the bytes/s that makes of the call (a lower bound of the kernel's own rate: a row tile is read once per
column tile).  A record, not a gate.  Writes profiles/skat_ds_speed.json."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skat_ds_speed.json"))
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
    flip16 = s > n
    lut16 = np.where(flip16[:, None], np.stack([2 + 0 * mean, 1 + 0 * mean, 0 * mean, 2 - mean], axis=1),
                     np.stack([0 * mean, 1 + 0 * mean, 2 + 0 * mean, mean], axis=1))
    packed16 = pack_dosage_2bit(codes)
    u8_16 = np.where(ok, codes, 0xFF).astype(np.uint8)
    x = np.where(ok, codes.astype(np.float64), np.nan)
    f64_16 = np.clip(x + rng.normal(0, 0.08, x.shape) * (rng.random(x.shape) < 0.3), 0, 2)
    fs = np.nansum(f64_16, axis=1)
    means = {"u8": np.where(flip16, 2 - mean, mean), "f64": np.where(fs > n, 2 - fs / n, fs / n)}
    flips = {"u8": flip16.astype(np.uint8), "f64": (fs > n).astype(np.uint8)}
    res = {"n_samp": N, "units": a.units, "reps": a.reps, "sizes": {}}

    def best(f):
        ts = []
        for rep in range(a.reps + 1):               # the first round warms up (code object, workspace)
            t0 = time.perf_counter()
            score, cov = f()
            ts.append(time.perf_counter() - t0)
        assert np.isfinite(score).all() and all(np.isfinite(c).all() for c in cov)
        return min(ts[1:])
    with Scanner(sm) as sc:
        for m in (int(v) for v in a.sizes.split(",")):
            rows = a.units * m
            pick = np.arange(rows) % base
            ptr = np.arange(0, rows + 1, m)
            packed, lut = np.ascontiguousarray(packed16[pick]), lut16[pick]
            t2 = best(lambda: sc.skat_2bit(packed, ptr, np.arange(rows, dtype=np.int32), lut))
            r = {"skat_2bit_call_s": t2, "skat_2bit_packed_bytes": int(packed.nbytes)}
            # the block holds up to 256 rows (copies of the 16 at addresses of their own: 110 MB of uint8, 880 MB of
            # float64 rows, beyond what the caches hold); with more entries than that the units share the block's rows
            nres = min(rows, 256)
            idx = (np.arange(rows) % nres).astype(np.int32)
            for kind, mat in (("u8", u8_16), ("f64", f64_16)):
                with sc.dosage_block(mat.dtype, nres) as blk:
                    blk.load(mat[np.arange(nres) % base])
                    t = best(lambda: blk.skat(ptr, idx, flips[kind][pick], means[kind][pick]))
                row_bytes = rows * N * mat.dtype.itemsize          # of the rows the entries name, once per entry
                r[kind] = {"call_s": t, "units_per_s": a.units / t, "resident_rows": nres, "entry_row_bytes": int(row_bytes),
                           "entry_row_bytes_per_s": row_bytes / t, "bytes_per_sample_vs_2bit": 4 * mat.dtype.itemsize,
                           "time_vs_skat_2bit": t / t2}
            res["sizes"][str(m)] = r
            print(m, r, flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
