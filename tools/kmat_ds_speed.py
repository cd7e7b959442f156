#!/usr/bin/env python
"""Speed of SKAT on an explicit GRM from dosage rows (sgx_ds_block_skat_kmat) against the 2-bit entry.

N samples (default 430 000), K a block-diagonal family matrix as tools/kmat_speed.py makes it, 4 units a call of
m = 16 / 64 / 256 variants.  Per m, in one run, on the SAME hard calls:

  2bit     Scanner.skat_kmat on the packed rows: ms per call split into columns, solves and products (sgx_skat_kmat_ms);
  uint8    DosageBlock.skat_kmat on the rows loaded into a uint8 block (4 x the bytes of a 2-bit row), the same split;
  float64  ... into a float64 block (32 x the bytes).

The number of interest is the column part ms[0] per entry of the dosage forms against the 2-bit entry's: the dosage
column kernel makes the K + 1 sums in one pass over the row, the 2-bit kernel walks the row K + 1 times.  The three
forms give the same bits (tests/test_gpu_kmat_ds.py); the tool records whether they did.  One JSON line on stdout, also
written to --out.  A record, not a gate.

    python tools/kmat_ds_speed.py [--n 430000] [--units 4] [--m 16,64,256] [--out profiles/kmat_ds_speed.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(call, split):
    call()                                  # warm-up: buffers grow here
    t = time.perf_counter()
    r = call()
    return r, (time.perf_counter() - t) * 1e3, [float(v) for v in split()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430000)
    ap.add_argument("--units", type=int, default=4)
    ap.add_argument("--m", default="16,64,256")
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--maxiter", type=int, default=500)
    ap.add_argument("--seed", type=int, default=20262)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmat_ds_speed.json"))
    a = ap.parse_args()
    import torch  # noqa: F401
    from kmat_speed import _Upper, family_upper
    from saigegds_amd import aggregate, synth
    from saigegds_amd._lib import ExplicitGrmOperator, Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    from saigegds_amd.nullmod import init_nullmod
    n = a.n
    rng = np.random.default_rng(a.seed)
    mod = synth.synth_null_model(n, "binary", 0.1, n_cov=3, seed=a.seed)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(np.nanmean(mod.var_ratio)))
    w, tau = np.ascontiguousarray(mod.V, dtype=np.float64), np.array([1.0, 0.5])
    i, j, x = family_upper(n, a.seed)
    res = {"n": n, "units": a.units, "covariates": int(sm.k), "tol": a.tol, "maxiter": a.maxiter, "tau": tau.tolist(),
           "grm_entries": int(2 * i.size - n), "cases": []}
    with Scanner(sm) as sc, ExplicitGrmOperator(_Upper(n, i, j, x)) as op:
        for m in [int(v) for v in a.m.split(",")]:
            nv = a.units * m
            af = 10 ** rng.uniform(-3, -1.3, nv)
            codes = np.empty((nv, n), dtype=np.uint8)
            for r0 in range(0, nv, 64):              # (64 rows at a time: the random numbers of all rows would not fit)
                p = af[r0:r0 + 64, None].astype(np.float32)
                sh = (p.shape[0], n)
                codes[r0:r0 + 64] = (rng.random(sh, dtype=np.float32) < p).astype(np.uint8) + (rng.random(sh, dtype=np.float32) < p)
            up = np.arange(a.units + 1, dtype=np.int64) * m
            vi = np.arange(nv, dtype=np.int32)
            flip, mean = aggregate.flip_mean(np.full(nv, float(n)), codes.sum(axis=1, dtype=np.float64))
            lut = aggregate.dosage_tables(flip, mean)
            packed = pack_dosage_2bit(codes)
            ref, ms2, split2 = timed(lambda: sc.skat_kmat(op, packed, up, vi, lut, w, tau, a.maxiter, a.tol), sc.skat_kmat_ms)
            case = {"m": m, "pcg_iters_max": int(ref[2].max()), "2bit_ms": ms2, "2bit_columns_ms": split2[0],
                    "2bit_solve_ms": split2[1], "2bit_products_ms": split2[2], "2bit_columns_ms_per_entry": split2[0] / nv}
            for name, dt in (("uint8", np.uint8), ("float64", np.float64)):
                with sc.dosage_block(dt, nv) as blk:
                    blk.load(codes.astype(dt))
                    got, ms, split = timed(lambda: blk.skat_kmat(op, up, vi, flip, mean, w, tau, a.maxiter, a.tol), sc.skat_kmat_ms)
                same = np.array_equal(got[0], ref[0]) and all(np.array_equal(p, q) for p, q in zip(got[1], ref[1]))
                case.update({f"{name}_ms": ms, f"{name}_columns_ms": split[0], f"{name}_solve_ms": split[1],
                             f"{name}_products_ms": split[2], f"{name}_columns_ms_per_entry": split[0] / nv,
                             f"{name}_columns_over_2bit": split[0] / split2[0], f"{name}_same_bits_as_2bit": bool(same)})
            res["cases"].append(case)
            print(f"m={m}: columns 2bit {split2[0]:.1f} ms, uint8 {case['uint8_columns_ms']:.1f} ms, float64 "
                  f"{case['float64_columns_ms']:.1f} ms", file=sys.stderr, flush=True)
    res["note"] = "one run each, wall time on the host around the synchronous calls; no spread taken"
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
