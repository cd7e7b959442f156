#!/usr/bin/env python
"""Speed of SKAT on an explicit GRM (sgx_skat_kmat_2bit) against the route available before it.

N samples (default 430 000), K a block-diagonal family matrix as tools/kmat_speed.py makes it, 4 units a call of
m = 16 / 64 / 256 variants.  Per m, in one run:

  device   Scanner.skat_kmat: ms per call split into columns, solves and products (sgx_skat_kmat_ms), PCG steps;
  host     the same quantities without the new entry points: adj in numpy from the decoded rows, the solves by
           ExplicitGrmOperator.pcg_many from host arrays (16 N m bytes over PCIe per unit), C, D, E in numpy;
  ratio    host ms / device ms, and the largest scaled difference of the two Phi^K.

One JSON line on stdout, also written to --out.

    python tools/skat_kmat_speed.py [--n 430000] [--units 4] [--m 16,64,256] [--out profiles/skat_kmat_speed.json]
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


def host_route(op, sm, codes, lut, unit_ptr, w, tau, maxiter, tol):
    """Phi^K per unit by the route of the parent commit -> ([Phi], ms: columns, solves, products; largest step count)."""
    ms, phis, it_max = [0.0, 0.0, 0.0], [], 0
    X = np.ascontiguousarray(sm.t_X.T)
    t = time.perf_counter()
    Z, _ = op.pcg_many(w, tau, X, maxiter, tol)
    ms[1] += (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    Ei = np.linalg.inv(0.5 * (X @ Z.T + Z @ X.T))
    ms[2] += (time.perf_counter() - t) * 1e3
    for u in range(len(unit_ptr) - 1):
        e0, e1 = int(unit_ptr[u]), int(unit_ptr[u + 1])
        t = time.perf_counter()
        G = np.take_along_axis(lut[e0:e1], codes[e0:e1].astype(np.int64), axis=1)
        A = np.ascontiguousarray(G - (G @ sm.t_XVX_inv_XV) @ sm.t_X.T)
        ms[0] += (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        Y, it = op.pcg_many(w, tau, A, maxiter, tol)
        ms[1] += (time.perf_counter() - t) * 1e3
        it_max = max(it_max, int(it.max()))
        t = time.perf_counter()
        C, D = A @ Y.T, A @ Z.T
        phis.append(0.5 * (C + C.T) - D @ Ei @ D.T)
        ms[2] += (time.perf_counter() - t) * 1e3
    return phis, ms, it_max


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430000)
    ap.add_argument("--units", type=int, default=4)
    ap.add_argument("--m", default="16,64,256")
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--maxiter", type=int, default=500)
    ap.add_argument("--seed", type=int, default=20262)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skat_kmat_speed.json"))
    a = ap.parse_args()
    import torch  # noqa: F401
    from kmat_speed import _Upper, family_upper
    from saigegds_amd import synth
    from saigegds_amd._lib import ExplicitGrmOperator, Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    from saigegds_amd.nullmod import init_nullmod
    n = a.n
    rng = np.random.default_rng(a.seed)
    mod = synth.synth_null_model(n, "binary", 0.1, n_cov=3, seed=a.seed)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(np.nanmean(mod.var_ratio)))
    w, tau = np.ascontiguousarray(mod.V, dtype=np.float64), np.array([1.0, 0.5])
    i, j, x = family_upper(n, a.seed)
    res = {"n": n, "units": a.units, "tol": a.tol, "maxiter": a.maxiter, "tau": tau.tolist(), "grm_entries": int(2 * i.size - n),
           "cases": []}
    with Scanner(sm) as sc, ExplicitGrmOperator(_Upper(n, i, j, x)) as op:
        for m in [int(v) for v in a.m.split(",")]:
            nv = a.units * m
            af = 10 ** rng.uniform(-3, -1.3, nv)
            codes = np.empty((nv, n), dtype=np.uint8)
            for r0 in range(0, nv, 64):              # (64 rows at a time: the random numbers of all rows would not fit)
                p = af[r0:r0 + 64, None].astype(np.float32)
                sh = (p.shape[0], n)
                codes[r0:r0 + 64] = (rng.random(sh, dtype=np.float32) < p).astype(np.uint8) + (rng.random(sh, dtype=np.float32) < p)
            packed = pack_dosage_2bit(codes)
            z = np.zeros(nv)
            lut = np.stack([z, z + 1, z + 2, codes.mean(axis=1)], axis=1)
            up = np.arange(a.units + 1, dtype=np.int64) * m
            vi = np.arange(nv, dtype=np.int32)
            sc.skat_kmat(op, packed, up, vi, lut, w, tau, a.maxiter, a.tol)              # warm-up: buffers grow here
            t = time.perf_counter()
            _, cov, it = sc.skat_kmat(op, packed, up, vi, lut, w, tau, a.maxiter, a.tol)
            dev_ms = (time.perf_counter() - t) * 1e3
            split = sc.skat_kmat_ms()
            t = time.perf_counter()
            phis, hms, hit = host_route(op, sm, codes, lut, up, w, tau, a.maxiter, a.tol)
            host_ms = (time.perf_counter() - t) * 1e3
            diff = 0.0
            for p, q in zip(cov, phis):
                sd = np.sqrt(np.diag(q))
                diff = max(diff, float((np.abs(p - q) / (sd[:, None] * sd[None, :])).max()))
            res["cases"].append({"m": m, "device_ms": dev_ms, "device_columns_ms": float(split[0]), "device_solve_ms": float(split[1]),
                                 "device_products_ms": float(split[2]), "pcg_iters_max": int(it.max()), "host_ms": host_ms,
                                 "host_columns_ms": hms[0], "host_solve_ms": hms[1], "host_products_ms": hms[2],
                                 "host_pcg_iters_max": hit, "host_over_device": host_ms / dev_ms, "phi_scaled_diff": diff})
            print(f"m={m}: device {dev_ms:.1f} ms, host route {host_ms:.1f} ms", file=sys.stderr, flush=True)
    res["note"] = "one run each, wall time on the host around the synchronous calls; no spread taken"
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
