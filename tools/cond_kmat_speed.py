#!/usr/bin/env python
"""Speed of the conditional scan on an explicit GRM (sgx_cond_kmat_2bit) against the route available
before it: sgx_skat_kmat_2bit on the units {C, j}, one unit per scanned row, which solves the set's C columns again for
every row and forms (C + 1)^2 products where 2 C + 1 + K are needed.

N = 430 000, the block-diagonal families of tools/skat_kmat_speed.py, K = 3 covariates, C = 8, tol = 1e-5.  Both routes
run in the same process on the same rows: the new entry on `rows` (4 096) rows, the per-unit route on a sample of
`sample` (64) of them.  Reported: ms per row of either, the three stage times (sgx_skat_kmat_ms: rows and columns,
solves, products) and the ratio.  One run each, wall time on the host around the synchronous calls.  Only `distinct`
rows are generated and repeated to fill `rows`: a row's cost does not depend on the other rows.

    python tools/cond_kmat_speed.py [--n 430000] [--rows 4096] [--sample 64] [--out profiles/cond_kmat_speed.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430000)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=512)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--cond", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--maxiter", type=int, default=500)
    ap.add_argument("--seed", type=int, default=20263)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cond_kmat_speed.json"))
    a = ap.parse_args()
    import torch  # noqa: F401
    from kmat_speed import _Upper, family_upper
    from saigegds_amd import synth
    from saigegds_amd._lib import ExplicitGrmOperator, Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    from saigegds_amd.nullmod import init_nullmod
    n, C = a.n, a.cond
    rng = np.random.default_rng(a.seed)
    mod = synth.synth_null_model(n, "binary", 0.1, n_cov=3, seed=a.seed)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 0.05, float(np.nanmean(mod.var_ratio)))
    w, tau = np.ascontiguousarray(mod.V, dtype=np.float64), np.array([1.0, 0.5])
    i, j, x = family_upper(n, a.seed)
    nd = min(a.distinct, a.rows) + C
    af = 10 ** rng.uniform(-3, -1.3, nd)
    codes = np.empty((nd, n), dtype=np.uint8)
    for r0 in range(0, nd, 64):
        p = af[r0:r0 + 64, None].astype(np.float32)
        sh = (p.shape[0], n)
        codes[r0:r0 + 64] = (rng.random(sh, dtype=np.float32) < p).astype(np.uint8) + (rng.random(sh, dtype=np.float32) < p)
    packed_d = pack_dosage_2bit(codes)
    z = np.zeros(nd)
    lut_d = np.stack([z, z + 1, z + 2, codes.mean(axis=1)], axis=1)
    del codes
    pick = C + np.arange(a.rows) % (nd - C)
    packed, lut = np.ascontiguousarray(packed_d[pick]), np.ascontiguousarray(lut_d[pick])
    res = {"n": n, "covariates": 3, "n_cond": C, "rows": a.rows, "distinct_rows": nd - C, "unit_sample": a.sample, "tol": a.tol,
           "maxiter": a.maxiter, "tau": tau.tolist(), "grm_entries": int(2 * i.size - n)}
    with Scanner(sm) as sc, ExplicitGrmOperator(_Upper(n, i, j, x)) as op:
        t = time.perf_counter()
        sc.cond_kmat_set(op, packed_d[:C], lut_d[:C], w, tau, a.maxiter, a.tol)
        res["set_ms"] = (time.perf_counter() - t) * 1e3
        res["set_stage_ms"] = sc.skat_kmat_ms().tolist()
        sc.cond_kmat(op, packed[:128], lut[:128])                                        # warm-up: buffers grow here
        t = time.perf_counter()
        score, var, cov, it = sc.cond_kmat(op, packed, lut)
        new_ms = (time.perf_counter() - t) * 1e3
        res.update(cond_kmat_ms=new_ms, cond_kmat_ms_per_row=new_ms / a.rows, cond_kmat_stage_ms=sc.skat_kmat_ms().tolist(),
                   pcg_iters_max=int(it.max()))
        print(f"sgx_cond_kmat_2bit: {new_ms / a.rows:.3f} ms per row", file=sys.stderr, flush=True)
        # the per-unit route on the first `sample` rows: units (c_1 .. c_C, j) over the set's rows and the sample's
        m = min(a.sample, a.rows)
        rows_u = np.ascontiguousarray(np.concatenate([packed_d[:C], packed[:m]]))
        lut_u = np.concatenate([lut_d[:C], lut[:m]])
        vi = np.concatenate([np.concatenate([np.arange(C), [C + r]]) for r in range(m)]).astype(np.int32)
        up = np.arange(m + 1, dtype=np.int64) * (C + 1)
        sc.skat_kmat(op, rows_u, up[:3], vi[:2 * (C + 1)], lut_u[vi[:2 * (C + 1)]], w, tau, a.maxiter, a.tol)      # warm-up
        t = time.perf_counter()
        _, ucov, _ = sc.skat_kmat(op, rows_u, up, vi, lut_u[vi], w, tau, a.maxiter, a.tol)
        old_ms = (time.perf_counter() - t) * 1e3
        res.update(unit_route_ms=old_ms, unit_route_ms_per_row=old_ms / m, unit_route_stage_ms=sc.skat_kmat_ms().tolist(),
                   unit_route_over_cond_kmat=(old_ms / m) / (new_ms / a.rows),
                   same_bits=bool(all(u[C, C] == var[r] and np.array_equal(u[C, :C], cov[r]) for r, u in enumerate(ucov))))
        print(f"per-unit route: {old_ms / m:.3f} ms per row", file=sys.stderr, flush=True)
    res["note"] = "one run each, wall time on the host around the synchronous calls; no spread taken"
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
