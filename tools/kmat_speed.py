#!/usr/bin/env python3
"""Speed of the explicit-matrix operator (sgx_kmat, ExplicitGrmOperator) beside the implicit one, in one run:

  (a) CSR: a block-diagonal family matrix (families of 1..5) at N = 430 000;
  (b) dense: N = 32 768 (8 GiB), with the product as a fraction of the HBM peak for 8 N^2 bytes (--hbm-peak);
  (c) GrmOperator on a synthetic device-resident 430 000 x 100 000 genotype matrix.

For each: milliseconds per product (the kernels, by device events where the operator has them; else wall time of
crossprod_many with its copies) and per PCG iteration (wall time of a solve held to --iters iterations, divided
by them), at k = 1 and k = 16 right-hand sides.

    python tools/kmat_speed.py [--n-sparse 430000] [--n-dense 32768] [--markers 100000] [--out profiles/kmat_speed.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def family_upper(n, seed):
    """Upper triangle (i, j, x) of a block-diagonal matrix: consecutive families of 1..5, kinship 0.25 / 0.5 off
    the diagonal (one value per family), diagonal in [1, 1.1]."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 6, n)
    start = np.concatenate([[0], np.cumsum(sizes)])
    nf = int(np.searchsorted(start, n, side="left"))
    start, sizes = start[:nf], sizes[:nf].copy()
    sizes[-1] = n - start[-1]
    kin = rng.choice([0.25, 0.5], nf)
    i, j, x = [np.arange(n)], [np.arange(n)], [rng.uniform(1.0, 1.1, n)]
    for a in range(5):
        for b in range(a + 1, 5):
            f = np.flatnonzero(sizes > b)
            i.append(start[f] + a); j.append(start[f] + b); x.append(kin[f])
    i, j, x = np.concatenate(i), np.concatenate(j), np.concatenate(x)
    o = np.lexsort((j, i))
    return i[o].astype(np.int32), j[o].astype(np.int32), x[o]


class _Upper:
    def __init__(self, n, i, j, x):
        self.n, self.i, self.j, self.x = n, i, j, x


def time_operator(op, n, iters, rng, event_ms):
    out = {}
    w = rng.uniform(0.05, 0.25, n)
    for k in (1, 16):
        B = rng.standard_normal((k, n))
        op.crossprod_many(B)                            # warm-up (and buffers for k columns)
        t0 = time.perf_counter()
        op.crossprod_many(B)
        wall = 1e3 * (time.perf_counter() - t0)
        row = {"product_wall_ms": round(wall, 4)}
        if event_ms:
            row["product_kernel_ms"] = round(op.matvec_ms(), 4)
        op.pcg_many(w, [1.0, 0.5], B, 2, 1e-300)
        t0 = time.perf_counter()
        _, its = op.pcg_many(w, [1.0, 0.5], B, iters, 1e-300)
        row["pcg_iteration_ms"] = round(1e3 * (time.perf_counter() - t0) / max(int(its.max()), 1), 4)
        row["pcg_iterations_timed"] = int(its.max())
        out[f"k{k}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-sparse", type=int, default=430000)
    ap.add_argument("--n-dense", type=int, default=32768)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=20261)
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes per second (vendor figure)")
    ap.add_argument("--skip-implicit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmat_speed.json"))
    args = ap.parse_args()
    import torch
    from saigegds_amd._lib import ExplicitGrmOperator, GrmOperator
    if not torch.cuda.is_available():
        raise SystemExit("kmat_speed.py needs an MI355X")
    rng = np.random.default_rng(args.seed)
    line = {"metric": "explicit-matrix operator: ms per product and per PCG iteration", "iters": args.iters}

    n = args.n_sparse
    i, j, x = family_upper(n, args.seed)
    with ExplicitGrmOperator(_Upper(n, i, j, x)) as op:
        line["csr"] = {"n_samples": n, "nnz_full_pattern": int(2 * i.size - n), **time_operator(op, n, args.iters, rng, True)}

    n = args.n_dense
    u = rng.standard_normal(n)
    K = np.multiply.outer(u, u * (0.05 / n))
    K[np.arange(n), np.arange(n)] += 1.0
    with ExplicitGrmOperator(K) as op:
        d = {"n_samples": n, "bytes": 8 * n * n, **time_operator(op, n, args.iters, rng, True)}
    del K
    for k in ("k1", "k16"):
        d[k]["fraction_of_hbm_peak"] = round(8.0 * n * n / (d[k]["product_kernel_ms"] * 1e-3) / args.hbm_peak, 4)
    d["hbm_peak_assumed"] = args.hbm_peak
    line["dense"] = d

    if not args.skip_implicit:
        from grm_batch_bench import _matrix
        n, m = args.n_sparse, args.markers
        packed, bpv = _matrix(n, m, args.seed)
        with GrmOperator(None, n, 0, dev_ptr=packed.data_ptr(), n_markers=m, bytes_per_marker=bpv) as op:
            line["implicit"] = {"n_samples": n, "n_markers": m, **time_operator(op, n, args.iters, rng, False)}
    print(json.dumps(line), flush=True)
    if args.out != "/dev/null":
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
