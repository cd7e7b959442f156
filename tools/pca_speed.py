#!/usr/bin/env python3
"""Speed record of the GRM's principal components (sgx_grm_pca), N = 430 000 x M = 100 000, L = 32.

    timeout -k 10 900 python tools/pca_speed.py [--n N] [--m M] [--block L] [--rounds R] [--out FILE]

Synthetic common markers generated on the device (bench_grm.py's: MAF 0.01 .. 0.5, no structure, so nothing converges
and every call runs its `rounds` rounds).  One call of one round warms the handle up (scratch allocation); then one call
of `rounds` rounds is timed by the solver's own clocks (sgx_grm_pca_stats): the milliseconds in the products K Q
(sgx_grm_crossprod_multi_dev, with the host waiting at both ends) and in everything else of the loop (the block
kernels ts_gram / ts_apply / ts_axpy_cols, their small copies, Cholesky and Jacobi on the host).  Per round, and the
split against the cost model of DESIGN.md 8o: 58 ms of products, under 1 ms of block kernels.
Writes profiles/pca_speed.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EST_PRODUCT_MS, EST_BLOCK_MS = 58.0, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--block", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_speed.json"))
    a = ap.parse_args()
    import torch
    from saigegds_amd import synth
    from saigegds_amd._lib import GrmOperator, Scanner
    from saigegds_amd.nullmod import init_nullmod
    if not torch.cuda.is_available():
        raise SystemExit("pca_speed.py needs an MI355X")
    n, m, L, seed = a.n, a.m, a.block, 20260
    dev = torch.device("cuda", 0)
    mod = synth.synth_null_model(min(n, 20000), "binary", 0.1, seed=seed)
    sm = init_nullmod(mod, np.arange(min(n, 20000)), float("nan"), 10, 0.1, 0.05, 0.94)
    gen = Scanner(sm, 0)
    gen.n = n                       # only the generator of this handle is used
    bpv = ((n + 255) // 256) * 64
    packed = torch.empty((m, bpv), dtype=torch.uint8, device=dev)
    thr = synth.variant_thresholds(0, m, seed, log10_maf=(-2.0, -0.3), flip_frac=0.0, miss_rate=1e-3)
    thr_d = torch.from_numpy(thr.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    gen.synth_2bit_dev(packed.data_ptr(), bpv, m, 0, seed, thr_d.data_ptr())
    gen.sync()
    op = GrmOperator(None, n, 0, dev_ptr=packed.data_ptr(), n_markers=m, bytes_per_marker=bpv)
    del packed
    torch.cuda.empty_cache()
    Q0 = np.random.default_rng(1).standard_normal((L, n))
    n_pc = max(1, L - 12)
    op.pca(n_pc, Q0, max_iter=1, tol=0.0)
    t0 = time.perf_counter()
    r = op.pca(n_pc, Q0, max_iter=a.rounds, tol=0.0)
    wall = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    rl = op.pca(n_pc, Q0, max_iter=1, tol=0.0, loadings=True)
    wall_load = (time.perf_counter() - t0) * 1e3
    op.close()
    it = r["iters"]
    prod, blk = r["ms_products"] / it, r["ms_block"] / it
    res = {"n_samp": n, "n_markers": m, "block": L, "n_pc": n_pc, "rounds": it,
           "ms_products_per_round": prod, "ms_block_per_round": blk, "ms_call": wall,
           "ms_call_one_round_with_loadings": wall_load, "ms_call_one_round": rl["ms_products"] + rl["ms_block"],
           "estimate_ms_products_per_round": EST_PRODUCT_MS, "estimate_ms_block_per_round": EST_BLOCK_MS,
           "products_over_estimate": prod / EST_PRODUCT_MS, "block_over_estimate": blk / EST_BLOCK_MS,
           "block_share_of_round": blk / (prod + blk),
           "eigval_head": [float(x) for x in r["eigval"][:3]], "resid_head": [float(x) for x in r["resid"][:3]],
           "note": ("one run on one MI355X; one warm-up call, then one call of `rounds` rounds timed by the host clock "
                    "inside sgx_grm_pca with the stream idle at both ends of every product; ms_block is the rest of the "
                    "loop: block kernels, their copies and host synchronisations, Cholesky and Jacobi on the host, and "
                    "the upload of Q0 and the download of the vectors once per call")}
    print(json.dumps(res))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
