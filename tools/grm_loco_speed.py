#!/usr/bin/env python3
"""Cost of one leave-one-chromosome-out IRLS step on the implicit-GRM operator: 22 x (1 + K) solves at K = 3,
every chromosome with its own weights, on a synthetic device-resident matrix of 430 000 x 100 000 markers in
22 groups sized like the human autosomes.

  * loco:   one sgx_grm_pcg_loco call per batch of 64 columns, each column leaving its chromosome out;
  * floor:  the same right-hand sides through sgx_grm_pcg_multi on the whole GRM, one weight vector (the cost of
            the same sweeps without per-column weights, masks or diagonals);
  * naive:  22 sgx_grm_pcg_multi calls of 1 + K columns on operators of the markers outside each chromosome,
            built one at a time (the build is timed apart).

    python tools/grm_loco_speed.py [--n-samp 430000] [--markers 100000] [--out profiles/grm_loco_speed.json]

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

# lengths of the human autosomes 1 .. 22 in Mb (GRCh38, rounded): the group sizes follow them
AUTOSOME_MB = (248, 242, 198, 190, 182, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47, 51)


def groups_like_autosomes(m):
    edges = np.floor(np.cumsum(AUTOSOME_MB) / float(np.sum(AUTOSOME_MB)) * m + 0.5).astype(np.int64)
    edges[-1] = m
    return np.searchsorted(edges, np.arange(m), side="right").astype(np.int32)


def measure(n=430_000, m=100_000, K=3, seed=20260):
    import torch
    from grm_batch_bench import _matrix
    from saigegds_amd._lib import GrmOperator
    if not torch.cuda.is_available():
        raise SystemExit("grm_loco_speed.py needs an MI355X")
    packed, bpv = _matrix(n, m, seed)
    group = groups_like_autosomes(m)
    ng, nb = len(AUTOSOME_MB), 1 + K
    rng = np.random.default_rng(1)
    mu = rng.uniform(0.02, 0.4, (ng, n))
    W, tau = mu * (1 - mu), np.array([1.0, 0.3])
    B = rng.standard_normal((ng * nb, n))
    w_idx, excl = np.repeat(np.arange(ng), nb), np.repeat(np.arange(ng), nb)
    line = {"metric": "one LOCO IRLS step on the implicit-GRM operator", "n_samples": n, "n_markers": m,
            "groups": ng, "rhs_per_group": nb, "tau": tau.tolist(), "tol": 1e-5}

    op = GrmOperator(None, n, 0, dev_ptr=packed.data_ptr(), n_markers=m, bytes_per_marker=bpv)
    t0 = time.perf_counter()
    op.set_groups(group, ng)
    line["set_groups_s"] = round(time.perf_counter() - t0, 3)
    op.pcg_many(W[0], tau, B[:2], 2, 1e-5)                      # (first-call allocations out of the timings)
    op.pcg_loco(W[:1], [0, 0], tau, B[:2], [0, 1], 2, 1e-5)
    t0 = time.perf_counter()
    X, it = op.pcg_loco(W, w_idx, tau, B, excl, 500, 1e-5)
    t_loco = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, it_floor = op.pcg_many(W[0], tau, B, 500, 1e-5)
    t_floor = time.perf_counter() - t0
    op.close()
    line["loco"] = {"seconds": round(t_loco, 3), "iterations": [int(it.min()), int(it.max())], "sum_iterations": int(it.sum())}
    line["floor_full_grm"] = {"seconds": round(t_floor, 3), "iterations": [int(it_floor.min()), int(it_floor.max())],
                              "sum_iterations": int(it_floor.sum())}

    # the naive route: an operator of the markers outside each chromosome, one at a time
    t_build = t_solve = 0.0
    worst, same_iters = 0.0, True
    for c in range(ng):
        keep = torch.from_numpy(np.flatnonzero(group != c)).to(packed.device)
        t0 = time.perf_counter()
        sub_rows = packed.index_select(0, keep)
        torch.cuda.synchronize()
        sub = GrmOperator(None, n, 0, dev_ptr=sub_rows.data_ptr(), n_markers=int(keep.numel()), bytes_per_marker=bpv)
        t_build += time.perf_counter() - t0
        t0 = time.perf_counter()
        Xs, its = sub.pcg_many(W[c], tau, B[c * nb:(c + 1) * nb], 500, 1e-5)
        t_solve += time.perf_counter() - t0
        sub.close()
        del sub_rows
        same_iters &= bool(np.array_equal(its, it[c * nb:(c + 1) * nb]))
        worst = max(worst, float(np.max(np.abs(Xs - X[c * nb:(c + 1) * nb])) / np.max(np.abs(Xs))))
    line["naive_subset_operators"] = {"solve_seconds": round(t_solve, 3), "build_seconds": round(t_build, 3),
                                      "same_iterations_as_loco": same_iters, "max_rel_diff_to_loco": worst}
    line["loco_over_floor"] = round(t_loco / t_floor, 4)
    line["naive_solves_over_loco"] = round(t_solve / t_loco, 4)
    del packed
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-samp", type=int, default=430_000)
    ap.add_argument("--markers", type=int, default=100_000)
    ap.add_argument("--seed", type=int, default=20260)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grm_loco_speed.json"))
    args = ap.parse_args()
    line = measure(args.n_samp, args.markers, 3, args.seed)
    print(json.dumps(line), flush=True)
    if args.out != "/dev/null":
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
