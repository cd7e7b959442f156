#!/usr/bin/env python3
"""Speed of the explicit GRM (sgx_grm_sparse / sgx_grm_dense) on a synthetic device-resident matrix
(sgx_synth_2bit_dev), N = 32 768 samples x M = 65 536 markers by default:

  (a) sparse(0.125): wall time and the per-stage split of sgx_grm_sparse_stats (second call: the per-handle tables
      of the screen are built by the first and reported apart);
  (b) the same entries by the one-hot route, crossprod_many on columns of the identity, IN THE SAME RUN: the only
      way to K_ij before this kernel.  --onehot-cols columns (default 2048) are timed and scaled to N; the line
      says so ("onehot_scaled": true) unless all N were run;
  (c) the screen as a fraction of the int8 matrix-pipe bound (4 limb products: 8 N_pairs M int8 operations, against
      --int8-peak, the vendor's dense figure), and the FP64 tile kernel on a dense 8192 x 8192 block as a fraction of
      the rate tools/fp64_rate.hip measures on the same box (--fp64-ns: its ns per v_fma_f64 wave-instruction per
      SIMD; or --fp64-rate in flop/s; without either the fraction is left out).  The kernels are timed by events on
      the device, apart from the copy to the host.

    python tools/grm_dense_speed.py [--n-samp 32768] [--markers 65536] [--out profiles/grm_dense_speed.json]

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


def measure(n, m, seed, onehot_cols, dense_edge, int8_peak, fp64_rate):
    import torch
    from grm_batch_bench import _matrix
    from saigegds_amd._lib import GrmOperator
    if not torch.cuda.is_available():
        raise SystemExit("grm_dense_speed.py needs an MI355X")
    packed, bpv = _matrix(n, m, seed)
    op = GrmOperator(None, n, 0, dev_ptr=packed.data_ptr(), n_markers=m, bytes_per_marker=bpv)
    line = {"metric": "explicit GRM: sparse(0.125) against the one-hot route", "n_samples": n, "n_markers": m}

    # (a)
    t0 = time.perf_counter()
    i, j, x, st0 = op.sparse(0.125, return_stats=True)
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    i, j, x, st = op.sparse(0.125, return_stats=True)
    t_sparse = time.perf_counter() - t0
    line["sparse"] = {"seconds": round(t_sparse, 4), "first_call_seconds": round(first, 4),
                      "ms_prepare_first_call": round(st0["ms_prepare"], 3), "stats": st}

    # (b) the one-hot route on the first onehot_cols samples
    k = min(onehot_cols, n)
    B = np.zeros((k, n))
    B[np.arange(k), np.arange(k)] = 1.0
    op.crossprod_many(B[:2])
    t0 = time.perf_counter()
    cols = op.crossprod_many(B)
    t_cols = time.perf_counter() - t0
    line["onehot"] = {"columns_timed": k, "seconds_timed": round(t_cols, 4), "onehot_scaled": k < n,
                      "seconds_all_columns": round(t_cols * n / k, 3), "ms_per_column": round(1e3 * t_cols / k, 4)}
    line["onehot_over_sparse"] = round(t_cols * n / k / t_sparse, 2)
    # the two routes agree where they overlap (the operator's limbs against FP64: to rounding)
    blk = op.dense_block(0, k, 0, n)
    line["max_abs_diff_onehot_vs_dense"] = float(np.max(np.abs(blk - cols)))

    # (c)
    pairs = st["tiles_screened"] * 64 * 64
    ops = 8.0 * pairs * (((m + 511) // 512) * 512)
    line["screen"] = {"int8_ops": ops, "tops": round(ops / (st["ms_screen"] * 1e-3) / 1e12, 2),
                      "fraction_of_int8_peak": round(ops / (st["ms_screen"] * 1e-3) / int8_peak, 4),
                      "int8_peak_assumed": int8_peak}
    # an off-diagonal block where N allows it: every tile of it is needed and computed once, 2 e^2 M flop (on the
    # diagonal the mirrored tiles are not computed, and the count would be about half)
    e = min(dense_edge, n // 2) if n >= 2 * 256 else n
    j0 = e if 2 * e <= n else 0
    op.dense_block(0, 64, 0, 64)
    t0 = time.perf_counter()
    op.dense_block(0, e, j0, e)
    t_dense = time.perf_counter() - t0
    t_kern = op.dense_kernel_ms() * 1e-3
    flop = 2.0 * e * e * m if j0 else 2.0 * (e // 16) * (e // 16 + 1) / 2 * 256 * m
    line["dense_block"] = {"edge": e, "first_column": j0, "flop": flop, "seconds_with_copy_out": round(t_dense, 4),
                           "kernel_seconds": round(t_kern, 4), "kernel_tflops": round(flop / t_kern / 1e12, 3)}
    if fp64_rate:
        line["dense_block"]["fp64_rate_measured"] = fp64_rate
        line["dense_block"]["fraction_of_measured_fp64_rate"] = round(flop / t_kern / fp64_rate, 4)
    op.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-samp", type=int, default=32768)
    ap.add_argument("--markers", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=20260)
    ap.add_argument("--onehot-cols", type=int, default=2048)
    ap.add_argument("--dense-edge", type=int, default=8192)
    ap.add_argument("--int8-peak", type=float, default=5.0e15, help="int8 dense operations per second (vendor figure)")
    ap.add_argument("--fp64-rate", type=float, default=0.0, help="flop/s measured by tools/fp64_rate on this box")
    ap.add_argument("--fp64-ns", type=float, default=0.0,
                    help="instead: ns per v_fma_f64 wave-instruction per SIMD as tools/fp64_rate prints it (the best "
                         "of its lines); the rate is 64 lanes x 2 flop x SIMDs / that")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grm_dense_speed.json"))
    args = ap.parse_args()
    rate = args.fp64_rate
    if not rate and args.fp64_ns:
        import torch
        simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
        rate = 128.0 * simds / (args.fp64_ns * 1e-9)
    line = measure(args.n_samp, args.markers, args.seed, args.onehot_cols, args.dense_edge, args.int8_peak, rate)
    print(json.dumps(line), flush=True)
    if args.out != "/dev/null":
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
