#!/usr/bin/env python3
"""Speed of KING-robust kinship (sgx_grm_king_pairs) on a synthetic device-resident matrix (sgx_synth_2bit_dev),
N = 32 768 samples x M = 65 536 markers by default: one warm-up, then the median of --repeats king_pairs(2^-4.5)
calls -- the kernel by HIP events (sgx_grm_king_stats.ms_kernel) and the whole call -- as pair-markers per second and
int8 operations per second of the five products issued (2 x 5 x pairs x markers, the markers rounded up to the
128-marker step) against --int8-peak, the vendor's dense figure.  IN THE SAME RUN on the same handle: sparse(0.125),
whose screen (four products, table decode, the same tile shape) is the yardstick.

    python tools/king_speed.py [--n-samp 32768] [--markers 65536] [--out profiles/king_speed.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def measure(n, m, seed, repeats, cutoff, int8_peak):
    import torch
    from grm_batch_bench import _matrix
    from saigegds_amd._lib import GrmOperator
    if not torch.cuda.is_available():
        raise SystemExit("king_speed.py needs an MI355X")
    packed, bpv = _matrix(n, m, seed)
    op = GrmOperator(None, n, 0, dev_ptr=packed.data_ptr(), n_markers=m, bytes_per_marker=bpv)
    line = {"metric": "KING-robust pairs against the GRM screen, same handle, same run", "n_samples": n, "n_markers": m,
            "kin_cutoff": cutoff, "repeats": repeats}
    op.king_pairs(cutoff)
    kern, call, st = [], [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        st = op.king_pairs(cutoff, return_stats=True)[5]
        call.append(time.perf_counter() - t0)
        kern.append(st["ms_kernel"])
    ms = statistics.median(kern)
    pairs = st["tiles"] * 64 * 64
    steps_m = ((m + 127) // 128) * 128
    ops = 2.0 * 5 * pairs * steps_m
    line["king"] = {"ms_kernel_median": round(ms, 3), "ms_kernel_all": [round(v, 3) for v in kern],
                    "seconds_call_median": round(statistics.median(call), 4), "tiles": st["tiles"], "pairs_found": st["pairs"],
                    "products": 5, "pair_markers_per_second": pairs * m / (ms * 1e-3), "int8_ops": ops,
                    "tops": round(ops / (ms * 1e-3) / 1e12, 2),
                    "fraction_of_int8_peak": round(ops / (ms * 1e-3) / int8_peak, 4), "int8_peak_assumed_vendor": int8_peak}
    op.sparse(0.125)
    scr = []
    for _ in range(repeats):
        s = op.sparse(0.125, return_stats=True)[3]
        scr.append(s["ms_screen"])
    ms_s = statistics.median(scr)
    pairs_s = s["tiles_screened"] * 64 * 64
    ops_s = 2.0 * 4 * pairs_s * (((m + 511) // 512) * 512)
    line["screen"] = {"ms_screen_median": round(ms_s, 3), "ms_screen_all": [round(v, 3) for v in scr], "products": 4,
                      "int8_ops": ops_s, "tops": round(ops_s / (ms_s * 1e-3) / 1e12, 2),
                      "note": "ms_screen is host wall time around the screen launch and its counter read-back"}
    line["king_over_screen"] = round(ms / ms_s, 3)
    line["king_over_screen_per_product"] = round((ms / 5) / (ms_s / 4), 3)
    op.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-samp", type=int, default=32768)
    ap.add_argument("--markers", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=20260)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cutoff", type=float, default=2.0 ** -4.5)
    ap.add_argument("--int8-peak", type=float, default=5.0e15, help="int8 dense operations per second (vendor figure)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "king_speed.json"))
    args = ap.parse_args()
    line = measure(args.n_samp, args.markers, args.seed, args.repeats, args.cutoff, args.int8_peak)
    print(json.dumps(line), flush=True)
    if args.out != "/dev/null":
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
