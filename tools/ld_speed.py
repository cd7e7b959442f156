#!/usr/bin/env python3
"""Speed record of the LD kernel (sgx_ld_block_2bit), N = 430 000.

    timeout -k 10 900 python tools/ld_speed.py [--n N] [--out FILE]

Random 2-bit rows (allele frequency 0.05 to 0.5, 1 % missing; the kernel's work does not depend on the values).  A
block of 256 candidate rows against a window of 256 and of 1 024 kept rows: the window is filled by pushes, then
`LdEngine.block` is called 6 times and the first call dropped.  Per window size, the median of the 5:
  ms per block -- the kernels alone (HIP events: the two contractions and the decision) and the whole call (host wall
  time: upload of the block, kernels, download of the flags);
  pair-samples per second = pairs N / kernel time, where pairs counts what the kernel EXECUTES: 256 W against the
  window, and of the block's own square the 36 of 64 tiles of 32 x 32 that hold a pair with j < i (36 864 pairs, of
  which 32 640 are the wanted ones);
  the fraction of the bound of the form that ships, the MFMA form: six int8 products per executed pair-sample, 2
  operations each, against the int8 matrix peak (dense, ~5e15 operations / s: twice the BF16 peak);
  the time of tests/ld_ref.py (numpy: counts and decision in int64) for the first 16 rows of the block against the
  window of 256 and the block, measured once, and 16 times that as the estimate for the whole block (the full block
  takes numpy several minutes).
Writes profiles/ld_speed.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE = 32            # LD_TILE: rows of a wave's tile on either side (kern_ld.h)
PEAK_I8 = 5.0e15     # int8 operations / s of the matrix cores, MI355X, dense


def rows_of(rng, m, n):
    out = np.empty((m, (n + 3) // 4), dtype=np.uint8)
    for k in range(m):
        f = rng.uniform(0.05, 0.5)
        c = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=4 * out.shape[1],
                       p=[0.99 * (1 - f) ** 2, 0.99 * 2 * f * (1 - f), 0.99 * f * f, 0.01]).reshape(-1, 4)
        out[k] = c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ld_speed.json"))
    a = ap.parse_args()
    import ld_ref as R
    from saigegds_amd._lib import LD_BLOCK, LdEngine
    n, t2 = a.n, 0.04
    rng = np.random.default_rng(1)
    blk = rows_of(rng, LD_BLOCK, n)
    res = {"n_samp": n, "block": LD_BLOCK, "form": "mfma_i32_16x16x64_i8, six products", "peak_int8_ops_per_s": PEAK_I8,
           "windows": {}}
    with LdEngine(n, blk.shape[1]) as eng:
        for W in (256, 1024):
            eng.reset()
            win = []
            while eng.window_len < W:
                w = rows_of(rng, LD_BLOCK, n)
                eng.block(w, t2)
                eng.push(np.arange(LD_BLOCK), 0)
                win.append(w)
            wall, kern = [], []
            for _ in range(6):
                t = time.perf_counter()
                flags = eng.block(blk, t2)
                wall.append(time.perf_counter() - t)
                kern.append(eng.kernel_ms() * 1e-3)
            wall, kern = wall[1:], kern[1:]
            extra = {}
            if W == 256:
                cb, cw = R.unpack(blk, n), R.unpack(np.concatenate(win), n)
                t = time.perf_counter()
                ref = np.concatenate([R.in_ld(R.counts(cb[:16], cw), t2), R.in_ld(R.counts(cb[:16], cb), t2)], axis=1)
                t_ref = time.perf_counter() - t
                same = np.array_equal(flags[:16, :W], ref[:, :W]) and np.array_equal(np.tril(flags[:16, W:], -1), np.tril(ref[:, W:], -1))
                extra = {"numpy_ref_16_rows_ms": t_ref * 1e3, "numpy_ref_block_estimate_ms": 16 * t_ref * 1e3,
                         "flags_equal_ref_16_rows": bool(same)}
            nt = LD_BLOCK // TILE
            pairs = LD_BLOCK * W + (nt * (nt + 1) // 2) * TILE * TILE     # executed: the window part, the lower tiles
            med, ps = statistics.median(kern), pairs * n
            res["windows"][str(W)] = {
                "kernel_ms": [x * 1e3 for x in kern], "median_kernel_ms": med * 1e3,
                "call_ms": [x * 1e3 for x in wall], "median_call_ms": statistics.median(wall) * 1e3,
                "pairs_executed": pairs, "pairs_wanted": LD_BLOCK * W + LD_BLOCK * (LD_BLOCK - 1) // 2, "pair_samples": ps, "pair_samples_per_s": ps / med, "int8_ops_per_s": 12 * ps / med,
                "fraction_of_int8_peak": 12 * ps / med / PEAK_I8, "pairs_in_ld": int(flags[:, :W].sum()), **extra}
    res["note"] = ("one run on one MI355X; median of 5 calls after a warm-up; kernel time by HIP events, call time by the "
                   "host clock with the block's upload and the flags' download inside; pair-samples and the fraction of the peak count the pairs the kernel executes; the numpy reference is timed once on 16 rows of the block")
    print(json.dumps(res))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
