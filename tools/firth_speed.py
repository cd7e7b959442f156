#!/usr/bin/env python3
"""Speed record of the Firth kernel (sgx_firth_2bit_dev), N = 430 000, K = 3, cases : controls = 1 : 99.

    timeout -k 10 900 python tools/firth_speed.py [--n N] [--rows M] [--out FILE]

Synthetic resident 2-bit rows (the benchmark's generator), `rows` (2 048) of each class: MAF 0.001, 0.05, 0.3 and
alt-major 0.3 (flipped by the scan), 0.5 % missing.  Per class, in one run:
  (a) resident rows -> out4: sgx_firth_2bit_dev + sgx_sync, best of 3 calls after a warm-up call; ms per row, entries
      of the lists (samples with a non-zero dosage, from the scan's AF and counts), iterations;
  (b) the yardstick: the exact per-variant SPA kernel of kern_spa.h on the same rows -- a scan of them with the SPA
      threshold at 1 and the `force_dense` option, whose SPA stage (stats: ms_spa over n_spa variants) is that kernel:
      dense pass, compaction, Newton on the compact list, one workgroup per flagged variant.
No ratio is asked of the two; both are recorded.  Writes profiles/firth_speed.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = (("maf_0.001", 0.001, 0.0), ("maf_0.05", 0.05, 0.0), ("maf_0.3", 0.3, 0.0), ("maf_0.3_flipped", 0.3, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "firth_speed.json"))
    a = ap.parse_args()
    import torch
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.cond import _tables
    from saigegds_amd.nullmod import init_nullmod
    n, m = a.n, a.rows
    dev = torch.device("cuda", 0)
    mod = synth.synth_null_model(n, "binary", 0.01, n_cov=a.k, seed=1)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 1.0, float(mod.var_ratio[0]))      # every valid row is flagged
    res = {"n_samp": n, "k": a.k, "cases": int(np.sum(sm.y)), "rows_per_class": m, "classes": {}}
    with Scanner(sm) as sc:
        bpv = sc.row_stride()
        rows = torch.empty((m, bpv), dtype=torch.uint8, device=dev)
        out8 = torch.empty((m, 8), dtype=torch.float64, device=dev)
        valid = torch.zeros(m, dtype=torch.uint8, device=dev)
        out4 = torch.empty((m, 4), dtype=torch.float64, device=dev)
        for ci, (name, maf, flip) in enumerate(CLASSES):
            lg = float(np.log10(maf))
            thr = torch.from_numpy(synth.variant_thresholds(ci * m, m, 1, (lg, lg), flip, 0.005).view(np.int32)).to(dev)
            torch.cuda.synchronize()
            sc.synth_2bit_dev(rows.data_ptr(), bpv, m, ci * m, 1, thr.data_ptr())
            sc.sync()
            # (b) first: its table gives (a) the tables
            sc.set_option("force_dense", 1)
            spa = []
            for _ in range(3):
                sc.scan_2bit_dev(rows.data_ptr(), bpv, m, out8.data_ptr(), valid.data_ptr())
                sc.sync()
                spa.append(sc.stats())
            sc.set_option("force_dense", 0)
            best = min(spa[1:], key=lambda s: s["ms_spa"])
            lut = _tables(out8[:, 0], valid != 0)
            torch.cuda.synchronize()
            times = []
            for _ in range(4):
                t = time.perf_counter()
                sc.firth_2bit_dev(rows.data_ptr(), bpv, m, lut.data_ptr(), out4.data_ptr())
                sc.sync()
                times.append(time.perf_counter() - t)
            o4, o8 = out4.cpu().numpy(), out8.cpu().numpy()
            ok = o4[:, 3] == 1
            af, num = o8[:, 0], o8[:, 2]
            q = np.where(af > 0.5, 1 - af, af)
            entries = num * (1 - (1 - q) ** 2) + (n - num)            # expected carriers of the minor allele + the imputed samples
            firth_ms = min(times[1:]) * 1e3
            res["classes"][name] = {
                "maf": maf, "alt_major": bool(flip), "valid_rows": int((valid != 0).sum().item()),
                "firth_ms": [x * 1e3 for x in times], "firth_ms_per_row": firth_ms / m,
                "list_entries_mean": float(np.nanmean(entries)), "firth_ns_per_entry": firth_ms * 1e6 / float(np.nansum(entries)),
                "converged": int(ok.sum()), "iterations_mean": float(o4[ok, 2].mean()) if ok.any() else None,
                "iterations_max": float(o4[ok, 2].max()) if ok.any() else None,
                "spa_exact_rows": int(best["n_spa"]), "spa_exact_ms": float(best["ms_spa"]),
                "spa_exact_ms_per_row": float(best["ms_spa"]) / max(1, int(best["n_spa"])),
            }
            c = res["classes"][name]
            c["firth_over_spa_exact_per_row"] = c["firth_ms_per_row"] / c["spa_exact_ms_per_row"] if c["spa_exact_rows"] else None
    res["note"] = ("one run on one MI355X; host wall time around sgx_firth_2bit_dev + sgx_sync, best of 3 after a warm-up; "
                   "spa_exact: ms_spa of a scan with force_dense (kern_spa.h's kernel for every row that enters the SPA stage; "
                   "rows with |z| < 2 leave before it and are not counted)")
    print(json.dumps(res))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
