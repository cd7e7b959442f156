#!/usr/bin/env python
"""Speed record of the dosage Firth kernel (sgx_ds_block_firth), N = 430 000, K = 3, cases : controls = 1 : 99.

    timeout -k 10 1100 python tools/firth_ds_speed.py [--n N] [--budget BYTES] [--out FILE]

Per frequency class -- those of tools/firth_speed.py (MAF 0.001, 0.05, 0.3 and alt-major 0.3: hard calls from the
synthetic generator) plus "imputed", in which nearly every sample has a small non-zero dosage -- one block of
aggregate.DS_BUDGET bytes of u8 rows and one of f64 rows:
  (a) resident rows -> out4: DosageBlock.firth (synchronous; tables up, results back), best of 3 calls after a warm-up
      call; us per row, list entries, ns per list entry, iterations;
  (b) the yardstick, in the same run: sgx_firth_2bit_dev + sgx_sync on the 2-bit form of the same hard-call rows (the
      imputed class has no 2-bit form).
No ratio is asked of the two; both are recorded.  Writes profiles/firth_ds_speed.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = (("maf_0.001", 0.001, 0.0), ("maf_0.05", 0.05, 0.0), ("maf_0.3", 0.3, 0.0), ("maf_0.3_flipped", 0.3, 1.0),
           ("imputed", None, 0.0))


def best_of(call, reps=4):
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t)
    return out, times


def record(o4, times, entries):
    ok = o4[:, 3] == 1
    m, best = o4.shape[0], min(times[1:])
    return {"rows": m, "ms": [x * 1e3 for x in times], "us_per_row": best * 1e6 / m, "list_entries_mean": float(entries.mean()),
            "ns_per_entry": best * 1e9 / max(1.0, float(entries.sum())), "converged": int(ok.sum()),
            "iterations_mean": float(o4[ok, 2].mean()) if ok.any() else None,
            "iterations_max": float(o4[ok, 2].max()) if ok.any() else None}


def main():
    from saigegds_amd import aggregate
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=430_000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--budget", type=int, default=aggregate.DS_BUDGET)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "firth_ds_speed.json"))
    a = ap.parse_args()
    import torch
    from saigegds_amd import firth, synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import unpack_dosage_2bit
    from saigegds_amd.nullmod import init_nullmod
    n = a.n
    m8, m64 = (max(1, a.budget // aggregate.ds_row_bytes(dt, n)) for dt in (np.uint8, np.float64))
    dev = torch.device("cuda", 0)
    mod = synth.synth_null_model(n, "binary", 0.01, n_cov=a.k, seed=1)
    sm = init_nullmod(mod, np.arange(n), 0.0, 0.0, 1.0, 1.0, float(mod.var_ratio[0]))
    res = {"n_samp": n, "k": a.k, "cases": int(np.sum(sm.y)), "budget_bytes": a.budget, "rows_u8": m8, "rows_f64": m64, "classes": {}}
    rng = np.random.default_rng(2)
    with Scanner(sm) as sc, sc.dosage_block(np.uint8, m8) as b8, sc.dosage_block(np.float64, m64) as b64:
        bpv = sc.row_stride()
        rows = torch.empty((m8, bpv), dtype=torch.uint8, device=dev)
        out4 = torch.empty((m8, 4), dtype=torch.float64, device=dev)
        for ci, (name, maf, flipped) in enumerate(CLASSES):
            c = {"maf": maf, "alt_major": bool(flipped)}
            if maf is None:       # imputed: 95 % of the samples carry a small dosage (u8: the byte 1; f64: (0, 0.05])
                d8 = (rng.random((m8, n), dtype=np.float32) < 0.95).astype(np.uint8)
                d64 = np.where(rng.random((m64, n)) < 0.95, 0.05 * (1 - rng.random((m64, n))), 0.0)
            else:
                lg = float(np.log10(maf))
                thr = torch.from_numpy(synth.variant_thresholds(ci * m8, m8, 1, (lg, lg), flipped, 0.005).view(np.int32)).to(dev)
                torch.cuda.synchronize()
                sc.synth_2bit_dev(rows.data_ptr(), bpv, m8, ci * m8, 1, thr.data_ptr())
                sc.sync()
                codes = unpack_dosage_2bit(rows.cpu().numpy(), n)
                d8 = np.where(codes == 3, 0xFF, codes).astype(np.uint8)
                d64 = np.where(codes[:m64] == 3, np.nan, codes[:m64].astype(np.float64))
                # (b) the yardstick on the 2-bit form of the same rows, tables from the rows' own counts
                num = (codes != 3).sum(axis=1)
                af = np.where(codes != 3, codes, 0).sum(axis=1) / (2.0 * np.maximum(num, 1))
                lut = torch.from_numpy(firth.firth_tables(af)[0]).to(dev)
                torch.cuda.synchronize()

                def two_bit():
                    sc.firth_2bit_dev(rows.data_ptr(), bpv, m8, lut.data_ptr(), out4.data_ptr())
                    sc.sync()
                    return out4.cpu().numpy()
                o4, times = best_of(two_bit)
                g = firth.firth_tables(af)[0]
                ent = np.stack([(codes == k).sum(axis=1) * (g[:, k] != 0) for k in range(4)]).sum(axis=0)
                c["firth_2bit"] = record(o4, times, ent)
            for key, blk, d in (("u8", b8, d8), ("f64", b64, d64)):
                nv, s, _ = blk.load(d)
                fl, mean = aggregate.flip_mean(nv, s)
                idx = np.arange(d.shape[0], dtype=np.int32)
                o4, times = best_of(lambda: blk.firth(idx, fl, mean))
                miss = (d == 0xFF) if d.dtype == np.uint8 else ~np.isfinite(d)
                val = np.where(miss, 0, d).astype(np.float64)
                g = np.where(miss, mean[:, None], np.where(fl[:, None] != 0, 2 - val, val))
                c[key] = record(o4, times, (g != 0).sum(axis=1))
            res["classes"][name] = c
    res["note"] = ("one run on one MI355X; host wall time around DosageBlock.firth (synchronous) and around sgx_firth_2bit_dev "
                   "+ sgx_sync, best of 3 after a warm-up call; the f64 block holds the first rows_f64 rows of the class")
    print(json.dumps(res))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
