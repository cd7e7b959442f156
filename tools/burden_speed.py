#!/usr/bin/env python3
"""Throughput of the burden calls at N = 430 000 (device collapse + FP64 dosage scan).
2-bit rows (sgx_burden_2bit):      python tools/burden_speed.py [N] [units] [variants_per_unit]
dosage rows (sgx_dsblock_*):       python tools/burden_speed.py --dosage f64|u8 [--n N] [--units U] [--per V] [--cols C]
                                   [--hard] [--reps R]
The dosage mode times load (the one upload of the batch), scan and burden of a DosageBlock separately and prints one
JSON line with the bytes behind each figure; --hard fills the rows with hard calls (the data of the 2-bit mode)."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa
from saigegds_amd import synth
from saigegds_amd._lib import Scanner
from saigegds_amd.nullmod import init_nullmod


def model(N):
    mod = synth.synth_null_model(N, "binary", 0.01, n_cov=3, seed=20260)
    return init_nullmod(mod, np.arange(N), 0.0, 0.0, 1.0, 0.05, float(mod.var_ratio[0]))


def rare_rows(M, N, rng):
    """cheap random rare variants (not the counter-based generator): sample indices of the carriers per row"""
    return [rng.integers(0, N, size=max(1, int(2 * 10 ** rng.uniform(-3.3, -1.5) * N))) for _ in range(M)]


def dosage_mode(argv):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--dosage", choices=("f64", "u8"), required=True)
    ap.add_argument("--n", type=int, default=430000)
    ap.add_argument("--units", type=int, default=20)
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--cols", type=int, default=2)
    ap.add_argument("--hard", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args(argv)
    N, U, V, C = a.n, a.units, a.per, a.cols
    M = U * V
    rng = np.random.default_rng(0)
    dt = np.float64 if a.dosage == "f64" else np.uint8
    ds = np.zeros((M, N), dtype=dt)
    for j, idx in enumerate(rare_rows(M, N, rng)):
        if a.dosage == "f64":
            ds[j, idx] = 1.0 if a.hard else np.rint(rng.uniform(0.3, 2.0, idx.size) * 127) / 127
            ds[j, rng.integers(0, N, size=N // 200)] = np.nan
        else:
            ds[j, idx] = 1 if a.hard else rng.integers(1, 3, idx.size)
            ds[j, rng.integers(0, N, size=N // 200)] = 0xFF
    grp_ptr = np.arange(0, M + 1, V)
    var_idx = np.arange(M, dtype=np.int32)
    w = np.full((M, C), 1.0 / V)
    with Scanner(model(N)) as sc, sc.dosage_block(dt, M) as blk:
        t = {"load": [], "scan": [], "burden": []}
        for rep in range(a.reps + 1):                      # the first round warms up (code objects, workspaces)
            t0 = time.time()
            nv, s, st = blk.load(ds)
            t1 = time.time()
            blk.scan()
            t2 = time.time()
            m = st / np.maximum(nv, 1)
            out, valid = blk.burden(grp_ptr, var_idx, (st > nv).astype(np.uint8), w, m[:, None] * w)
            t3 = time.time()
            stt = sc.stats()
            if rep:
                t["load"].append(t1 - t0); t["scan"].append(t2 - t1); t["burden"].append(t3 - t2)
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps({"mode": "dosage", "dtype": a.dosage, "hard_calls": a.hard, "N": N, "units": U, "per_unit": V, "cols": C,
                      "dosage_bytes": int(ds.nbytes), "uploads_per_batch": 1, "collapsed_row_bytes": U * C * N * 8,
                      "ms_load": med["load"] * 1e3, "ms_scan": med["scan"] * 1e3, "ms_burden": med["burden"] * 1e3,
                      "ms_total": sum(med.values()) * 1e3, "upload_GBps": ds.nbytes / med["load"] / 1e9,
                      "ms_upload_at_55GBps": ds.nbytes / 55e9 * 1e3, "burden_ms_score": stt["ms_score"],
                      "burden_ms_spa": stt["ms_spa"], "valid_rows": int(valid.sum()), "reps": a.reps}))


if "--dosage" in sys.argv:
    dosage_mode(sys.argv[1:])
    sys.exit(0)

N = int(sys.argv[1]) if len(sys.argv) > 1 else 430000
U = int(sys.argv[2]) if len(sys.argv) > 2 else 400
V = int(sys.argv[3]) if len(sys.argv) > 3 else 20
sm = model(N)
M = U * V
thr = synth.variant_thresholds(0, M, 5, log10_maf=(-3.3, -1.5), flip_frac=0.0, miss_rate=1e-3)
rng = np.random.default_rng(0)
packed = np.zeros((M, (N + 3) // 4), dtype=np.uint8)
for j in range(M):                      # cheap random rare variants (not the counter-based generator)
    p = 10 ** rng.uniform(-3.3, -1.5)
    idx = rng.integers(0, N, size=max(1, int(2 * p * N)))
    np.add.at(packed[j], idx // 4, (1 << (2 * (idx % 4))).astype(np.uint8))
lut = np.tile(np.array([0, 1, 2, 0.01]) / V, (M, 1))
row_ptr = np.arange(0, M + 1, V)
with Scanner(sm) as sc:
    sc.burden_2bit(packed[:V * 4], row_ptr[:5], np.arange(V * 4, dtype=np.int32), lut[:V * 4])
    t = time.time()
    out, valid = sc.burden_2bit(packed, row_ptr, np.arange(M, dtype=np.int32), lut)
    dt = time.time() - t
    st = sc.stats()
print(f"N={N} units={U} x {V} variants: {dt*1e3:.1f} ms wall ({U/dt:.0f} burden rows/s incl. H2D of {packed.nbytes/1e6:.0f} MB), "
      f"device score {st['ms_score']:.1f} ms spa {st['ms_spa']:.1f} ms, valid {int(valid.sum())}, n_spa {st['n_spa']}")
