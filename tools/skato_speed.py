#!/usr/bin/env python3
"""Speed record of the SKAT-O spectrum stage (sgx_skato_spectra, kern_eig.h) and of the host combination.

    timeout -k 10 600 python tools/skato_speed.py [--problems 64] [--out FILE]

At m = 16, 64 and 256, `problems` (64) matrices A = diag(w) G' diag(v) G diag(w) of random hard calls with weights
dbeta(maf; 1, 25), the default grid of seven rho (eight matrices per problem), in one run on one device:
  (a) the device: Scanner.skato_spectra on all problems, a host clock around the synchronous call -- the upload of the
      matrices, the launches and the download are inside it; a warm-up call, then 5 calls, all recorded, the median
      over the problems is `device_ms_per_problem`;
  (b) numpy on the same box: np.linalg.eigvalsh of the same eight closed-form matrices of 8 of the problems,
      `numpy_ms_per_problem`;
  (c) the host combination: skato_pvalue with the device's spectra handed in, on 8 problems, `combine_ms_per_problem`;
  (d) the sweeps the kernel took (that rotated): largest and mean per matrix kind.
(a) and (b) also give the largest |dlam| / (m eps lam_max) between the two on the timed matrices.  A run without a
device fails; nothing falls back.  Writes profiles/skato_speed.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def problem(m, seed):
    rng = np.random.default_rng(seed)
    rows = max(400, 2 * m)
    maf = np.exp(rng.uniform(np.log(0.005), np.log(0.5), m))
    G = rng.binomial(2, maf[None, :], size=(rows, m)).astype(np.float64)
    G[rng.integers(0, rows, m), np.arange(m)] += 1.0
    w = 25.0 * (1 - maf) ** 24
    A = (G * rng.uniform(0.05, 0.25, rows)[:, None]).T @ G * w[:, None] * w[None, :]
    return np.ascontiguousarray(0.5 * (A + A.T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skato_speed.json"))
    a = ap.parse_args()
    import torch
    from conftest import scan_model
    from saigegds_amd._lib import Scanner
    from saigegds_amd.skato import RHO_DEFAULT, skato_matrices, skato_pvalue
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    eps = float(np.finfo(np.float64).eps)
    res = {"device": torch.cuda.get_device_name(0), "problems": a.problems, "rho": list(RHO_DEFAULT), "runs": 1, "sizes": {}}
    with Scanner(scan_model("saige_model.npz", mac=0.0, maf=0.0, missing=1.0)) as sc:
        for m in (16, 64, 256):
            mats = [problem(m, 7919 * m + k) for k in range(a.problems)]
            sc.skato_spectra(mats, RHO_DEFAULT)                                  # warm-up: code objects, buffers
            ms = []
            for _ in range(5):
                t = time.perf_counter()
                lam, sw = sc.skato_spectra(mats, RHO_DEFAULT)
                ms.append(1e3 * (time.perf_counter() - t))
            t = time.perf_counter()
            ref = [np.array([np.linalg.eigvalsh(B) for B in skato_matrices(A, RHO_DEFAULT)]) for A in mats[:8]]
            np_ms = 1e3 * (time.perf_counter() - t) / 8
            off = max(float((np.abs(x - y).max(axis=1) / (m * eps * np.abs(y).max(axis=1))).max()) for x, y in zip(lam, ref))
            rng = np.random.default_rng(m)
            ss = [np.linalg.cholesky(A + 1e-12 * np.trace(A) * np.eye(m)) @ rng.standard_normal(m) for A in mats[:8]]
            t = time.perf_counter()
            pv = [skato_pvalue(s, A, RHO_DEFAULT, spectra=x)["pval"] for s, A, x in zip(ss, mats[:8], lam)]
            cb_ms = 1e3 * (time.perf_counter() - t) / 8
            res["sizes"][str(m)] = {
                "device_call_ms": ms, "device_ms_per_problem": float(np.median(ms)) / a.problems,
                "numpy_ms_per_problem": np_ms, "combine_ms_per_problem": cb_ms,
                "device_vs_numpy_worst_dlam_over_m_eps_lmax": off,
                "sweeps_max": int(sw.max()), "sweeps_mean_B": float(sw[:, :-1].mean()), "sweeps_mean_W": float(sw[:, -1].mean()),
                "pval_finite": int(np.sum(np.isfinite(pv)))}
            print(m, json.dumps(res["sizes"][str(m)]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
