#!/usr/bin/env python3
"""Timing of the multi-vector GRM operator (sgx_grm_crossprod_multi_dev / sgx_grm_pcg_multi) against the
single-vector calls, on a synthetic device-resident genotype matrix (sgx_grm_init_dev):

  * crossprod_many for k = 1, 8, 16, 32 against k single products (device vectors, back to back);
  * one pcg_many of 30 +-1 vectors (the Hutchinson trace of get_trace) against 30 single solves;
  * one seqGLMM_GxG_spa pair end to end (use_approx_tau=False), its GRM the same matrix.

    python tools/grm_batch_bench.py [--n-samp 430000] [--markers 100000] [--reps 3] [--no-pair]

Prints one JSON line (DESIGN.md section "Several right-hand sides")."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _matrix(n, m, seed):
    """Synthetic 2-bit genotypes generated on the device (as bench_grm.py)."""
    import torch
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.nullmod import init_nullmod
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
    gen.n = min(n, 20000)
    gen.close()
    return packed, bpv


def measure(n=430_000, m=100_000, reps=3, pair=True, seed=20260):
    import torch
    from saigegds_amd._lib import GrmOperator
    if not torch.cuda.is_available():
        raise SystemExit("grm_batch_bench.py needs an MI355X")
    dev = torch.device("cuda", 0)
    packed, bpv = _matrix(n, m, seed)
    op = GrmOperator(None, n, 0, dev_ptr=packed.data_ptr(), n_markers=m, bytes_per_marker=bpv)
    rng = np.random.default_rng(1)
    line = {"metric": "multi-vector implicit-GRM operator", "n_samples": n, "n_markers": m, "reps": reps}

    # ---- products
    B = torch.from_numpy(rng.standard_normal((32, n))).to(dev)
    O = torch.empty_like(B)
    torch.cuda.synchronize()
    op.crossprod_dev(B[0].data_ptr(), O[0].data_ptr())
    op.crossprod_many_dev(B.data_ptr(), n, 32, O.data_ptr())
    op.sync()
    prod = {}
    for k in (1, 8, 16, 32):
        t0 = time.perf_counter()
        for _ in range(reps):
            for j in range(k):
                op.crossprod_dev(B[j].data_ptr(), O[j].data_ptr())
        op.sync()
        t_single = (time.perf_counter() - t0) / reps
        single = O[:k].clone()
        t0 = time.perf_counter()
        for _ in range(reps):
            op.crossprod_many_dev(B.data_ptr(), n, k, O.data_ptr())
        op.sync()
        t_many = (time.perf_counter() - t0) / reps
        prod[str(k)] = {"ms_single_x_k": round(t_single * 1e3, 2), "ms_many": round(t_many * 1e3, 2),
                        "ratio": round(t_many / t_single, 4), "bit_identical": bool(torch.equal(single, O[:k]))}
    line["crossprod_many"] = prod

    # ---- the 30 trace vectors of one get_trace call
    mu = rng.uniform(0.02, 0.4, n)
    w, tau = mu * (1 - mu), np.array([1.0, 0.3])
    U = 2.0 * rng.integers(0, 2, (30, n)) - 1
    t0 = time.perf_counter()
    X1 = np.empty_like(U)
    it1 = np.zeros(30, dtype=np.int64)
    for j in range(30):
        X1[j], it1[j] = op.pcg(w, tau, U[j], 500, 1e-5)
    t_single = time.perf_counter() - t0
    t0 = time.perf_counter()
    X, it = op.pcg_many(w, tau, U, 500, 1e-5)
    t_many = time.perf_counter() - t0
    line["pcg_many_30"] = {"s_single_x_30": round(t_single, 3), "s_many": round(t_many, 3),
                           "speedup": round(t_single / t_many, 3), "iterations": [int(it.min()), int(it.max())],
                           "same_iterations": bool(np.array_equal(it, it1)), "bit_identical": bool(np.array_equal(X, X1)),
                           "tau": tau.tolist(), "tol": 1e-5}
    del B, O

    # ---- one interaction pair end to end: 2 covariates, the two SNPs and their product refitted with the GLMM
    if pair:
        from saigegds_amd.assoc import GenotypeSource
        from saigegds_amd.gds import pack_dosage_2bit
        from saigegds_amd.gxg import seqGLMM_GxG_spa
        sid = [f"s{i}" for i in range(n)]
        x1, x2 = rng.standard_normal(n), rng.integers(0, 2, n).astype(np.float64)
        snp = np.stack([rng.binomial(2, 0.2, n), rng.binomial(2, 0.3, n)]).astype(np.uint8)
        eta = -1.0 + 0.3 * x1 + 0.2 * x2 + 0.3 * snp[0] * snp[1]
        y = (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.float64)
        src = GenotypeSource(sid, packed=pack_dosage_2bit(snp), variant_id=np.array([1, 2]))
        t0 = time.perf_counter()
        res = seqGLMM_GxG_spa("y ~ x1 + x2", {"sample.id": sid, "y": y, "x1": x1, "x2": x2}, src, None,
                              {"s1": [1], "s2": [2]}, variant_id=[1, 2], verbose=False,
                              operator_factory=lambda p, nn: _Borrowed(op))
        line["gxg_pair"] = {"seconds": round(time.perf_counter() - t0, 2), "use_approx_tau": False,
                            "pval": float(res["pval"][0]), "tau_G": float(res["tau_G"][0]),
                            "note": "GRM: the synthetic device matrix; the pair's SNPs from a host GenotypeSource"}
    op.close()
    del packed
    torch.cuda.empty_cache()
    return line


class _Borrowed:
    """The bench's operator handed to seqGLMM_GxG_spa without giving it away (close() is a no-op)."""

    def __init__(self, op):
        self._op, self.n = op, op.n

    def __getattr__(self, k):
        return getattr(self._op, k)

    def close(self):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-samp", type=int, default=430_000)
    ap.add_argument("--markers", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-pair", action="store_true", help="skip the end-to-end interaction pair")
    ap.add_argument("--seed", type=int, default=20260)
    args = ap.parse_args()
    print(json.dumps(measure(args.n_samp, args.markers, args.reps, not args.no_pair, args.seed)), flush=True)


if __name__ == "__main__":
    main()
