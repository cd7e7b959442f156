#!/usr/bin/env python3
"""Every result of the GRM operator on the shared test inputs (tests/grm_ref.py), in one .npz, to compare
two builds of the library bit for bit on the same GPU:

    python tools/grm_dump.py OUT.npz [--tree DIR]        # DIR: the checkout whose saigegds_amd is loaded (default: this one)
    python tools/grm_dump.py --compare A.npz B.npz       # exit status 1 unless every array is equal (NaNs equal)

For each of CASES: diag, crossprod of every vector kind (one call each), crossprod_many of all kinds (plus a
NaN and an infinite vector); for each of PCG_SHAPES x PCG_TAUS: pcg per right-hand side and pcg_many of all,
solutions and iteration counts, and both with maxiter = 0."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grm_ref as R  # noqa: E402


def dump(out, tree):
    sys.path.insert(0, os.path.abspath(tree))
    from saigegds_amd._lib import GrmOperator
    arrays = {}
    for c in R.CASES:
        n, m, miss = c
        seed = R.case_seed(n, m, miss)
        codes, B = R.make_codes(n, m, seed, miss), R.vectors(n, seed)
        bad = np.stack([B[0], B[0]])
        bad[0, n // 3] = np.nan
        bad[1, 0] = np.inf
        key = R.case_id(c)
        with GrmOperator(R.pack(codes), n) as op:
            arrays[key + "/diag"] = op.diag()
            for kind, b in zip(R.VECTOR_KINDS, B):
                arrays[key + "/crossprod/" + kind] = op.crossprod(b)
            arrays[key + "/crossprod_many"] = op.crossprod_many(np.concatenate([B, bad]))
            arrays[key + "/crossprod/nan"] = op.crossprod(bad[0])
    for n, m in R.PCG_SHAPES:
        codes, w, B = R.pcg_inputs(n, m)
        with GrmOperator(R.pack(codes), n) as op:
            for tau in R.PCG_TAUS:
                for maxiter in (R.PCG_MAXITER, 0):
                    key = "pcg-n%d-m%d-tau%g,%g-maxiter%d" % (n, m, tau[0], tau[1], maxiter)
                    for name, b in zip(R.PCG_RHS, B):
                        x, it = op.pcg(w, tau, b, maxiter, R.PCG_TOL)
                        arrays[key + "/pcg/" + name] = x
                        arrays[key + "/pcg_iters/" + name] = np.array(it)
                    X, its = op.pcg_many(w, tau, B, maxiter, R.PCG_TOL)
                    arrays[key + "/pcg_many"] = X
                    arrays[key + "/pcg_many_iters"] = np.asarray(its)
    np.savez(out, **arrays)
    print("%d arrays -> %s" % (len(arrays), out))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    names = sorted(set(A.files) | set(B.files))
    bad = [k for k in names if k not in A.files or k not in B.files or A[k].shape != B[k].shape
           or not np.array_equal(A[k], B[k], equal_nan=True)]
    print("%d arrays, %d differ%s" % (len(names), len(bad), ": " + ", ".join(bad[:10]) if bad else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--compare", action="store_true")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.paths)
    dump(args.paths[0], args.tree)
    return 0


if __name__ == "__main__":
    sys.exit(main())
