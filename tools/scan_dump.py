#!/usr/bin/env python3
"""Scan fixed-seed blocks through the library in both forms of the contraction kernel and save every table and its
valid flags (numpy.save, one pair of files per case and form), or compare two such directories bit for bit: how a
change to score3_kernel, s3_reduce_kernel or score3_epilogue is checked against its parent on the same GPU.

    python tools/scan_dump.py OUTDIR                  # run in each of the two checkouts
    python tools/scan_dump.py --compare DIR_A DIR_B   # exit status 1 on any difference

The cases are those of tests/s3_cases.py: a quantitative and a binary model with few B fragments (the one-set
three-plane schedule among them), wide binary models, long rows with eight tile groups, full rounds with leftover
tiles; a few thousand variants in all."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("q1", "b2", "b4", "b13", "Q16", "ng4", "rounds-three")


def dump(outdir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (before the first HIP call: the library binds to the torch wheel's runtime)
    import s3_cases as S
    from saigegds_amd._lib import Scanner
    os.makedirs(outdir, exist_ok=True)
    total = 0
    for name in CASES:
        (c,) = [c for c in S.CASES if c.name == name]
        sm, packed = S.build(c)
        with Scanner(sm, device=0) as sc:
            for form in (0, 1):
                sc.set_option("three_plane", form)
                out, valid = sc.scan_2bit(packed)
                st = sc.stats()
                assert st["three_plane"] == form and st["score_launches"] > 0, (name, form, st)
                np.save(os.path.join(outdir, f"{name}.form{form}.table.npy"), np.ascontiguousarray(out))
                np.save(os.path.join(outdir, f"{name}.form{form}.valid.npy"), np.ascontiguousarray(valid))
                print(f"{name}: {c.trait} K={c.k} N={c.n} M={len(packed)} NBF={c.nbf} three_plane={form}: "
                      f"{int(np.count_nonzero(valid))} valid, n_spa={st['n_spa']}", flush=True)
        total += len(packed)
    print(f"{total} variants in {len(CASES)} cases, both forms -> {outdir}")


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    bad = sorted(set(names) ^ set(f for f in os.listdir(b) if f.endswith(".npy")))
    for f in bad:
        print(f"{f}: in one directory only")
    for f in names:
        if f in bad:
            continue
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        print(f"{f}: {x.shape} {x.dtype}: {'bit-identical' if same else 'DIFFERENT'}")
        bad += [] if same else [f]
    return 1 if bad or not names else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
