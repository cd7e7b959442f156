#!/usr/bin/env python3
"""Scan fixed-seed cases through the library and save every table and its valid flags (numpy.save, one group of files
per case and form), or compare two such directories bit for bit: how a change to the kernels of a scan is checked
against its parent on the same GPU.  SAIGEHIP_LIB selects the library (saigegds_amd/_lib.py), so one checkout can dump
both builds.

    python tools/scan_dump.py OUTDIR                  # the score stage: both forms of the contraction kernel
    python tools/scan_dump.py spa OUTDIR              # the SPA stage
    python tools/scan_dump.py --compare DIR_A DIR_B   # exit status 1 on any difference

Score stage: the cases of tests/s3_cases.py -- a quantitative and a binary model with few B fragments (the one-set
three-plane schedule among them), wide binary models, long rows with eight tile groups, full rounds with leftover
tiles; a few thousand variants in all.

SPA stage: the cases of tests/spa2b_cases.py and tests/ds_scan_cases.py.  2-bit rows by the row-major call
(SERIES_CASES at the four K_PER_SEG at N = 16 385 and the four of N = 20 011; default, "score_v1", "spa_exact",
"force_dense"); the N = 16 385 rows resident in a Block (lists used, lists ignored, clist_avg = 300; one lane and two);
one ROWLEN_CASES entry per N at K = 3 (both forms of spa5_kernel); u8 and f64 dosage rows at one K per segment length
(default and "score_v1").  Beside each table and its valid flags the counters n_spa, n_spa_slow, n_spa_dense."""
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


def scan_rows(sc, on):
    """The hook "lists ignored"; a library from before it had the name takes the bit of "spa_abl"."""
    from saigegds_amd._lib import SgxError
    try:
        sc.set_option("spa_scan_rows", on)
    except SgxError as e:
        if e.code != -1:                                  # SGX_EINVAL: the name is unknown to this library
            raise
        sc.set_option("spa_abl", 512 if on else 0)


def dump_spa(outdir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import ds_scan_cases as D
    import spa2b_cases as S
    from saigegds_amd._lib import Block, Scanner
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda", 0)
    count = [0, 0]

    def save(tag, out, valid, st):
        np.save(os.path.join(outdir, f"{tag}.table.npy"), np.ascontiguousarray(out))
        np.save(os.path.join(outdir, f"{tag}.valid.npy"), np.ascontiguousarray(valid))
        np.save(os.path.join(outdir, f"{tag}.counters.npy"),
                np.array([st["n_spa"], st["n_spa_slow"], st["n_spa_dense"]], dtype=np.int64))
        count[0] += 3
        count[1] += len(out)
        print(f"{tag}: {len(out)} variants, n_spa {st['n_spa']} slow {st['n_spa_slow']} dense {st['n_spa_dense']}", flush=True)

    def block_scans(sc, blk, m, n_scans):
        bufs = [(torch.full((m, 8), -1.0, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.uint8, device=dev))
                for _ in range(n_scans)]
        for out, valid in bufs:
            sc.scan_block(blk, out.data_ptr(), valid.data_ptr())
        sc.sync()
        return [(o.cpu().numpy(), v.cpu().numpy()) for o, v in bufs]

    # 2-bit rows, row-major call
    for n, m, k in [c for c in S.SERIES_CASES if c[2] in S.K_PER_SEG]:
        sm, packed = S.case(n, m, k)
        for option in (None, "score_v1", "spa_exact", "force_dense"):
            with Scanner(sm, device=0) as sc:
                if option:
                    sc.set_option(option, 1)
                out, valid = sc.scan_2bit(packed)
                save(f"rows.n{n}.k{k}.{option or 'default'}", out, valid, sc.stats())
    # the N = 16 385 rows resident in a Block
    for k in S.K_PER_SEG:
        n, m = S.N_SERIES, 96
        sm, packed = S.case(n, m, k)
        for lanes in (1, 2):
            with Scanner(sm, device=0) as sc:
                sc.set_option("lanes", lanes)
                for form in ("lists", "norows", "short"):
                    with (Block(sm.n, m, clist_avg=300) if form == "short" else Block(sm.n, m)) as blk:
                        sc.load_block(blk, packed)
                        scan_rows(sc, 1 if form == "norows" else 0)
                        for i, (out, valid) in enumerate(block_scans(sc, blk, m, lanes)):
                            save(f"block.k{k}.lanes{lanes}.{form}.scan{i}", out, valid, sc.stats())
                        scan_rows(sc, 0)
    # both forms of spa5_kernel by row length
    for n, m, k in [c for c in S.ROWLEN_CASES if c[2] == 3]:
        sm, packed = S.case(n, m, k)
        with Scanner(sm, device=0) as sc:
            out, valid = sc.scan_2bit(packed)
            save(f"rowlen.n{n}.k{k}", out, valid, sc.stats())
    # dosage rows
    for k in S.K_PER_SEG:
        for kind in ("u8", "f64"):
            n, m = 4097, 96
            sm, rows = D.case(n, m, k, "binary", kind)
            for option in (None, "score_v1"):
                with Scanner(sm, device=0) as sc:
                    if option:
                        sc.set_option(option, 1)
                    out, valid = D.scan(sc, rows)
                    save(f"ds.{kind}.k{k}.{option or 'default'}", out, valid, sc.stats())
    print(f"{count[0]} arrays of {count[1]} variants -> {outdir}")


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
    print(f"{len(names)} arrays compared, {len(bad)} differ")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 3 and sys.argv[1] == "spa":
        dump_spa(sys.argv[2])
    elif len(sys.argv) == 2:
        dump(sys.argv[1])
    else:
        sys.exit(__doc__)
