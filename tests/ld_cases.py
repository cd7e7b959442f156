"""The case table of the LD tests: rows for the counts kernel at every sample count around a dword, a 16-byte lane
load, a 64-byte unit and several sample slabs, the row counts around the 16-row fragment and the 32-row wave tile, the
special rows, the padding, and the synthetic source of the pruning driver."""
import numpy as np

import ld_ref as R

NS = (1, 3, 4, 5, 63, 64, 65, 127, 129, 255, 257, 1023, 1025, 4097, 16385)
# (ma, mb) drawn from 1, 15, 16, 17, 33, 65 -- paired with the sample counts in turn, not the full product
SHAPES = ((1, 1), (15, 17), (16, 16), (17, 15), (33, 65), (65, 33), (1, 65), (65, 1), (16, 33), (33, 17), (17, 17),
          (65, 65), (15, 1), (33, 16), (65, 65))
COUNT_CASES = tuple((n, ma, mb) for n, (ma, mb) in zip(NS, SHAPES))
TIE_X, TIE_Y = (0, 1, 1, 2), (0, 1, 2, 1)                       # c = 4, vx = vy = 8: r = 1/2 exactly


def random_codes(n, m, seed, missing=0.05):
    """m rows: allele frequencies 0.05 to 0.5, `missing` of the calls missing; rows 0..3 (as far as m goes) are all
    missing, monomorphic (all 0), called on the even samples only and called on the odd samples only (a pair with
    n = 0); row 4 is called on sample 0 alone and row 5 everywhere (n = 1 against row 4)."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, (m, 1))
    u = rng.random((m, n))
    codes = ((u < f * f).astype(np.uint8) + (u < 1 - (1 - f) ** 2)).astype(np.uint8)
    codes[rng.random((m, n)) < missing] = 3
    if m > 0:
        codes[0] = 3
    if m > 1:
        codes[1] = 0
    if m > 2:
        codes[2, 1::2] = 3
    if m > 3:
        codes[3, 0::2] = 3
    if m > 4:
        codes[4, 1:] = 3
        codes[4, 0] = 1
    if m > 5:
        codes[5] = np.where(codes[5] == 3, 2, codes[5])
    return codes


def padded(codes, extra, seed):
    """Packed rows at stride ceil(n/4) + extra: random bytes in the padding and random bits in the fields of the
    last byte at and beyond n."""
    rng = np.random.default_rng(seed)
    m, n = codes.shape
    p = R.pack(codes)
    if n % 4:
        p[:, -1] |= (rng.integers(0, 256, m, dtype=np.uint8) << np.uint8(2 * (n % 4))).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([p, rng.integers(0, 256, (m, extra), dtype=np.uint8)], axis=1))


def ld_source(n=120, per_chrom=(90, 70, 60, 40), names=("1", "chr7", "chrX", "2"), seed=11, missing=0.02):
    """A synthetic file with LD to prune: within a chromosome each row is, with probability 0.7, a noisy copy of the row
    before it (5 % of its calls redrawn), else a fresh one.  Positions are irregular and non-decreasing, with repeats.
    -> (codes [M, n], chromosome names per row, positions, variant ids)."""
    rng = np.random.default_rng(seed)
    rows, chrom, pos = [], [], []
    for name, m in zip(names, per_chrom):
        p = 1000
        prev = None
        for _ in range(m):
            f = rng.uniform(0.1, 0.5)
            fresh = rng.binomial(2, f, n).astype(np.uint8)
            if prev is not None and rng.random() < 0.7:
                row = np.where(rng.random(n) < 0.05, fresh, prev)
            else:
                row = fresh
            prev = row
            row = row.copy()
            row[rng.random(n) < missing] = 3
            rows.append(row)
            chrom.append(name)
            p += int(rng.choice([0, 0, 1, 7, 50, 400, 3000]))
            pos.append(p)
    codes = np.stack(rows)
    codes[5] = 0                                       # a monomorphic row and one over the missing rate
    codes[9, : n // 2] = 3
    ids = np.arange(1, codes.shape[0] + 1) * 3 + 1000
    return codes, chrom, np.asarray(pos, dtype=np.int64), ids


DRIVER_CPU = dict(n=120, per_chrom=(90, 70, 60, 40), seed=11)           # the driver on the numpy engine
DRIVER_GPU = dict(n=500, per_chrom=(1200, 900, 500, 400), seed=12)      # the driver on the device: M = 3000
THRESHOLDS = (0.2, 0.5)                                                  # the t of every decision the tests take
FLAG_ROWS = dict(n=257, per_chrom=(150,), names=("1",), seed=13)        # block() against the reference decision
RING = dict(n=129, m=600, seed=4, t2=0.01)                                # the window ring: uniform codes 0..2, no missing
# The drivers' sample subsets: samples first::step.  (Starting at sample 0 either table holds a pair with r^2 = 1/25
# exactly, within an ulp of the double 0.2 * 0.2: such inputs are kept out -- tests/test_ld_ref.py checks these.)
SUBSETS = {"DRIVER_CPU": (1, 2), "DRIVER_GPU": (1, 3)}


def subset(name, n):
    first, step = SUBSETS[name]
    return np.arange(first, n, step)


def ring_codes():
    return np.random.default_rng(RING["seed"]).integers(0, 3, (RING["m"], RING["n"]), dtype=np.uint8)
