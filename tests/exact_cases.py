"""The rows of the exact-p-value tests (tests/test_gpu_exact.py) -- TEST INFRASTRUCTURE ONLY, no GPU.

``case(n)``: fitted means in [1e-3, 0.999] (no p-value underflows), a trait, the rows of ``ROWS`` as 2-bit codes with
the tables the driver would make for them, and their reference (tests/exact_ref.py) at max_mac = 63.  The seeds are
such that for every row and every a != A_obs the gap |d_a - d_obs| is exactly 0 or at least 1e-6 in rationals, so that
the kernel's comparisons in double and the reference's in rationals fall the same way (checked on the CPU by
tests/test_exact_ref.py, for every N of the GPU test)."""
import numpy as np

import exact_ref as R

NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 16385)
ROWS = ("one het", "one hom alone", "hets and homs, MAC 63", "carriers at samples 0 and N - 1", "all carriers cases",
        "all carriers controls", "flipped table", "flipped table, one missing", "one missing sample", "5 % missing",
        "hets only, 1 % missing")
_cache = {}


def tables(codes):
    """The driver's tables: the scan's AF over the non-missing samples -> firth_tables."""
    from saigegds_amd import firth
    num = (codes < 3).sum(axis=1)
    af = np.where(codes < 3, codes, 0).sum(axis=1) / (2.0 * num)
    return firth.firth_tables(af)[0]


def model_values(n):
    rng = np.random.default_rng(1000 + n)
    mu = rng.uniform(1e-3, 0.999, n)
    y = (rng.random(n) < 0.3).astype(np.float64)
    if n > 1:
        y[0], y[n - 1] = 1.0, 0.0
    return mu, y


def rows(n, y):
    rng = np.random.default_rng(2000 + n)
    codes = np.zeros((len(ROWS), n), dtype=np.uint8)
    some = lambda k, pool=None: rng.choice(np.arange(n) if pool is None else pool, min(k, n if pool is None else len(pool)), replace=False)
    codes[0, n // 2] = 1
    codes[1, n // 3] = 2
    if n >= 42:                                                  # 21 homs and 21 hets: MAC 63 exactly
        c = some(42)
        codes[2, c[:21]], codes[2, c[21:]] = 2, 1
    else:                                                        # as many as the row holds
        codes[2, :] = 1
        codes[2, ::2] = 2
    codes[3, 0], codes[3, n - 1] = 1, (2 if n > 1 else 1)
    cases, ctrl = np.flatnonzero(y != 0), np.flatnonzero(y == 0)
    for r, pool in ((4, cases), (5, ctrl)):
        if len(pool) == 0:
            pool = np.arange(n)
        c = some(5, pool)
        codes[r, c] = 1
        codes[r, c[:1]] = 2
    for r in (6, 7):                                             # alt-major rows: the carriers are the codes 1 and 0
        codes[r, :] = 2
        c = some(4 + r)
        codes[r, c[:3]], codes[r, c[3:]] = 0, 1
    if n > 2:
        codes[7, some(1, np.flatnonzero(codes[7] == 2))] = 3
        c = some(7)
        codes[8, c[1:]] = 1
        codes[8, c[1:3]] = 2
        codes[8, c[0]] = 3
        c = some(12)
        codes[9, c[:8]], codes[9, c[8:]] = 1, 2
        codes[9, some(max(1, n // 20), np.flatnonzero(codes[9] == 0))] = 3
        codes[10, some(9)] = 1
        codes[10, some(max(1, n // 100), np.flatnonzero(codes[10] == 0))] = 3
    else:                                                        # no room for a missing sample beside a carrier
        codes[8:, 0] = 1
        codes[7] = codes[6]
    return codes


def case(n):
    """(mu, y, codes, lut, reference out4 at max_mac = 63, smallest non-zero gap of every row)."""
    if n not in _cache:
        mu, y = model_values(n)
        codes = rows(n, y)
        lut = tables(codes)
        if lut[1, 0] == 2:                                       # (N = 1: the lone hom has AF = 1; the table of the other
            lut[1] = [0.0, 1.0, 2.0, 2.0 - lut[1, 3]]            #  orientation -- not one the driver makes, one the entry takes)
        got = [R.exact_row(codes[j], lut[j], mu, y, 63, with_gap=True) for j in range(codes.shape[0])]
        _cache[n] = (mu, y, codes, lut, np.array([g[:4] for g in got]), [g[4] for g in got])
    return _cache[n]
