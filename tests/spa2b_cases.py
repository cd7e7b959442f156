"""The case table of test_gpu_spa2b.py -- TEST INFRASTRUCTURE ONLY (numpy: no GPU, no HIP).

The saddlepoint stage of packed 2-bit rows routes a flagged variant by its carrier count (spa_tier, dev_common.h):
at most SPA5_NNZ = 8192 carriers and it goes to the per-variant kernels (spa5_kernel), more and it enters the
cumulant pass over sample segments (spa4_moments<K, 12> / <K, 16> and spa4_solve: tiers A and B).  At the N <= 5000
of the other 2-bit tests no row has that many carriers, so the cases here are the smallest at which one has:

  SERIES_CASES   N = 16 385 = 4 x 4096 + 1 at every K (the last segment of every segment length holds one sample) and
                 N = 20 011 at one K per segment length (ragged last segment, N no multiple of 64); 96 rows
  ROWLEN_CASES   the forms of spa5_kernel by the length of the packed row (N + 63) / 64 * 16: N = 131 137, one
                 sample past 32 KiB + 16 bytes (512 threads, the row staged in LDS below the 48 KiB at which the
                 shared-memory attribute is set), and N = 491 585, one sample past 120 KiB + 16 bytes (not staged);
                 48 rows, K = 3 and 9 (UNG = 4 and 2 gathers per thread and step)

Models: binary, prevalence 0.2 as in ds_scan_cases.py (the models themselves are its models: one cache) -- at
N = 16 385 that is 3 300 cases, enough for a planted excess of minor alleles among them to give z-scores up to 6
at a minor-allele frequency of 0.01 with mac >= 10 and missing rate <= 0.1; spa_pval = 0.05.

Rows (rows / codes): pairs of rows alternate between COMMON, minor-allele frequency uniform in [0.36, 0.5] -- at
least 59 % of the samples carry the minor allele, about 9 600 of 16 385, over 8192 -- and RARE TO MODERATE,
log-uniform in rare_band(n): [0.01, 0.2] in the SERIES_CASES; in the ROWLEN_CASES scaled down so that 2 N af plus the
1 % of missing entries (which count as carriers) stays under 8192.  30 % of the rows are alt-major, 1 % of the
entries missing.  Every other row is drawn with an excess of minor alleles among the cases, by the construction of
ds_scan_cases.codes_of, for a z-score between 2.1 and 6: weak signals give short series (tier A), strong ones are
handed on to tier B or to the exact sweeps.  Which tier a variant starts in depends on SPA4_TIER_X applied to the
score-stage sums; the tests assert the routing by carrier count, which `carriers` restates exactly, not that split.
Planted: the rows of ds_scan_cases.PLANTED (the missing genotypes of "missing_last_tile" lie in the last SPA segment)
and FIRST_SEG_ROW, a common row whose only carrier outside the first segment is the last sample.

  model(n, k, seed)           the flattened model
  codes(n, m, k, seed)        (codes [m, n] uint8 0 / 1 / 2 / 3 = missing, flip [m])
  rows(n, m, k, seed)         the packed rows (pack_dosage_2bit)
  reference(n, m, k, seed)    (oracle table, valid, flagged per row), computed once and shared
"""
import functools

import numpy as np

import ds_scan_cases as D

PREVALENCE = D.PREVALENCE
SPA5_NNZ = 8192

K_ALL = tuple(range(1, 17))
K_PER_SEG = (1, 4, 8, 16)            # segments of 4096, 2048, 1024, 512 samples
N_SERIES = 16385
SERIES_CASES = [(N_SERIES, 96, k) for k in K_ALL] + [(20011, 96, k) for k in K_PER_SEG]
N_STAGED_NO_ATTR, N_UNSTAGED = 131137, 491585
ROWLEN_CASES = [(n, 48, k) for n in (N_STAGED_NO_ATTR, N_UNSTAGED) for k in (3, 9)]

PLANTED = D.PLANTED
FIRST_SEG_ROW = 41                   # (odd: drawn with a signal; not a PLANTED row)
Z_LO, Z_HI = 2.1, 6.0

spa_seg = D.spa_seg


def default_seed(n, m, k):
    return 2000 * k + 11 * m + n % 89


def row_bytes(n):
    """Bytes of a packed row as the per-variant kernels count them (host_spa.h: rowb5)."""
    return (n + 63) // 64 * 16


def rare_band(n):
    """Frequencies of the rare-to-moderate rows: [0.01, 0.2] while that keeps 2 N af + 1 % N under 8192 carriers
    (N <= 20 011 here), else [hi / 20, hi] with 2 N hi = 3200 (mac >= 160 at the low end)."""
    if n <= 20480:
        return 0.01, 0.2
    hi = 3200.0 / (2 * n)
    return hi / 20, hi


def carriers(codes_row, flip):
    """The count spa_push is given: n1 + n2 + n3 of a ref-major row, N - n2 of an alt-major one."""
    c = np.asarray(codes_row)
    return int((c != 2).sum()) if flip else int((c != 0).sum())


def model(n, k, seed):
    return D.model(n, k, "binary", seed)


def codes_of(n, m, k, y, seed):
    """-> (codes [m, n], flip [m]).  As ds_scan_cases.codes_of: p = af (1 + d) among the cases, af (1 - d f / (1 - f))
    among the controls (f = the share of cases), d = z (1 - f) sqrt(1 - af) / sqrt(2 n af f (1 - f)) for an expected
    z-score of z."""
    assert m >= 48 and n % 64 != 0
    rng = np.random.default_rng(seed)
    lo, hi = rare_band(n)
    common = (np.arange(m) // 2) % 2 == 0
    af = np.where(common, rng.uniform(0.36, 0.5, m), 10 ** rng.uniform(np.log10(lo), np.log10(hi), m))
    z = rng.uniform(Z_LO, Z_HI, m)
    case = np.asarray(y) > 0.5
    frac = case.mean()
    planted = set(PLANTED.values())
    ordinary = np.array([j for j in range(m) if j not in planted])
    flip = np.zeros(m, dtype=bool)
    flip[rng.choice(ordinary, size=-(-3 * ordinary.size // 10), replace=False)] = True
    af[PLANTED["missing_last_tile"]] = 0.2 if n <= 20480 else hi
    af[FIRST_SEG_ROW] = 0.45
    seg = spa_seg(k)
    out = np.zeros((m, n), dtype=np.uint8)
    for j in range(m):
        if j in (PLANTED["all_missing"], PLANTED["all_zero"], PLANTED["all_two"], PLANTED["tail_only"]):
            continue
        p = np.full(n, af[j])
        if j % 2 == 1:
            n_eff = seg if j == FIRST_SEG_ROW else n
            d = z[j] * (1 - frac) * np.sqrt(1 - af[j]) / np.sqrt(2 * n_eff * af[j] * frac * (1 - frac))
            p = np.where(case, af[j] * (1 + d), af[j] * max(0.0, 1 - d * frac / (1 - frac)))
        p = np.clip(p, 0.0, 0.95)
        c = (rng.random(n) < p).astype(np.uint8) + (rng.random(n) < p).astype(np.uint8)
        if j == FIRST_SEG_ROW:
            c[seg:] = 0
            c[n - 1] = 1
            flip[j] = False
        if flip[j]:
            c = (2 - c).astype(np.uint8)
        if j not in (PLANTED["missing_last_tile"], FIRST_SEG_ROW):
            c[rng.random(n) < 0.01] = 3
        out[j] = c
    out[PLANTED["all_missing"]] = 3
    out[PLANTED["all_zero"]] = 0
    out[PLANTED["all_two"]] = 2
    tail = n % 64
    out[PLANTED["tail_only"], n - tail:] = 2
    flip[PLANTED["tail_only"]] = False
    a = (n - 1) // seg * seg                     # the last SPA segment is [a, n)
    out[PLANTED["missing_last_tile"], n - min(n - a, max(1, n // 20)):] = 3
    return out, flip


@functools.lru_cache(maxsize=None)
def _codes(n, m, k, seed):
    c, f = codes_of(n, m, k, np.asarray(model(n, k, seed).y), seed)
    c.setflags(write=False)
    f.setflags(write=False)
    return c, f


def codes(n, m, k, seed=None):
    return _codes(n, m, k, default_seed(n, m, k) if seed is None else seed)


def rows(n, m, k, seed=None):
    """The packed 2-bit rows [m, ceil(n / 4)] of a case."""
    from saigegds_amd.gds import pack_dosage_2bit
    return pack_dosage_2bit(codes(n, m, k, seed)[0])


def case(n, m, k, seed=None):
    """-> (sm, packed rows)"""
    seed = default_seed(n, m, k) if seed is None else seed
    return model(n, k, seed), rows(n, m, k, seed)


@functools.lru_cache(maxsize=None)
def reference(n, m, k, seed=None):
    """The oracle's (table, valid, flagged [m] bool) of a case, from ds_scan_cases.oracle_scan on the hard calls as
    bytes (0xFF = missing) with its trace row by row: computed once, shared by the tests, not to be written to."""
    seed = default_seed(n, m, k) if seed is None else seed
    c, _ = _codes(n, m, k, seed)
    ref, valid, _, flagged = D.oracle_scan(model(n, k, seed), np.where(c == 3, 0xFF, c).astype(np.uint8), per_row_trace=True)
    for a in (ref, valid, flagged):
        a.setflags(write=False)
    return ref, valid, flagged


def flagged_groups(n, m, k):
    """-> dict of the per-row masks the tests count: flagged, many (carriers > SPA5_NNZ), flip (alt-major by the
    row's own allele frequency, as the library decides it: AF > 0.5; False where the row is rejected)."""
    c, _ = codes(n, m, k)
    ref, valid, flagged = reference(n, m, k)
    with np.errstate(invalid="ignore"):
        flip = (valid != 0) & (ref[:, 0] > 0.5)
    many = np.array([carriers(c[j], flip[j]) > SPA5_NNZ for j in range(m)])
    return {"flagged": flagged, "many": many, "flip": flip}
