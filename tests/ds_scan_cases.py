"""The case table of test_gpu_ds_score.py and test_gpu_ds_spa.py -- TEST INFRASTRUCTURE ONLY (numpy: no GPU, no HIP).

Dosage rows (RAW bytes with a value outside 0 / 1 / 2 / 0xFF, INTEGER rows with such a value, REAL rows) take a kernel
family of their own, compiled per covariate count K (csrc/kern_score.h, kern_spa4.h; launchers in host_spa.h):

  K <= 8   score_ds_tile_kernel<P, T> + score_ds_tile_epilogue<P>, P = 2 K + 2: 32 variants x one of `ns` sample ranges
           per workgroup, LDS tiles of tile(K) samples, the partial sums added in split order
  K >= 9   score_ds_kernel<P, 256, T>, one workgroup per variant (every K under set_option("score_v1", 1))
  binary   spa4_moments_ds<K, NC, INPUT> over segments of spa_seg(K) samples, then the per-variant kernels

tile, spa_seg and splits restate the library's formulas, so that test_ds_scan_cases.py can show without a GPU which
edges the shapes reach, and the GPU tests can assert that a case still has more than one split on the part they run on.

  case(n, m, k, trait, kind, seed, spa_pval)   (sm, rows) of a case
  reference(...)                               the oracle's table of a case, computed once and shared
"""
import functools

import numpy as np

NA_INTEGER = -2147483648

# ---- shapes ---------------------------------------------------------------------------------------------
# N = 321 = 5 x 64 + 1: one sample over the 320-sample tile of K = 5, across the 192 / 256 tiles of K = 6 .. 8, and
#     large enough that 16 covariates leave a variance to compare (the note in test_gpu_stress.py)
# N = 4097: two splits of 2112 and 1985 samples, one sample in the second 4096-sample SPA segment
# N = 9001: three splits of 3008, 3008, 2985; several SPA segments at every K, the last one ragged
# M = 33: the second block of 32 variants holds one live variant; M = 96: three full blocks
N_LIST = (321, 4097, 9001)
M_LIST = (1, 33, 96)
K_ALL = tuple(range(1, 17))
K_FEW = (1, 3, 5, 8, 9, 16)
KINDS = ("u8", "f64", "i32")
PREVALENCE = 0.2
N_CU = 256                      # compute units assumed where a case is laid out (MI355X); the GPU tests ask the device

SHAPES = [(n, m, k) for n in N_LIST for m in M_LIST for k in (K_ALL if (n, m) == (4097, 33) else K_FEW)]
# the score stage alone: quantitative models (no SPA stage), binary models with spa_pval = 0 (no variant flagged)
SCORE_CASES = [(n, m, k, trait) for (n, m, k) in SHAPES for trait in ("quantitative", "binary")]
BLOCK_CASES = [(4097, 33, k, trait, kind) for k in (1, 8, 9, 16) for trait in ("quantitative", "binary") for kind in ("u8", "f64")]
# the saddlepoint stage on dosage rows: binary models, spa_pval = 0.05
SPA_CASES = [(4097, 96, k) for k in K_ALL] + [(9001, 96, k) for k in (1, 5, 8, 16)]
SPA_PATH_K = (3, 9, 16)

# rows planted in every case of at least 33 variants
PLANTED = {"all_missing": 2, "all_zero": 7, "all_two": 11, "tail_only": 20, "missing_last_tile": 32}
NONCALL_ROW = 5                 # the row (0 in a one-row case) with the values that keep a block off the 2-bit path
NONCALL_U8, NONCALL_I32 = 3, 5


# ---- the library's formulas -----------------------------------------------------------------------------
def tile(k):
    """Samples per LDS tile of score_ds_tile_kernel<P>: at most 32 KiB of score vectors, a multiple of 64."""
    return max(64, (4096 // (2 * k + 2)) & ~63)


def spa_seg(k):
    """Samples per segment of the series SPA stage (kern_spa2.h): rows of (K + 2) & ~1 doubles in 128 KiB."""
    row = ((k + 2) & ~1) * 8
    return 4096 if row <= 32 else 2048 if row <= 64 else 1024 if row <= 128 else 512


def split_plan(n, m, n_cu):
    """launch_score_fp64: (ns, per) -- the sample ranges of the tiled kernels and their length."""
    vb = (m + 31) // 32
    ns = max(1, min((4 * n_cu + vb - 1) // vb, (n + 4095) // 4096))
    per = (((n + ns - 1) // ns) + 63) & ~63
    return (n + per - 1) // per, per


def splits(n, m, n_cu):
    return split_plan(n, m, n_cu)[0]


def last_tile(n, m, k, n_cu=N_CU):
    """[start, stop) of the last tile of the last split."""
    ns, per = split_plan(n, m, n_cu)
    s0 = (ns - 1) * per
    return s0 + (n - s0 - 1) // tile(k) * tile(k), n


# ---- models and rows ------------------------------------------------------------------------------------
def default_seed(n, m, k):
    return 1000 * k + 7 * m + n % 97


@functools.lru_cache(maxsize=None)
def model(n, k, trait, seed, spa_pval=0.05):
    """As _synthetic_case of test_gpu_parity.py: mac >= 10, missing rate <= 0.1."""
    from saigegds_amd import synth
    from saigegds_amd.nullmod import init_nullmod
    mod = synth.synth_null_model(n, trait, PREVALENCE, n_cov=k, seed=seed)
    return init_nullmod(mod, np.arange(n), float("nan"), 10, 0.1, spa_pval, float(mod.var_ratio[0]))


def codes_of(n, m, k, y, seed):
    """-> (codes [m, n] uint8: 0, 1, 2 and 3 = missing, in the stored orientation; flip [m] bool).  Minor-allele
    frequency log-uniform in [0.01, 0.5], 30 % of the rows alt-major, 1 % of the entries missing; every other ordinary
    row is drawn with more minor alleles among the samples of the upper half of y (a z-score of 2.5 .. 4.5 whatever N:
    the binary cases need flagged variants among 33); every third ordinary row has a call of 1 on the last sample."""
    rng = np.random.default_rng(seed)
    af = 10 ** rng.uniform(-2.0, np.log10(0.5), m)
    hi = y > np.median(y) if np.unique(y).size > 2 else y > 0.5
    frac = max(hi.mean(), 1.0 / n)
    codes = np.zeros((m, n), dtype=np.uint8)
    planted = set(PLANTED.values()) if m >= 33 else set()
    ordinary = np.array([j for j in range(m) if j not in planted])
    flip = np.zeros(m, dtype=bool)
    if m > 1:
        flip[rng.choice(ordinary, size=-(-3 * ordinary.size // 10), replace=False)] = True
    if m == 1:
        af[0] = 0.2
    if m >= 33:
        af[PLANTED["missing_last_tile"]] = 0.2
    for j in range(m):
        p = np.full(n, af[j])
        if j % 2 == 1 and j not in planted:
            d = rng.uniform(2.5, 4.5) / np.sqrt(2 * n * af[j] * frac * (1 - frac))
            p = np.where(hi, af[j] * (1 + d), af[j] * max(0.0, 1 - d * frac / (1 - frac)))
        p = np.clip(p, 0.0, 0.95)
        c = (rng.random(n) < p).astype(np.uint8) + (rng.random(n) < p).astype(np.uint8)
        if flip[j]:
            c = (2 - c).astype(np.uint8)
        if j != PLANTED["missing_last_tile"] or m < 33:
            c[rng.random(n) < 0.01] = 3
        if j % 3 == 0:
            c[n - 1] = 1
        codes[j] = c
    if m >= 33:
        codes[PLANTED["all_missing"]] = 3
        codes[PLANTED["all_zero"]] = 0
        codes[PLANTED["all_two"]] = 2
        tail = n % 64
        assert tail > 0
        codes[PLANTED["tail_only"]] = 0
        codes[PLANTED["tail_only"], n - tail:] = 2
        a, b = last_tile(n, m, k)
        codes[PLANTED["missing_last_tile"], b - min(b - a, max(1, n // 20)):] = 3
    return codes, flip


def rows_of(codes, kind, seed):
    """The stored rows of a kind.  u8: 0xFF = missing and one value 3 (the block is not all hard calls: can_pack fails);
    i32: those with NA_INTEGER and one 5 more (i32_rows_to_f64); f64: the calls times a per-row factor in (0.9, 1.0),
    NaN = missing -- the all-2 row keeps its 2.0 (times a factor it would be a valid row with a constant dosage, whose
    adjusted genotype is rounding noise)."""
    m, n = codes.shape
    row = NONCALL_ROW if m > NONCALL_ROW else 0
    if kind == "f64":
        f = np.random.default_rng(seed + 1).uniform(0.9, 1.0, m)
        f[f <= 0.9] = 0.95
        if m >= 33:
            f[PLANTED["all_two"]] = 1.0
        return np.where(codes == 3, np.nan, codes.astype(np.float64) * f[:, None])
    u8 = np.where(codes == 3, 0xFF, codes).astype(np.uint8)
    u8[row, n // 2] = NONCALL_U8
    if kind == "u8":
        return u8
    assert kind == "i32", kind
    i32 = np.where(u8 == 0xFF, NA_INTEGER, u8.astype(np.int64)).astype(np.int32)
    i32[row, n // 3] = NONCALL_I32
    return i32


def case(n, m, k, trait, kind, seed=None, spa_pval=0.05):
    """-> (sm, rows): the flattened model and the rows [m, n] in the dtype of the kind."""
    seed = default_seed(n, m, k) if seed is None else seed
    sm = model(n, k, trait, seed, spa_pval)
    codes, _ = _codes(n, m, k, trait, seed)
    return sm, rows_of(codes, kind, seed)


@functools.lru_cache(maxsize=None)
def _codes(n, m, k, trait, seed):
    return codes_of(n, m, k, np.asarray(model(n, k, trait, seed).y), seed)


def flip_flags(n, m, k, trait, seed=None):
    return _codes(n, m, k, trait, default_seed(n, m, k) if seed is None else seed)[1]


# ---- the oracle's side ----------------------------------------------------------------------------------
def as_oracle_rows(rows):
    """INTEGER rows as the doubles get_ds makes of them (NA_INTEGER -> NaN)."""
    if rows.dtype == np.int32:
        return np.where(rows == NA_INTEGER, np.nan, rows.astype(np.float64))
    return rows


def oracle_scan(sm, rows, per_row_trace=False):
    """-> (table, valid, trace dict, flagged): the oracle's scan of the rows; flagged = the variants that reach the
    saddlepoint approximation proper (pval_noadj <= spa_pval and |z| >= 2: what the library counts as n_spa), from
    a scan row by row when per_row_trace is set, else None."""
    from oracle import Oracle
    orc = Oracle(sm)
    rows = as_oracle_rows(rows)
    scan = orc.scan_u8 if rows.dtype == np.uint8 else orc.scan_f64
    ref, ref_valid = scan(rows)
    trace = orc.trace.as_dict()
    flagged = None
    if per_row_trace:
        flagged = np.zeros(rows.shape[0], dtype=bool)
        for j in range(rows.shape[0]):
            before = orc.trace.as_dict()
            scan(rows[j:j + 1])
            d = {key: v - before[key] for key, v in orc.trace.as_dict().items()}
            # (a variant whose first cutoff test lets it leave has cutoff_exit and no spa_done)
            flagged[j] = d["spa_entered"] == 1 and not (d["cutoff_exit"] >= 1 and d["spa_done"] == 0 and d["not_converged"] == 0)
    orc.close()
    return ref, ref_valid, trace, flagged


@functools.lru_cache(maxsize=None)
def reference(n, m, k, trait, kind, spa_pval=0.05, per_row_trace=False):
    """The oracle's (table, valid, trace, flagged) of a case: computed once, shared by the tests, not to be written to."""
    sm, rows = case(n, m, k, trait, kind, spa_pval=spa_pval)
    out = oracle_scan(sm, rows, per_row_trace)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


# ---- the comparison both GPU files make ------------------------------------------------------------------
EPS = 2.0 ** -53


def scan(sc, rows):
    """Scanner.scan_u8 / scan_i32 / scan_f64 by the rows' dtype."""
    return {np.dtype(np.uint8): sc.scan_u8, np.dtype(np.int32): sc.scan_i32, np.dtype(np.float64): sc.scan_f64}[rows.dtype](rows)


def check(out, valid, ref, ref_valid, n, kind, quant, what):
    """valid equal; AF / mac / num equal for u8 and i32 rows (integer sums are exact); for f64 rows num equal (a count)
    and AF and mac within 2 N 2^-53 of the sum AC they are made of -- two double sums of N non-negative terms in
    different orders differ by at most that much of the sum.  For AF = AC / (2 num), and for mac = AC of a ref-major
    row, that is the bound relative to the column itself; for an alt-major row mac = 2 num - AC is a difference, its
    error is AC's, and the bound is 2 N 2^-53 AC, not 2 N 2^-53 mac: relative to mac the oracle's own sequential sum is
    off the exact rational value by up to 5.3 x (2 N 2^-53) in these cases (N = 4097, K = 2; 2.8 x at N = 321, 2.5 x
    at N = 9001), so no kernel can be held to that.  beta / SE / pval[/ p.norm / converged] by the project's 1e-10
    rule (conftest.assert_table_close, unchanged).  Prints the worst ratio to each tolerance."""
    from conftest import assert_table_close, table_errors
    assert np.array_equal(valid, ref_valid), f"{what}: filter mask differs"
    v = ref_valid.astype(bool)
    o = out.copy()
    if kind == "f64":
        tol = 2 * n * EPS
        ov, rv = out[v], ref[v]
        ac = 2 * rv[:, 0] * rv[:, 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.stack([np.abs(ov[:, 0] - rv[:, 0]) / (tol * rv[:, 0]), np.abs(ov[:, 1] - rv[:, 1]) / (tol * ac)], axis=1)
        e = np.where(ov[:, :2] == rv[:, :2], 0.0, e)
        head = float(e.max()) if e.size else 0.0
        print(f"{what}: AF / mac off by {head:.3g} x (2 N 2^-53) of their sum")
        assert not np.isnan(e).any() and head <= 1.0, f"{what}: AF / mac off by {head:.3g} x (2 N 2^-53) of their sum"
        assert np.array_equal(ov[:, 2], rv[:, 2]), f"{what}: num is a count"
        o[:, :3] = ref[:, :3]
    worst = {name: (float(np.nanmax(e)) if e.size else 0.0) for name, e in table_errors(o[v], ref[v], quant).items()}
    print(f"{what}: worst errors in units of the tolerance {worst}")
    assert_table_close(o, valid, ref, ref_valid, quant=quant, what=what)
    assert np.isnan(out[~v]).all(), f"{what}: a rejected variant's row is not NaN"
