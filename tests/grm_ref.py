"""Long-double reference of the implicit-GRM operator, with the inputs that test_grm_ref.py (the CPU
oracle) and test_gpu_grm_edges.py (the HIP operator) share.  No test functions here.

The operator (reference src/saige_fitnull.cpp:159-230, 435-536):  out = G'(G b) / M  with
G[v, i] = (code_vi - 2 af_v) inv_v, 0 for a missing code.  af_v and inv_v are computed IN DOUBLE, as
saige_fitnull.cpp:181-203, oracle/grm_oracle.c and grm_marker_stats do -- they are part of the
operator's definition -- and everything after them in np.longdouble (80-bit extended here).

Error metric.  max|out - ref| / max|ref| says nothing for a constant vector: G 1 cancels to rounding
level, so max|ref| is itself rounding-sized.  scaled_error() measures against the amplification
    scale_i = (1/M) sum_v g^_vi (sum_j g^_vj) max|b|,    g^ = (code + 2 af) inv  (0 for missing),
the sum of the magnitudes of every term of out_i, which bounds the plain form and the split
l0 + code * inv of the HIP kernels alike, in units of 2^-53.
"""
import functools
from collections import namedtuple

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than double here: the reference would prove nothing"

U = 2.0 ** -53

# Largest scaled error of the double-precision oracle (grm_oracle.c) against reference() over CASES x
# VECTOR_KINDS, in units of 2^-53: measured 9.7395 (N = 20000, M = 40, 30 % missing, the all-ones vector,
# whose 20000-term sequential dot products cancel; 0.58 for the same shape at 0.5 % missing, 0.48 for
# +-1, at most 0.27 for every other kind), rounded up.  test_grm_ref.py re-measures it and asserts that
# it is not exceeded; the GPU operator must stay within 4 E_ORC (test_gpu_grm_edges.py).
E_ORC = 9.74

SHAPES = [(5, 3), (16, 64), (17, 65), (255, 257), (256, 256), (257, 255), (511, 513), (512, 512), (513, 511),
          (1025, 33), (20000, 40), (40, 20000)]
MISS = (5e-3, 0.3)
CASES = [(n, m, miss) for n, m in SHAPES for miss in MISS]

VECTOR_KINDS = ("normal", "ones", "pm1", "wide", "tiny", "huge", "onehot")
CONSTANT_KINDS = ("ones",)     # max|ref| is rounding-sized: the 1e-11 max|ref| bound is vacuous for these


def case_id(c):
    return "n%d-m%d-miss%g" % c


def case_seed(n, m, miss):
    return 7919 * n + 104729 * m + int(round(1000 * miss))


def make_codes(n, m, seed, miss, maf_log10=(-2.0, np.log10(0.5)), flip_frac=0.2):
    """[m, n] uint8 codes 0..3 (3 = missing): log-uniform MAF, flip_frac of the markers counted on the
    major allele, missing at rate miss.  Planted where the shape allows (one ordinary marker is always left):
    an all-missing marker (row m - 1), a monomorphic one (row 0), one with 60 % missing, one whose only
    missing code is sample n - 1, a singleton; and sample n - 1 missing at every marker (n >= 2)."""
    rng = np.random.default_rng([seed, n, m])
    maf = 10.0 ** rng.uniform(maf_log10[0], maf_log10[1], m)
    af = np.where(rng.random(m) < flip_frac, 1 - maf, maf)
    codes = rng.binomial(2, af[:, None], size=(m, n)).astype(np.uint8)
    codes[rng.random((m, n)) < miss] = 3
    rows = []
    for r in (m - 1, 0, m // 2, m // 4, (3 * m) // 4):
        if r not in rows:
            rows.append(r)
    rows = rows[:max(0, min(5, m - 1))]
    for kind, r in zip(("allmiss", "mono", "miss60", "lastonly", "singleton"), rows):
        if kind == "allmiss":
            codes[r] = 3
        elif kind == "mono":
            codes[r] = 0
        elif kind == "miss60":
            codes[r] = rng.binomial(2, 0.3, n)
            codes[r, rng.permutation(n)[: (3 * n + 4) // 5]] = 3
        elif kind == "lastonly":
            codes[r] = rng.binomial(2, 0.25, n)
            codes[r, n - 1] = 3
        else:
            codes[r] = 0
            codes[r, (n // 2) if n // 2 != n - 1 else 0] = 1
    if n >= 2:
        codes[:, n - 1] = 3
    return codes


def pack(codes, stride=None, pad=0):
    """2-bit rows, code of sample s in bits 2 (s % 4) .. of byte s // 4; stride >= ceil(n / 4) bytes per
    marker.  The unused bit pairs of the last byte and every byte beyond it come from the byte pad
    (0xFF: all ones, i.e. stray 'missing' codes that must not count)."""
    codes = np.asarray(codes, dtype=np.uint8)
    m, n = codes.shape
    nb = (n + 3) // 4
    stride = nb if stride is None else int(stride)
    assert stride >= nb and 0 <= pad <= 0xFF
    c = np.empty((m, 4 * nb), dtype=np.uint8)
    c[:, :n] = codes
    for s in range(n, 4 * nb):
        c[:, s] = (pad >> (2 * (s % 4))) & 3
    out = np.full((m, stride), pad, dtype=np.uint8)
    out[:, :nb] = c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6)
    return out


def marker_stats(codes):
    """af, inv in double, exactly as saige_fitnull.cpp:181-203: sum / (2 nvalid), 1 / sqrt(2 af (1 - af)),
    both 0 where either is not finite."""
    codes = np.asarray(codes)
    valid = codes != 3
    nvalid = valid.sum(axis=1).astype(np.int64)
    s = np.where(valid, codes, 0).sum(axis=1, dtype=np.int64)
    with np.errstate(all="ignore"):
        af = s.astype(np.float64) / (2 * nvalid).astype(np.float64)
        inv = 1 / np.sqrt(2 * af * (1 - af))
    bad = ~np.isfinite(af) | ~np.isfinite(inv)
    af[bad] = 0
    inv[bad] = 0
    return af, inv


Ref = namedtuple("Ref", "out diag scale")


def reference(codes, B):
    """B: [n] or [k, n].  -> Ref(out, diag [n], scale), out and scale shaped like B, all np.longdouble."""
    codes = np.asarray(codes)
    m, n = codes.shape
    B = np.asarray(B, dtype=np.float64)
    one = B.ndim == 1
    B2 = np.atleast_2d(B).astype(LD)
    af, inv = marker_stats(codes)
    valid = codes != 3
    c = codes.astype(LD)
    af2, invl = 2 * af.astype(LD)[:, None], inv.astype(LD)[:, None]
    g = np.where(valid, (c - af2) * invl, LD(0))
    gh = np.where(valid, (c + af2) * invl, LD(0))
    out = (g.T @ (g @ B2.T)).T / LD(m)
    diag = (g * g).sum(axis=0) / LD(m)
    amp = (gh * gh.sum(axis=1)[:, None]).sum(axis=0) / LD(m)
    with np.errstate(invalid="ignore"):
        scale = amp[None, :] * np.max(np.abs(B2), axis=1)[:, None]
    return Ref(out[0], diag, scale[0]) if one else Ref(out, diag, scale)


def scaled_error(out, ref, scale):
    """max_i |out_i - ref_i| / scale_i over scale_i > 0, in units of 2^-53; where scale_i == 0 (no term
    of out_i is non-zero) both values must be exactly 0.  inf if out is not finite."""
    out, ref, scale = np.asarray(out, dtype=LD), np.asarray(ref, dtype=LD), np.asarray(scale, dtype=LD)
    assert out.shape == ref.shape == scale.shape
    pos = scale > 0
    assert np.all(ref[~pos] == 0), "reference not 0 where its amplification is 0"
    assert np.all(out[~pos] == 0), "result not exactly 0 at %s, where every term is 0" % np.flatnonzero(~pos & (out != 0))[:8]
    if not np.all(np.isfinite(out)):
        return float("inf")
    if not pos.any():
        return 0.0
    return float(np.max(np.abs(out - ref)[pos] / scale[pos]) / LD(U))


def vectors(n, seed):
    """[len(VECTOR_KINDS), n] float64, rows in the order of VECTOR_KINDS."""
    rng = np.random.default_rng([seed, n, 17])
    B = np.zeros((len(VECTOR_KINDS), n))
    B[0] = rng.standard_normal(n)
    B[1] = 1.0
    B[2] = 2.0 * rng.integers(0, 2, n) - 1            # Hutchinson (saige_fitnull.cpp:649)
    B[3] = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
    B[4] = rng.standard_normal(n) * 1e-300
    B[5] = rng.standard_normal(n) * (1e300 / n)
    B[6, n // 2] = -2.5
    return B


Case = namedtuple("Case", "n m miss codes B ref")


@functools.lru_cache(maxsize=None)
def case(n, m, miss):
    """Codes, vectors and their reference of one row of CASES: computed once, shared, read-only."""
    seed = case_seed(n, m, miss)
    codes = make_codes(n, m, seed, miss)
    B = vectors(n, seed)
    ref = reference(codes, B)
    for a in (codes, B) + tuple(ref):
        a.setflags(write=False)
    return Case(n, m, miss, codes, B, ref)


# ---- PCG_diag_sigma inputs (test_grm_ref.py conditions them, test_gpu_grm_edges.py solves them)
PCG_SHAPES = [(257, 255), (1025, 33)]
PCG_TOL, PCG_MAXITER = 1e-5, 500
PCG_TAUS = ([1.0, 0.33], [0.97, 2.5],
            [1e-6, 0.0],       # tau0 / w < 1e-4 for every sample: minv = 1e4 everywhere (get_diag_sigma's clamp)
            [2e-5, 0.0])       # clamps where w > 0.2 only
PCG_RHS = ("normal", "ones", "age")
PCG_SEED = {(257, 255): 3, (1025, 33): 3}


def pcg_inputs(n, m):
    """-> codes, w [n], B [3, n] (rows: PCG_RHS).  w = mu (1 - mu), mu ~ U(0.02, 0.4): 0.02 .. 0.24."""
    codes = make_codes(n, m, case_seed(n, m, 5e-3), 5e-3)
    rng = np.random.default_rng([PCG_SEED[(n, m)], n, 23])
    mu = rng.uniform(0.02, 0.4, n)
    w = mu * (1 - mu)
    B = np.empty((3, n))
    B[0] = rng.standard_normal(n)
    B[1] = 1.0
    age = rng.normal(50.0, 10.0, n)
    B[2] = age - age.mean()
    return codes, w, B
