"""Long-double reference of the explicit GRM K = G'G/M (sgx_grm_dense / sgx_grm_sparse), the planted relatives
and the numpy stand-in operator that the CPU and GPU tests share.  No test functions here.

K_ij = (1/M) sum_v g_vi g_vj with g = (code - 2 af) inv, 0 for a missing code; af and inv in double
(grm_ref.marker_stats: they are part of the definition), the rest in np.longdouble.  The long-double Gram sum is
evaluated exactly: g is cut into four fixed-point pieces of at most 18 bits, the pieces' Gram products are float64
matrix products without rounding (36-bit products, 2^14 markers per block), and the blocks are added in long
double.  The piece pairs left out (p + q >= 7) are below 2^-75 of the largest |g|^2.

Error metric: |K - ref| against the amplification scale_ij = (1/M) sum_v g^_vi g^_vj, g^ = (code + 2 af) inv,
the sum of the magnitudes of every term (and of the split l0 + code inv of the kernels), in units of 2^-53.
"""
import functools
from collections import namedtuple

import numpy as np

import grm_ref as R

LD = np.longdouble

# Largest scaled error of a plain float64 g.T @ g / M against reference() over CASES and PLANTED, in units of
# 2^-53: measured 3.359 (N = 1025, M = 33, 30 % missing; at most 0.68 elsewhere) by test_grm_dense_ref.py, which
# asserts that it is not exceeded; rounded up.  The GPU kernel must
# stay within 4 E_DENSE: one more rounding per entry for its fma(code, inv, l0), a different summation order, the
# slab additions and the division.
E_DENSE = 3.36

SHAPES = [(5, 3), (17, 65), (255, 257), (257, 255), (513, 511), (1025, 33), (40, 20000), (300, 140000)]
CASES = [(n, m, miss) for n, m in SHAPES for miss in R.MISS]
PLANTED = [(257, 2048), (1025, 2048)]
CUTOFFS = (0.125, 0.25, 0.4)
EVERYTHING = -1e300
_BLOCK = 1 << 14


def _g(codes, sign):
    af, inv = R.marker_stats(codes)
    c = codes.astype(LD)
    return np.where(codes != 3, (c + sign * 2 * af.astype(LD)[:, None]) * inv.astype(LD)[:, None], LD(0))


def _gram_exact(g):
    """g' g of a long-double [m, n] matrix -> [n, n] long double (see the module docstring)."""
    m, n = g.shape
    out = np.zeros((n, n), dtype=LD)
    gmax = float(np.max(np.abs(g))) if g.size else 0.0
    if gmax == 0:
        return out
    e0 = int(np.ceil(np.log2(gmax))) + 1
    for b0 in range(0, m, _BLOCK):
        r = g[b0:b0 + _BLOCK].copy()
        pieces = []
        for k in range(1, 5):
            q = LD(2.0) ** (17 * k - e0)
            p = np.rint(r * q) / q
            r = r - p
            pieces.append(p.astype(np.float64))
        for p in range(4):
            for q in range(p, 4):
                if p + q + 2 >= 7:
                    continue
                t = (pieces[p].T @ pieces[q]).astype(LD)
                out += t if p == q else t + t.T
    return out


Ref = namedtuple("Ref", "K scale")


def reference(codes):
    """-> Ref(K, scale), both [n, n] np.longdouble."""
    codes = np.asarray(codes)
    m = codes.shape[0]
    gh = _g(codes, +1).astype(np.float64)                   # (a yardstick, not a value: double is enough, and 0 stays 0)
    return Ref(_gram_exact(_g(codes, -1)) / LD(m), ((gh.T @ gh) / m).astype(LD))


def scaled_error(K, ref):
    return R.scaled_error(np.asarray(K), ref.K, ref.scale)


def double_gram(codes):
    """The plain float64 evaluation: g in double as (code - 2 af) inv, g.T @ g / M."""
    af, inv = R.marker_stats(codes)
    g = np.where(codes != 3, (codes.astype(np.float64) - 2 * af[:, None]) * inv[:, None], 0.0)
    return (g.T @ g) / codes.shape[0]


# ---- planted relatives
Planted = namedtuple("Planted", "codes dup parent_child sibs disjoint")


def _transmit(rng, gcol):
    """One allele of a genotype column (0 / 1 / 2; 3 stays 3)."""
    t = np.where(gcol == 2, 1, 0).astype(np.uint8)
    het = gcol == 1
    t[het] = rng.integers(0, 2, int(het.sum()), dtype=np.uint8)
    t[gcol == 3] = 3
    return t


def plant_relatives(n, m, seed, miss=5e-3):
    """grm_ref.make_codes plus: a duplicate pair, two children of the same two parents by gene dropping (two
    parent-child pairs per child, one sibling pair), and a pair of samples missing at disjoint halves of the markers
    (K exactly 0).  A child is missing where a parent is."""
    codes = R.make_codes(n, m, seed, miss).copy()
    rng = np.random.default_rng([seed, n, m, 99])
    dup = (3, n - 57)
    pa, pb = 10, 50
    kids = (n // 2 + 2, n - 2)
    dis = (20, n - 17)
    assert len({*dup, pa, pb, *kids, *dis, n - 1, n // 2}) == 10
    codes[:, dup[1]] = codes[:, dup[0]]
    for k in kids:
        ta, tb = _transmit(rng, codes[:, pa]), _transmit(rng, codes[:, pb])
        codes[:, k] = np.where((ta == 3) | (tb == 3), 3, (ta + tb) & 3)
    codes[: m // 2, dis[0]] = 3
    codes[m // 2:, dis[1]] = 3
    codes.setflags(write=False)
    return Planted(codes, dup, [(pa, kids[0]), (pb, kids[0]), (pa, kids[1]), (pb, kids[1])], kids, dis)


PLANT_SEED = {(257, 2048): 11, (1025, 2048): 11}


@functools.lru_cache(maxsize=None)
def planted(n, m):
    p = plant_relatives(n, m, PLANT_SEED[(n, m)])
    ref = reference(p.codes)
    for a in ref:
        a.setflags(write=False)
    return p, ref


@functools.lru_cache(maxsize=None)
def case(n, m, miss):
    """(codes, Ref) of one row of CASES: grm_ref's codes, computed once, read-only."""
    codes = R.case(n, m, miss).codes if (n, m, miss) in R.CASES else R.make_codes(n, m, R.case_seed(n, m, miss), miss)
    codes.setflags(write=False)
    ref = reference(codes)
    for a in ref:
        a.setflags(write=False)
    return codes, ref


def threshold(K, cutoff):
    """{(i, j): K_ij} of i <= j with K_ij >= cutoff or i == j -> (i, j, x) sorted by (i, j)."""
    K = np.asarray(K)
    i, j = np.triu_indices(K.shape[0])
    keep = (K[i, j] >= cutoff) | (i == j)
    return i[keep].astype(np.int32), j[keep].astype(np.int32), K[i, j][keep]


# ---- numpy stand-in of the operator (host logic of seqFitDenseGRM / seqFitSparseGRM without a GPU)
class NumpyGrm:
    def __init__(self, packed, n_samp):
        from saigegds_amd.gds import unpack_dosage_2bit
        self.n = int(n_samp)
        self.packed = np.asarray(packed)
        self.m = int(self.packed.shape[0])
        self.K = double_gram(unpack_dosage_2bit(self.packed, self.n))

    def dense_block(self, i0, ni, j0, nj):
        return self.K[i0:i0 + ni, j0:j0 + nj].copy()

    def dense(self):
        return self.K.copy()

    def sparse(self, cutoff):
        return threshold(self.K, cutoff)

    def diag(self):
        return np.diag(self.K).copy()

    def close(self):
        pass
