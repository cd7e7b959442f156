"""Reference of KING-robust kinship for the CPU and GPU tests; it shares nothing with the kernel.

The 2-bit rows are unpacked, one-hot indicator matrices of the codes are built, the five counts of every pair come
from matrix products of those 0 / 1 matrices, and kinship / IBS0 are the two expressions of the definition,
elementwise in numpy float64.  The products run in float64 and are turned into int64: every partial sum is an integer
of at most M < 2^53, so they are exact in any order (numpy's int64 ``@`` has no BLAS and takes minutes at the sizes
used here; test_king_ref.py checks the two against each other).  Also: planted pedigrees in two Balding-Nichols
populations, and the numpy stand-in operator the driver's CPU tests inject.  No test functions here."""
import functools
from collections import namedtuple

import numpy as np

import grm_ref as R

FST = 0.1
MISS = 0.01
CUT = 2.0 ** -4.5
EDGES = (2.0 ** -1.5, 2.0 ** -2.5, 2.0 ** -3.5, 2.0 ** -4.5)
MARGIN = 0.01                 # every planted and unplanted kinship of PEDIGREES is at least this far from a band edge
# (N, M) -> seed of the planted pedigrees the GPU tests use; test_king_ref.py asserts MARGIN for each
PEDIGREES = {(257, 20000): 1, (600, 20000): 1}
FILTER = dict(maf=0.0, missing_rate=1.0)     # the marker filter of the driver calls: every marker passes


def unpack(packed, n):
    """[m, stride] uint8 2-bit rows -> codes [m, n] uint8 (sample s in bits 2 (s % 4) .. of byte s // 4)."""
    p = np.asarray(packed, dtype=np.uint8)
    out = np.empty((p.shape[0], 4 * p.shape[1]), dtype=np.uint8)
    for k in range(4):
        out[:, k::4] = (p >> (2 * k)) & 3
    return out[:, :n]


def counts(codes):
    """codes [m, n] -> int64 [5, n, n]: nn, hi, hj, hh, ibs0 of every ordered pair (i, j)."""
    c = np.asarray(codes)
    one = [(c == k).astype(np.int64).astype(np.float64) for k in range(3)]   # one-hot: code 0, 1, 2
    called = one[0] + one[1] + one[2]

    def dot(a, b):
        return np.rint(a.T @ b).astype(np.int64)

    nn, hi, hj, hh = dot(called, called), dot(one[1], called), dot(called, one[1]), dot(one[1], one[1])
    ibs0 = dot(one[0], one[2]) + dot(one[2], one[0])
    return np.stack([nn, hi, hj, hh, ibs0])


def counts_int(codes):
    """The same by numpy's int64 ``@`` (small inputs only)."""
    c = np.asarray(codes)
    one = [(c == k).astype(np.int64) for k in range(3)]
    called = one[0] + one[1] + one[2]
    return np.stack([called.T @ called, one[1].T @ called, called.T @ one[1], one[1].T @ one[1],
                     one[0].T @ one[2] + one[2].T @ one[0]])


def values(cnt):
    """The five counts [5, ...] -> (kinship, IBS0) in float64, NaN where undefined."""
    nn, hi, hj, hh, ibs0 = (np.asarray(cnt[k], dtype=np.int64) for k in range(5))
    D = (hi + hj - 2 * hh) + 4 * ibs0
    mn = np.minimum(hi, hj)
    with np.errstate(invalid="ignore", divide="ignore"):
        kin = np.where(mn > 0, 0.5 - D.astype(np.float64) / (4.0 * mn.astype(np.float64)), np.nan)
        ibs = np.where(nn > 0, ibs0.astype(np.float64) / nn.astype(np.float64), np.nan)
    return kin, ibs


def pairs(cnt, cutoff):
    """Related at cutoff: i < j, mn > 0, kinship >= cutoff -> (i, j, kinship, IBS0, counts [pairs, 5]) sorted by (i, j)."""
    kin, ibs = values(cnt)
    n = kin.shape[0]
    i, j = np.triu_indices(n, 1)
    with np.errstate(invalid="ignore"):
        keep = (np.minimum(cnt[1], cnt[2])[i, j] > 0) & (kin[i, j] >= cutoff)
    i, j = i[keep], j[keep]
    return i.astype(np.int32), j.astype(np.int32), kin[i, j], ibs[i, j], cnt[:, i, j].T.astype(np.int32)


def band(kin):
    """KING's inference band: 0 duplicate / MZ, 1, 2, 3, -1 below 2^-4.5 (or NaN)."""
    k = np.asarray(kin, dtype=np.float64)
    out = np.full(k.shape, -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for d in (3, 2, 1, 0):
            out[k > EDGES[d]] = d
    return out


# ---- planted pedigrees
Pedigree = namedtuple("Pedigree", "codes pop planted")     # planted: {(i, j) with i < j: degree 0 .. 3}


def _child(rng, codes, a, b):
    def half(g):
        t = (g == 2).astype(np.uint8)
        het = g == 1
        t[het] = rng.integers(0, 2, int(het.sum()), dtype=np.uint8)
        return t
    return half(codes[:, a]) + half(codes[:, b])


def pedigree(n, m, seed):
    """[m, n] codes: samples 0 .. n/2 - 1 from population 0, the others from population 1 (Balding-Nichols, F_ST = FST,
    ancestral frequencies U(0.1, 0.9)); in each population one extended family is planted by gene dropping over
    unlinked markers, in the population's first 13 samples f .. f + 12:
        f + 0, f + 1 founders (a couple), f + 2, f + 3 their children (full sibs), f + 4, f + 5 the children's mates
        (founders), f + 6 child of (f + 2, f + 4), f + 7 child of (f + 3, f + 5): first cousins; f + 8 a founder with
        two mates f + 9, f + 10 and the half sibs f + 11 (f + 8, f + 9), f + 12 (f + 8, f + 10).
    In population 0 sample f + 13 is a duplicate of f + 14.  Then every entry is missing at rate MISS."""
    assert n >= 40
    rng = np.random.default_rng([seed, n, m, 77])
    anc = rng.uniform(0.1, 0.9, m)
    a = (1 - FST) / FST
    freq = rng.beta(anc[:, None] * a, (1 - anc[:, None]) * a, size=(m, 2))
    pop = (np.arange(n) >= n // 2).astype(np.int64)
    codes = rng.binomial(2, freq[:, pop]).astype(np.uint8)
    planted = {}

    def put(i, j, d):
        planted[(min(i, j), max(i, j))] = d

    for f in (0, n // 2):
        for kid, pa, pb in ((f + 2, f, f + 1), (f + 3, f, f + 1), (f + 6, f + 2, f + 4), (f + 7, f + 3, f + 5),
                            (f + 11, f + 8, f + 9), (f + 12, f + 8, f + 10)):
            codes[:, kid] = _child(rng, codes, pa, pb)
            put(kid, pa, 1)
            put(kid, pb, 1)
        put(f + 2, f + 3, 1)                               # full sibs
        put(f + 11, f + 12, 2)                             # half sibs
        for g, uncle in ((f + 6, f + 3), (f + 7, f + 2)):
            put(g, uncle, 2)                               # avuncular
            put(g, f, 2)                                   # grandparents
            put(g, f + 1, 2)
        put(f + 6, f + 7, 3)                               # first cousins
    codes[:, 13] = codes[:, 14]
    put(13, 14, 0)
    codes[rng.random((m, n)) < MISS] = 3
    codes.setflags(write=False)
    return Pedigree(codes, pop, planted)


@functools.lru_cache(maxsize=None)
def planted(n, m):
    """(Pedigree, counts int64 [5, n, n]) of one of PEDIGREES, computed once, read-only."""
    p = pedigree(n, m, PEDIGREES[(n, m)])
    c = counts(p.codes)
    c.setflags(write=False)
    return p, c


def source(codes, prefix="s"):
    """An in-memory GenotypeSource of 2-bit rows."""
    from saigegds_amd.assoc import GenotypeSource
    return GenotypeSource([f"{prefix}{i}" for i in range(codes.shape[1])], packed=R.pack(codes))


# ---- numpy stand-in of the operator (host logic of seqFitKING without a GPU)
class NumpyKing:
    def __init__(self, packed, n_samp):
        self.n = int(n_samp)
        self.m = int(np.asarray(packed).shape[0])
        self.cnt = counts(unpack(packed, self.n))

    def king_counts(self, i0, ni, j0, nj):
        return self.cnt[:, i0:i0 + ni, j0:j0 + nj].astype(np.int32)

    def king_pairs(self, cutoff):
        return pairs(self.cnt, cutoff)

    def close(self):
        pass
