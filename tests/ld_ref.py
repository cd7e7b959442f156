"""The reference of the LD tests, sharing nothing with the kernel or the driver: the six sums of a pair
from unpacked codes in int64 numpy, the decision in the double expression and exactly (Python integers and
``Fraction(t2)``), the one-candidate-at-a-time greedy rule, and an engine in numpy for the driver's host logic."""
from fractions import Fraction

import numpy as np


def unpack(packed, n):
    """[m, >= ceil(n/4)] packed rows -> [m, n] codes; nothing at or beyond sample n is looked at."""
    p = np.asarray(packed, dtype=np.uint8)[:, :(n + 3) // 4]
    c = np.stack([(p >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(p.shape[0], -1)
    return c[:, :n]


def pack(codes):
    c = np.asarray(codes, dtype=np.uint8)
    m, n = c.shape
    c = np.concatenate([c, np.zeros((m, (-n) % 4), np.uint8)], axis=1).reshape(m, -1, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)


def counts(ca, cb):
    """codes [ma, n], [mb, n] -> int64 [ma, mb, 6] = (n, sx, sy, sxx, syy, sxy) over the samples called in both."""
    ca, cb = np.asarray(ca).astype(np.int64), np.asarray(cb).astype(np.int64)
    pa, pb = (ca != 3).astype(np.int64), (cb != 3).astype(np.int64)
    xa, xb = ca * pa, cb * pb
    out = np.empty((ca.shape[0], cb.shape[0], 6), dtype=np.int64)
    out[..., 0] = pa @ pb.T
    out[..., 1] = xa @ pb.T
    out[..., 2] = pa @ xb.T
    out[..., 3] = (xa * xa) @ pb.T
    out[..., 4] = pa @ (xb * xb).T
    out[..., 5] = xa @ xb.T
    return out


def cvv(s):
    s = np.asarray(s).astype(np.int64)
    n, sx, sy, sxx, syy, sxy = (s[..., k] for k in range(6))
    return n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy


def in_ld(s, t2):
    """The decision as the kernel states it: doubles of the exact int64 c, vx, vy, three products, strict >."""
    c, vx, vy = cvv(s)
    cd = c.astype(np.float64)
    return (vx > 0) & (vy > 0) & (cd * cd > np.float64(t2) * (vx.astype(np.float64) * vy.astype(np.float64)))


def in_ld_exact(s, t2):
    """The same decision with no rounding at all: Python integers against the exact rational value of the double t2."""
    c, vx, vy = cvv(s)
    T = Fraction(float(t2))
    out = np.zeros(c.shape, dtype=bool)
    for k in np.ndindex(c.shape):
        C, X, Y = int(c[k]), int(vx[k]), int(vy[k])
        out[k] = X > 0 and Y > 0 and Fraction(C * C) > T * X * Y
    return out


def min_rel_gap(s, t2):
    """The smallest |c^2 / (vx vy) - t2| / t2 over the pairs with vx, vy > 0 (inf: none): the condition on test inputs
    under which the double and the exact decision must agree."""
    c, vx, vy = cvv(s)
    T, best = Fraction(float(t2)), float("inf")
    live = (vx > 0) & (vy > 0)
    if T <= 0 or not live.any():
        return best
    # in double first (a few ulp off the true ratio): only what comes within 1e-6 there is worth the exact arithmetic
    with np.errstate(invalid="ignore", divide="ignore"):
        approx = np.abs(c.astype(np.float64) ** 2 / (vx.astype(np.float64) * vy.astype(np.float64)) - float(t2)) / float(t2)
    far = live & (approx >= 1e-6)
    if far.any():
        best = float(approx[far].min())
    for k in zip(*np.nonzero(live & ~far)):
        best = min(best, float(abs(Fraction(int(c[k]) ** 2, int(vx[k]) * int(vy[k])) - T) / T))
    return best


def marker_ok(codes, maf, missing_rate):
    """The candidates' filter, stated on codes: min(af, 1 - af) >= maf, missing fraction <= missing_rate, not monomorphic."""
    codes = np.asarray(codes)
    n = codes.shape[1]
    valid = codes != 3
    nv = valid.sum(axis=1)
    ac = np.where(valid, codes, 0).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        af = ac / (2.0 * nv)
    return (np.minimum(af, 1 - af) >= maf) & ((n - nv) / n <= missing_rate) & (ac > 0) & (ac < 2 * nv)


def prune_ref(codes, chrom, pos, ids, t, maf, missing_rate, slide_max_bp, slide_max_n=None, autosome_only=True,
              candidates=None):
    """The sequential definition: per run of a chromosome name, candidates in file order, one at a time, each against
    every kept variant of the run within slide_max_bp (the last slide_max_n of them) -> {chromosome: [ids]}."""
    t2 = float(t) * float(t)
    ok = marker_ok(codes, maf, missing_rate)
    if candidates is not None:
        ok &= np.isin(ids, list(candidates))
    out = {}
    kept = []                                          # (row index) of the current run
    for i in range(len(chrom)):
        if i == 0 or chrom[i] != chrom[i - 1]:
            kept = []
        name = str(chrom[i])
        digits = name[3:] if name.lower().startswith("chr") else name
        if autosome_only and not (digits.isdigit() and 1 <= int(digits) <= 22):
            continue
        out.setdefault(name, [])
        if not ok[i]:
            continue
        against = [k for k in kept if pos[i] - pos[k] <= slide_max_bp]
        if slide_max_n is not None:
            against = [k for k in against if k in kept[-slide_max_n:]]
        if against and in_ld(counts(codes[i:i + 1], codes[against]), t2).any():
            continue
        kept.append(i)
        out[name].append(ids[i])
    return out


class NumpyLdEngine:
    """What ``_lib.LdEngine`` answers, in numpy: block flags [mb, W + mb] (window rows oldest first, then the block's
    own rows, of which only j < i is filled), push, reset, window_len.  ``max_rows``: the budget, as rows."""

    def __init__(self, n_samp, bytes_per_variant, max_rows=None):
        self.n, self.bpv, self.max_rows = int(n_samp), int(bytes_per_variant), max_rows
        self.win = np.zeros((0, self.n), dtype=np.uint8)
        self.blk = None
        self.calls = 0

    @property
    def window_len(self):
        return self.win.shape[0]

    def block(self, rows, t2):
        rows = np.asarray(rows, dtype=np.uint8)
        assert rows.ndim == 2 and rows.shape[1] == self.bpv and 1 <= rows.shape[0] <= 256
        self.blk = unpack(rows, self.n)
        self.calls += 1
        mb, W = self.blk.shape[0], self.win.shape[0]
        flags = np.zeros((mb, W + mb), dtype=np.uint8)
        if W:
            flags[:, :W] = in_ld(counts(self.blk, self.win), t2)
        flags[:, W:] = np.tril(in_ld(counts(self.blk, self.blk), t2), -1)
        return flags

    def push(self, keep_idx, drop_oldest=0):
        idx = np.asarray(keep_idx, dtype=np.int64).reshape(-1)
        assert 0 <= drop_oldest <= self.win.shape[0] and (np.diff(idx) > 0).all()
        assert idx.size == 0 or (0 <= idx[0] and idx[-1] < self.blk.shape[0])
        if self.max_rows is not None and self.win.shape[0] - drop_oldest + idx.size > self.max_rows:
            raise MemoryError("window over the budget")
        self.win = np.concatenate([self.win[drop_oldest:], self.blk[idx]])

    def reset(self):
        self.win = self.win[:0]

    def close(self):
        pass
