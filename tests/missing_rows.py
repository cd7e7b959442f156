"""Rows with a prescribed number of missing genotypes per (variant, sample range).

The two-plane form of the score stage lists the missing genotypes of every (variant, sample range) segment.  A
segment with more than LT_CAP = 256 of them (row-major calls, S3_LT_CAP in kern_lists.h), or one that finds its
sub-pool full (resident blocks), is not listed: the variant leaves the fixed-point path for the FP64 kernel and is
counted in stats["n_unlisted"].  The builders here put the missing genotypes of a segment exactly where a test wants
them -- spread out, in one run, against the start or the end of a range, in the last partial piece before sample N --
and say which variants must take that route.

Sample ranges as s3_layout.h derives them: ntile = 2 ceil(N / 512) tiles of 256 samples, nr = clamp((64 ntile + 8191)
// 8192, 1, 16) ranges, range g = tiles [g ntile // nr, (g + 1) ntile // nr), clipped to N.
"""
import numpy as np

from saigegds_amd.gds import pack_dosage_2bit

LT_CAP = 256           # S3_LT_CAP: listed entries of one segment of a row-major call
MISSING = 3


def layout(n):
    """-> (ntile, nr) of the list kernels for N = n samples."""
    ntile = 2 * ((n + 511) // 512)
    nr = min(max((64 * ntile + 8191) // 8192, 1), 16)
    return ntile, nr


def ranges(n):
    """-> [(s0, s1)] sample ranges of the lists, s1 clipped to n."""
    ntile, nr = layout(n)
    return [(min(n, 256 * (g * ntile // nr)), min(n, 256 * ((g + 1) * ntile // nr))) for g in range(nr)]


def block_subcap(n, m):
    """Entries of one sub-pool of a resident block of m variants of n samples (host_blocks.h block_idx_cap,
    kern_lists.h s3_lists_setup with full_wg = the workgroups of a full load, four segments each)."""
    _, nr = layout(n)
    idx_cap = min(max(m * max(64, n // 128), 1024 * 256), 0xF0000000)
    full_wg = (m * nr + 3) // 4
    nsub = 1
    while nsub * 2 <= 1024 and nsub * 2 <= full_wg:
        nsub *= 2
    return idx_cap // nsub


def base_codes(rng, m, n, af):
    """[m, n] called genotypes (0, 1, 2), alt allele frequency af[j] (Hardy-Weinberg), nothing missing."""
    af = np.broadcast_to(np.asarray(af, dtype=np.float64), (m,))
    codes = (rng.random((m, n)) < af[:, None]).astype(np.uint8)
    codes += (rng.random((m, n)) < af[:, None]).astype(np.uint8)
    return codes


def sprinkle(rng, codes, rate, rows=None):
    """Each genotype of the rows (default: all) missing with probability rate (a row's own rate if an array)."""
    rows = np.arange(codes.shape[0]) if rows is None else np.asarray(rows)
    rate = np.broadcast_to(np.asarray(rate, dtype=np.float64), (rows.size,))
    for r, p in zip(rows, rate):
        codes[r, rng.random(codes.shape[1]) < p] = MISSING


def positions(s0, s1, count, where, offset=0):
    """count sample indices in [s0, s1): 'spread' (evenly), 'start', 'end' (up against s1 - 1), 'run' (contiguous
    from s0 + offset)."""
    span = s1 - s0
    if count > span:
        raise ValueError(f"{count} missing genotypes do not fit a range of {span} samples")
    if where == "spread":
        return s0 + (np.arange(count, dtype=np.int64) * span) // count
    if where == "start":
        return np.arange(s0, s0 + count)
    if where == "end":
        return np.arange(s1 - count, s1)
    if where == "run":
        if offset + count > span:
            raise ValueError("run leaves the range")
        return np.arange(s0 + offset, s0 + offset + count)
    raise ValueError(where)


def set_segment(rng, codes, v, g, count, where, offset=0):
    """Range g of variant v gets exactly `count` missing genotypes at `where`; missing genotypes it held before
    elsewhere in the range become called genotypes (drawn at the row's allele frequency)."""
    n = codes.shape[1]
    s0, s1 = ranges(n)[g]
    seg = codes[v, s0:s1]
    called = seg[seg != MISSING]
    p = called.mean() / 2 if called.size else 0.0
    was = seg == MISSING
    seg[was] = (rng.random(int(was.sum())) < p).astype(np.uint8) + (rng.random(int(was.sum())) < p).astype(np.uint8)
    codes[v, positions(s0, s1, count, where, offset)] = MISSING


def segment_counts(codes):
    """[m, nr] missing genotypes per (variant, range)."""
    return np.stack([(codes[:, s0:s1] == MISSING).sum(1) for s0, s1 in ranges(codes.shape[1])], axis=1)


def expected_unlisted(codes):
    """Variants of a row-major two-plane call whose missing genotypes are not listed: some segment > LT_CAP."""
    return set(np.flatnonzero((segment_counts(codes) > LT_CAP).any(1)).tolist())


def pack(codes, pad3=False):
    """2-bit rows of pack_dosage_2bit; pad3: the unused slots of the last byte (samples N .. 4 ceil(N / 4) - 1)
    hold code 3, which the library must ignore."""
    packed = pack_dosage_2bit(codes)
    n = codes.shape[1]
    if pad3 and n % 4:
        fill = 0
        for k in range(n % 4, 4):
            fill |= MISSING << (2 * k)
        packed[:, -1] |= np.uint8(fill)
    return packed
