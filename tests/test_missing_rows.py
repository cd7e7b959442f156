"""The row builders of missing_rows.py (no GPU): the sample ranges of the list kernels, the segment counts the
builders make, and expected_unlisted against a count that finds each sample's range by brute force."""
import numpy as np
import pytest

import missing_rows as mr
from saigegds_amd.gds import unpack_dosage_2bit


@pytest.mark.parametrize("n,nr,sizes", [(3001, 1, {3001}), (50_000, 2, {25_088, 24_912}),
                                        (430_000, 14, {30_720, 30_640}), (540_001, 16, {33_536, 33_792, 33_633})])
def test_range_layout(n, nr, sizes):
    rg = mr.ranges(n)
    assert len(rg) == nr == mr.layout(n)[1]
    assert rg[0][0] == 0 and rg[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(rg, rg[1:]))
    lens = [s1 - s0 for s0, s1 in rg]
    if sizes is not None:
        assert set(lens) == sizes, lens
    if n == 430_000:
        assert lens[:-1] == [30_720] * 13 and lens[-1] == 30_640      # 14 x 120 tiles, the last clipped at N
    if n == 540_001:
        # 2110 tiles over 16 ranges of 131 or 132 tiles, the last (132 tiles) clipped at N: every range is longer
        # than the 8 x 64 pieces of 64 samples a wave of the list kernels holds (their long-range branch)
        assert set(lens[:-1]) == {33_536, 33_792} and lens[-1] == 540_001 - 256 * (15 * 2110 // 16)
        assert min(lens) > 8 * 64 * 64


def _brute_unlisted(codes):
    n = codes.shape[1]
    ntile = 2 * ((n + 511) // 512)
    nr = min(max((64 * ntile + 8191) // 8192, 1), 16)
    first = [g * ntile // nr for g in range(nr)]
    out = set()
    for v in range(codes.shape[0]):
        cnt = [0] * nr
        for i in np.flatnonzero(codes[v] == 3):
            t = i // 256
            g = max(k for k in range(nr) if first[k] <= t)
            cnt[g] += 1
        if max(cnt) > 256:
            out.add(v)
    return out


def test_builders_make_the_counts_asked_for():
    rng = np.random.default_rng(3)
    n = 50_000
    codes = mr.base_codes(rng, 12, n, np.linspace(0.05, 0.8, 12))
    mr.sprinkle(rng, codes, 0.002)
    rg = mr.ranges(n)
    plan = [(0, 0, 255, "spread"), (1, 0, 256, "end"), (2, 0, 257, "start"), (3, 1, 300, "end"),
            (4, 1, 2000, "run"), (5, 0, 256, "end"), (5, 1, 256, "start"), (6, 1, rg[1][1] - rg[1][0], "spread")]
    for v, g, c, where in plan:
        mr.set_segment(rng, codes, v, g, c, where, offset=100)
    cnt = mr.segment_counts(codes)
    for v, g, c, where in plan:
        assert cnt[v, g] == c, (v, g, c, where)
    s0, s1 = rg[0]
    assert (codes[1, s1 - 256:s1] == 3).all() and (codes[2, s0:s0 + 257] == 3).all()
    assert (codes[4, rg[1][0] + 100:rg[1][0] + 2100] == 3).all()
    assert (codes[6, rg[1][0]:] == 3).all()
    assert cnt[5].tolist() == [256, 256]                         # 512 in all, each segment at the cap
    assert mr.expected_unlisted(codes) == {2, 3, 4, 6} | set(np.flatnonzero(cnt.max(1) > 256).tolist())
    assert mr.expected_unlisted(codes) == _brute_unlisted(codes)
    assert 5 not in mr.expected_unlisted(codes) and 1 not in mr.expected_unlisted(codes)


def test_expected_unlisted_against_brute_force_at_many_ranges():
    rng = np.random.default_rng(5)
    for n in (3001, 430_000):
        m = 6
        codes = mr.base_codes(rng, m, n, 0.3)
        mr.sprinkle(rng, codes, rng.uniform(0.0, 0.03, m))
        cnt = mr.segment_counts(codes)
        assert cnt.shape == (m, mr.layout(n)[1]) and cnt.sum() == (codes == 3).sum()
        assert mr.expected_unlisted(codes) == _brute_unlisted(codes)


def test_pad_slots_of_the_last_byte():
    rng = np.random.default_rng(9)
    n = 3001
    codes = mr.base_codes(rng, 4, n, 0.4)
    plain, padded = mr.pack(codes), mr.pack(codes, pad3=True)
    assert plain.shape == padded.shape == (4, 751)
    assert np.array_equal(plain[:, :-1], padded[:, :-1])
    assert (padded[:, -1] >> 2 == 0x3F).all()                    # samples 3001 .. 3003: code 3
    assert np.array_equal(unpack_dosage_2bit(padded, n), codes)
    assert mr.block_subcap(430_000, 120) == 120 * 3359 // 256 and mr.block_subcap(3001, 200) == 262_144 // 32
