"""Variants whose missing genotypes do not fit the lists of the two-plane form.

The two-plane form of the score stage lists the missing genotypes of every (variant, sample range) segment.  A segment
of a row-major call with more than 256 of them (S3_LT_CAP), or a segment of a resident block that finds its sub-pool
full, is not listed: the epilogue puts the variant on its overflow list, score2b_kernel scores it in FP64 (filter, flip
and SPA records included) and stats["n_unlisted"] counts it.  These cases build such segments on purpose (row builders:
missing_rows.py) at the cap's edge, over many sample ranges, over ranges longer than the list kernels' registers and in
resident blocks, and hold every table against the oracle (integer fields bit-exact: a miscounted missing genotype moves
AF and mac) and every count of unlisted variants against what the rows say it must be.

Every case holds, besides its own rows: two variants above the missing-rate cutoff (0.15 here, so that rows at 8-10 %
missing stay valid), whose filter the FP64 kernel must apply; flipped variants (AF > 0.5); for binary traits, rare
variants whose carriers are all cases (p.norm < 0.05: the SPA stage), at least three of them unlisted.  From
N = 430 000 on, the saddle-point roots of those rare rows lie so far out that e^{g t} overflows in the reference's
Korg (SPATest.cpp:49): its p-value comes out 0 and the row falls back to p.norm, not converged -- which the SPA kernels
must reproduce (the `converged` column of assert_table_close).
"""
import numpy as np
import pytest

import missing_rows as mr
from conftest import assert_table_close

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

CUTOFF = 0.15


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """Import torch before the first HIP call of this process (libsaigehip.so binds to the torch wheel's runtime)."""
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    yield


def _model(n, trait, k, seed, missing=CUTOFF):
    from saigegds_amd import synth
    from saigegds_amd.nullmod import init_nullmod
    mod = synth.synth_null_model(n, trait, 0.3, n_cov=k, seed=seed)
    sm = init_nullmod(mod, np.arange(n), float("nan"), 4, missing, 0.05, float(mod.var_ratio[0]))
    assert sm.k == k
    return sm


def _oracle(sm, packed):
    from oracle import Oracle
    return Oracle(sm).scan_2bit(packed)


class Rows:
    """A code matrix filled row by row; remembers the rows of each kind."""

    def __init__(self, rng, sm, m, af_lo=0.02, af_hi=0.5, background=5e-4):
        self.rng, self.sm, self.n = rng, sm, sm.n
        af = rng.uniform(af_lo, af_hi, m)
        self.codes = mr.base_codes(rng, m, self.n, af)
        mr.sprinkle(rng, self.codes, background)
        self.next = 0
        self.kind = {}

    def take(self, kind, count=1):
        rows = list(range(self.next, self.next + count))
        assert rows[-1] < self.codes.shape[0], "more rows asked for than the matrix holds"
        self.next += count
        self.kind.setdefault(kind, []).extend(rows)
        return rows

    def flipped(self, v, af=None):
        """row v redrawn at an alt allele frequency above one half, keeping its missing genotypes"""
        af = self.rng.uniform(0.6, 0.9) if af is None else af
        miss = self.codes[v] == mr.MISSING
        self.codes[v] = mr.base_codes(self.rng, 1, self.n, af)[0]
        self.codes[v, miss] = mr.MISSING

    def rare_in_cases(self, v, carriers=16):
        """row v: `carriers` heterozygous cases, everybody else homozygous reference (missing genotypes kept)"""
        miss = self.codes[v] == mr.MISSING
        self.codes[v] = 0
        self.codes[v, miss] = mr.MISSING
        cases = np.flatnonzero((self.sm.y > 0.5) & ~miss)
        self.codes[v, self.rng.choice(cases, carriers, replace=False)] = 1

    def common_extras(self, unlisted_seg):
        """two rows above the cutoff, flipped rows and (binary) rare rows enriched in cases, each rare row with a
        segment of `unlisted_seg` missing genotypes"""
        for v in self.take("cutoff", 2):
            mr.sprinkle(self.rng, self.codes, 0.2, rows=[v])
        for v in self.take("flip", 6):
            self.flipped(v)
            if v % 2:
                mr.set_segment(self.rng, self.codes, v, int(self.rng.integers(len(mr.ranges(self.n)))), 257, "spread")
        if not self.sm.quant:
            for v in self.take("rare", 5):
                g = int(self.rng.integers(len(mr.ranges(self.n))))
                mr.set_segment(self.rng, self.codes, v, g, unlisted_seg, "run", offset=7)
                self.rare_in_cases(v)

    def done(self):
        assert self.next <= self.codes.shape[0]
        return self.codes


def _check_extras(rows, out, valid, ref, ref_valid, unlisted):
    """the cutoff rows are rejected, the flipped rows valid with AF > 0.5; binary: >= 3 unlisted rows go to SPA"""
    cut, flip = rows.kind["cutoff"], rows.kind["flip"]
    assert not valid[cut].any() and not ref_valid[cut].any()
    assert set(cut) <= unlisted
    assert ref_valid[flip].all() and (ref[flip, 0] > 0.5).all()
    if not rows.sm.quant:
        spa = {v for v in rows.kind["rare"] if ref_valid[v] and ref[v, 6] < 0.05}
        assert len(spa & unlisted) >= 3, (spa, unlisted)


def _same_tables(a, b, valid, quant, what):
    """two runs of the library: filter and counts bit-exact, the floats to 1e-11"""
    v = valid.astype(bool)
    assert np.array_equal(a[v][:, :3], b[v][:, :3]), what
    cols = slice(3, 6) if quant else slice(3, 8)
    np.testing.assert_allclose(a[v][:, cols], b[v][:, cols], rtol=1e-11, err_msg=what)


def _dev_rows(sc, packed):
    import torch
    m = packed.shape[0]
    bpv = sc.row_stride()
    t = torch.zeros((m, bpv), dtype=torch.uint8, device="cuda:0")
    t[:, :packed.shape[1]] = torch.from_numpy(packed).to("cuda:0")
    return t, bpv


def _dev_out(m):
    import torch
    return (torch.full((m, 8), -1.0, dtype=torch.float64, device="cuda:0"),
            torch.zeros(m, dtype=torch.uint8, device="cuda:0"))


# ---- A. the cap's edge, one range ------------------------------------------------------------------------------------
def _rows_cap_edge(sm, seed):
    """N = 3001 (one range): segments of 255, 256, 257 and 300 missing genotypes, spread over the range or packed
    against sample N - 1 (the last, partial piece of the row), each on a common, a flipped and (binary) a rare row."""
    rng = np.random.default_rng(seed)
    r = Rows(rng, sm, 120)
    for count in (255, 256, 257, 300):
        for where in ("spread", "end"):
            (v,) = r.take(f"{count}/{where}")
            mr.set_segment(rng, r.codes, v, 0, count, where)
            (v,) = r.take(f"{count}/{where}/flip")
            r.flipped(v)
            mr.set_segment(rng, r.codes, v, 0, count, where)
            if not sm.quant:
                (v,) = r.take(f"{count}/{where}/rare")
                mr.set_segment(rng, r.codes, v, 0, count, where)
                r.rare_in_cases(v)
                if count > 256:
                    r.kind.setdefault("rare", []).append(v)
    r.common_extras(400)
    for v in r.take("background", 30):
        mr.sprinkle(rng, r.codes, 0.01, rows=[v])
    return r


@pytest.mark.parametrize("trait,k", [("binary", 5), ("quantitative", 3)])
def test_cap_edge_one_range(trait, k):
    """255 / 256 are listed, 257 / 300 are not (row-major calls: S3_LT_CAP = 256 per segment); the two-plane count of
    unlisted variants is exact, the three-plane form lists nothing and counts none; both forms and the FP64 kernel
    ("score_v1") give the same rows.  The same with code 3 in the unused 2-bit slots of the last byte (samples
    3001 .. 3003), which must count for nothing."""
    from saigegds_amd._lib import Scanner
    sm = _model(3001, trait, k, seed=71)
    r = _rows_cap_edge(sm, 72)
    codes = r.done()
    exp = mr.expected_unlisted(codes)
    cnt = mr.segment_counts(codes)[:, 0]
    for count in (255, 256, 257, 300):
        for where in ("spread", "end"):
            v = r.kind[f"{count}/{where}"][0]
            assert cnt[v] == count and (v in exp) == (count > 256)
    ref, ref_valid = _oracle(sm, mr.pack(codes))
    print(f"\nA {trait} K={k}: {codes.shape[0]} rows, segments {sorted(set(cnt.tolist()) & {255, 256, 257, 300})} placed, "
          f"{len(exp)} expected unlisted")
    with Scanner(sm) as sc:
        for pad3 in (False, True):
            packed = mr.pack(codes, pad3=pad3)
            res = {}
            for form in (0, 1):
                sc.set_option("three_plane", form)
                out, valid = sc.scan_2bit(packed)
                st = sc.stats()
                what = f"A {trait} pad3={pad3} three_plane={form}"
                print(f"{what}: n_unlisted {st['n_unlisted']}, n_spa {st['n_spa']}")
                assert st["three_plane"] == form, st
                assert st["n_unlisted"] == (len(exp) if form == 0 else 0), (what, st, sorted(exp))
                assert_table_close(out, valid, ref, ref_valid, quant=sm.quant, what=what)
                res[form] = (out, valid)
            assert np.array_equal(res[0][1], res[1][1])
            _same_tables(res[0][0], res[1][0], ref_valid, sm.quant, f"A {trait} pad3={pad3}: two planes against three")
            sc.set_option("score_v1", 1)
            v1, v1_valid = sc.scan_2bit(packed)
            sc.set_option("score_v1", 0)
            u = sorted(exp)
            assert np.array_equal(v1_valid[u], res[0][1][u])
            np.testing.assert_allclose(res[0][0][u], v1[u], rtol=1e-11, equal_nan=True,
                                       err_msg=f"A {trait} pad3={pad3}: unlisted rows against the FP64 kernel's")
            _check_extras(r, res[0][0], res[0][1], ref, ref_valid, exp)


# ---- B. many ranges ---------------------------------------------------------------------------------------------------
def _rows_many_ranges(sm, seed, m=200):
    """N = 430 000 (14 ranges of 30 720 samples), 0.05 % missing everywhere, and on top: runs of 257 and 2 000 inside
    one range, a whole range missing (an untyped batch), 256 on each side of a range boundary (512 in all, every
    segment listed), 255 in every range (3 570 in all, listed), uniform 1-3 % (300-900 per range: unlisted)."""
    rng = np.random.default_rng(seed)
    n = sm.n
    rg = mr.ranges(n)
    nr = len(rg)
    r = Rows(rng, sm, m)
    for v in r.take("run257", 10):
        mr.set_segment(rng, r.codes, v, int(rng.integers(nr)), 257, "run", offset=int(rng.integers(0, 30_000)))
    for v in r.take("run2000", 10):
        mr.set_segment(rng, r.codes, v, int(rng.integers(nr)), 2000, "run", offset=int(rng.integers(0, 28_000)))
    for v in r.take("whole_range", 6):
        g = int(rng.integers(nr))
        mr.set_segment(rng, r.codes, v, g, rg[g][1] - rg[g][0], "start")
    for v in r.take("boundary", 10):
        g = int(rng.integers(nr - 1))
        mr.set_segment(rng, r.codes, v, g, 256, "end")
        mr.set_segment(rng, r.codes, v, g + 1, 256, "start")
    for v in r.take("255_everywhere", 10):
        for g in range(nr):
            mr.set_segment(rng, r.codes, v, g, 255, "spread")
    rows = r.take("uniform", 40)
    mr.sprinkle(rng, r.codes, rng.uniform(0.01, 0.03, len(rows)), rows=rows)
    r.common_extras(2000)
    return r


def test_many_ranges_host_pipeline_and_lanes():
    """N = 430 000: the host scan in three chunks (pipe_mb = 8: 78 rows of 107 520 bytes per chunk) sums the chunks'
    counts of unlisted variants; device-resident calls on two lanes, plain and with the deferred dense pass
    (force_dense), give the same tables and counts.  three_plane 0 (exact counts) and automatic (the count of each
    call that took the two-plane form exact, none in a three-plane call)."""
    from saigegds_amd._lib import Scanner
    sm = _model(430_000, "binary", 5, seed=81)
    r = _rows_many_ranges(sm, 82)
    codes = r.done()
    m = codes.shape[0]
    exp = mr.expected_unlisted(codes)
    cnt = mr.segment_counts(codes)
    for v in r.kind["boundary"] + r.kind["255_everywhere"]:
        assert v not in exp and cnt[v].max() <= 256
    assert set(r.kind["run257"] + r.kind["run2000"] + r.kind["whole_range"] + r.kind["uniform"]) <= exp
    packed = mr.pack(codes)
    ref, ref_valid = _oracle(sm, packed)
    print(f"\nB: {m} rows, largest segments {sorted(set(cnt.max(1).tolist()))[-6:]}, {len(exp)} expected unlisted")
    calls = [(0, 70), (70, 140), (140, m)]
    with Scanner(sm) as sc:
        sc.set_option("pipe_mb", 8)
        for form in (0, -1):
            sc.set_option("three_plane", form)
            sc.stats_total(reset=True)
            out, valid = sc.scan_2bit(packed)
            st = sc.stats()
            tot, ncalls = sc.stats_total(reset=True)
            what = f"B host, three_plane={form}"
            print(f"{what}: {ncalls} chunks, {tot['three_plane']} of them three-plane, n_unlisted {st['n_unlisted']}")
            assert ncalls >= 3
            assert_table_close(out, valid, ref, ref_valid, what=what)
            if tot["three_plane"] == 0:
                assert st["n_unlisted"] == len(exp), (what, st)
            else:
                assert form == -1 and st["n_unlisted"] <= len(exp)
            _check_extras(r, out, valid, ref, ref_valid, exp)
        rows, bpv = _dev_rows(sc, packed)
        o, vd = _dev_out(m)
        sc.set_option("lanes", 2)
        for dense in (0, 1):
            sc.set_option("force_dense", dense)
            for form in (0, -1):
                sc.set_option("three_plane", form)
                sc.stats_total(reset=True)
                want = 0
                forms = []
                for a, b in calls:
                    sc.scan_2bit_dev(rows[a].data_ptr(), bpv, b - a, o[a].data_ptr(), vd[a].data_ptr())
                    if form == -1:                  # (the stats of each call: syncs)
                        st = sc.stats()
                        forms.append(st["three_plane"])
                        want_call = 0 if st["three_plane"] else len(exp & set(range(a, b)))
                        assert st["n_unlisted"] == want_call, (a, b, st)
                    else:
                        want += len(exp & set(range(a, b)))
                sc.sync()
                tot, ncalls = sc.stats_total(reset=True)
                what = f"B device, lanes=2, force_dense={dense}, three_plane={form}"
                print(f"{what}: forms {forms or [0] * 3}, n_unlisted {tot['n_unlisted']}, n_spa_dense {tot['n_spa_dense']}")
                assert ncalls == 3
                if form == 0:
                    assert tot["three_plane"] == 0 and tot["n_unlisted"] == want == len(exp), tot
                if dense:
                    assert tot["n_spa_dense"] > 0, tot
                assert_table_close(o.cpu().numpy(), vd.cpu().numpy(), ref, ref_valid, what=what)
        sc.set_option("lanes", 1)


# ---- C. long ranges ---------------------------------------------------------------------------------------------------
def test_long_ranges_at_the_cap():
    """N = 540 001: 16 ranges of 33 536-33 792 samples, longer than the 8 x 64 pieces a wave of s3_lists_t3_kernel
    holds, so the pass walks each range in strides of 64 pieces (its `npiece > MAXLD * 64` branch).  256 and 257
    missing genotypes at the start and at the end of a range, the last range included (its end is sample N - 1)."""
    from saigegds_amd._lib import Scanner
    sm = _model(540_001, "binary", 5, seed=91)
    rng = np.random.default_rng(92)
    nr = len(mr.ranges(sm.n))
    r = Rows(rng, sm, 40)
    for g in (3, nr - 1):
        for count in (256, 257):
            for where in ("start", "end"):
                (v,) = r.take(f"{count}/{where}/{g}")
                mr.set_segment(rng, r.codes, v, g, count, where)
    r.common_extras(300)
    codes = r.done()
    exp = mr.expected_unlisted(codes)
    cnt = mr.segment_counts(codes)
    for g in (3, nr - 1):
        for where in ("start", "end"):
            assert r.kind[f"257/{where}/{g}"][0] in exp and r.kind[f"256/{where}/{g}"][0] not in exp
    packed = mr.pack(codes)
    ref, ref_valid = _oracle(sm, packed)
    with Scanner(sm) as sc:
        sc.set_option("three_plane", 0)
        out, valid = sc.scan_2bit(packed)
        st = sc.stats()
    print(f"\nC: 40 rows, segments of {sorted(set(cnt.max(1).tolist()))[-5:]}..., n_unlisted {st['n_unlisted']} "
          f"(expected {len(exp)})")
    assert st["three_plane"] == 0 and st["n_unlisted"] == len(exp), st
    assert_table_close(out, valid, ref, ref_valid, what="C long ranges")
    _check_extras(r, out, valid, ref, ref_valid, exp)


# ---- D. resident blocks with full sub-pools ----------------------------------------------------------------------------
def _scan_block(sc, blk, m):
    o, v = _dev_out(m)
    sc.scan_block(blk, o.data_ptr(), v.data_ptr())
    sc.sync()
    return o.cpu().numpy(), v.cpu().numpy()


def test_resident_block_with_full_pools():
    """A block of 120 variants at N = 430 000.  Its pool holds max(64, N // 128) = 3 359 entries per variant:
    120 x 3 359 = 403 080 entries, cut into nsub sub-pools, nsub the largest power of two <= min(1024, full_wg) with
    full_wg = ceil(120 x 14 ranges / 4) = 420 workgroups of a full load: 256 sub-pools of 403 080 // 256 = 1 574
    entries.  A fully missing range is 30 720 entries: larger than any sub-pool, its segment never touches the cursor
    (the `fits` branch) and the variant is unlisted; rows at 2-5 % missing (600-1 500 per segment, each above an
    eighth of a sub-pool: the per-wave reservations) fill their sub-pools, and some of their segments find them full.
    Two planes: the table is the oracle's and the row-major call's; automatic: the census of the load turns the block
    to the three-plane form, which lists nothing."""
    from saigegds_amd._lib import Block, Scanner
    sm = _model(430_000, "binary", 5, seed=101)
    rng = np.random.default_rng(102)
    n, m = sm.n, 120
    rg = mr.ranges(n)
    subcap = mr.block_subcap(n, m)
    assert subcap == 1574 and min(s1 - s0 for s0, s1 in rg) > subcap
    r = Rows(rng, sm, m)
    for v in r.take("whole_range", 8):
        g = int(rng.integers(len(rg)))
        mr.set_segment(rng, r.codes, v, g, rg[g][1] - rg[g][0], "start")
    rows = r.take("dirty", 60)
    mr.sprinkle(rng, r.codes, rng.uniform(0.02, 0.05, len(rows)), rows=rows)
    r.common_extras(2000)
    codes = r.done()
    packed = mr.pack(codes)
    ref, ref_valid = _oracle(sm, packed)
    cnt = mr.segment_counts(codes)
    with Scanner(sm) as sc, Block(n, m) as blk:
        sc.set_option("three_plane", 0)
        rm, rm_valid = sc.scan_2bit(packed)
        st_rm = sc.stats()
        sc.load_block(blk, packed)
        o0, v0 = _scan_block(sc, blk, m)
        st0 = sc.stats()
        sc.set_option("three_plane", -1)
        o1, v1 = _scan_block(sc, blk, m)
        st1 = sc.stats()
    too_big = set(np.flatnonzero((cnt > subcap).any(1)).tolist())      # unlisted whatever the sub-pools hold
    print(f"\nD: {m} rows, {len(too_big)} with a segment above the sub-pool ({subcap}); "
          f"block n_unlisted {st0['n_unlisted']}, row-major n_unlisted {st_rm['n_unlisted']}, automatic form {st1['three_plane']}")
    assert set(r.kind["whole_range"] + r.kind["cutoff"]) <= too_big
    assert st0["three_plane"] == 0 and st0["n_unlisted"] >= len(too_big), st0
    assert_table_close(o0, v0, ref, ref_valid, what="D block, two planes")
    assert np.array_equal(v0, rm_valid)
    _same_tables(o0, rm, ref_valid, False, "D block against the row-major call")
    assert st1["three_plane"] == 1 and st1["n_unlisted"] == 0, st1
    assert_table_close(o1, v1, ref, ref_valid, what="D block, automatic form")
    _same_tables(o0, o1, ref_valid, False, "D block, two planes against three")
    _check_extras(r, o0, v0, ref, ref_valid, too_big)


def test_small_block_with_heavy_missingness():
    """N = 3001, 200 rows at 30-40 % missing (900-1 200 per segment) in a block: 4 variants of a workgroup hold more
    than an eighth of a sub-pool (262 144 entries // 32 sub-pools = 8 192; an eighth is 1 024), so each wave reserves
    for itself (the `together = false` branch of the reservation), and the sub-pools that two workgroups share fill up.
    The missing-rate cutoff is 0.5 here so that these rows are scored; the two rows above it are at 60 %."""
    from saigegds_amd._lib import Block, Scanner
    sm = _model(3001, "binary", 5, seed=111, missing=0.5)
    rng = np.random.default_rng(112)
    m = 200
    assert mr.block_subcap(sm.n, m) == 8192
    r = Rows(rng, sm, m)
    rows = r.take("heavy", 190)
    mr.sprinkle(rng, r.codes, rng.uniform(0.3, 0.4, len(rows)), rows=rows)
    for v in r.take("cutoff", 2):
        mr.sprinkle(rng, r.codes, 0.6, rows=[v])
    codes = r.done()
    packed = mr.pack(codes)
    ref, ref_valid = _oracle(sm, packed)
    assert not ref_valid[r.kind["cutoff"]].any() and ref_valid[rows].sum() > 150
    with Scanner(sm) as sc, Block(sm.n, m) as blk:
        sc.set_option("three_plane", 0)
        sc.load_block(blk, packed)
        o, v = _scan_block(sc, blk, m)
        st = sc.stats()
    print(f"\nD small block: n_unlisted {st['n_unlisted']} of {m}")
    assert st["three_plane"] == 0
    assert_table_close(o, v, ref, ref_valid, what="D small block, per-wave reservations")


# ---- E. the `over` rule of row-major calls -------------------------------------------------------------------------
def test_over_rule_turns_row_major_calls_to_three_planes():
    """Binary K = 5 at N = 50 000 (two ranges), 400 rows: 20 rows (5 %, more than 1/32) with a run of 300 missing
    genotypes in one range, plus the rare and cutoff rows, 0.17 % of all genotypes missing.  The first device-resident
    call is two-plane with the exact count of unlisted variants; more than 1/32 of them unlisted turns the next call
    to the three-plane form.  That step counts fewer than 0.3 % missing (SGX_DENSE_OFF) and turns the calls after it
    back: with missingness this concentrated the forms alternate (printed, not pinned)."""
    from saigegds_amd._lib import Scanner
    sm = _model(50_000, "binary", 5, seed=121)
    rng = np.random.default_rng(122)
    m = 400
    r = Rows(rng, sm, m)
    for v in r.take("run300", 20):
        mr.set_segment(rng, r.codes, v, int(rng.integers(2)), 300, "run", offset=int(rng.integers(0, 24_000)))
    for v in r.take("cutoff", 2):
        mr.sprinkle(rng, r.codes, 0.16, rows=[v])
    for v in r.take("flip", 6):
        r.flipped(v)
    for v in r.take("rare", 4):
        mr.set_segment(rng, r.codes, v, int(rng.integers(2)), 300, "run", offset=11)
        r.rare_in_cases(v)
    codes = r.done()
    exp = mr.expected_unlisted(codes)
    frac = float((codes == mr.MISSING).mean())
    assert len(exp) * 32 > m and frac < 0.003, (len(exp), frac)
    packed = mr.pack(codes)
    ref, ref_valid = _oracle(sm, packed)
    forms = []
    with Scanner(sm) as sc:
        rows, bpv = _dev_rows(sc, packed)
        o, vd = _dev_out(m)
        for call in range(4):
            sc.scan_2bit_dev(rows.data_ptr(), bpv, m, o.data_ptr(), vd.data_ptr())
            st = sc.stats()
            forms.append((st["three_plane"], st["n_unlisted"]))
            if call == 0:
                assert st["three_plane"] == 0 and st["n_unlisted"] == len(exp), st
                _check_extras(r, o.cpu().numpy(), vd.cpu().numpy(), ref, ref_valid, exp)
            if call == 1:
                assert st["three_plane"] == 1 and st["n_unlisted"] == 0, st
            assert_table_close(o.cpu().numpy(), vd.cpu().numpy(), ref, ref_valid, what=f"E call {call}")
    print(f"\nE: {len(exp)} of {m} rows unlisted, {100 * frac:.3f} % missing; (three_plane, n_unlisted) per call: {forms}")


# ---- F. the form a call reports, and the choice it leaves, on the FP64 paths ------------------------------------------
def test_fp64_calls_report_their_own_form_and_keep_the_choice():
    """A call of the FP64 kernels ("score_v1") after a three-plane call reports three_plane = 0 and no unlisted
    variants, and leaves the automatic choice of the next fixed-point call as it was -- row-major calls and a resident
    block scanned through sgx_scan_block's FP64 branch alike."""
    from saigegds_amd._lib import Block, Scanner
    sm = _model(3001, "binary", 5, seed=131)
    rng = np.random.default_rng(132)
    m = 800
    codes = mr.base_codes(rng, m, sm.n, rng.uniform(0.02, 0.5, m))
    mr.sprinkle(rng, codes, 0.03)
    packed = mr.pack(codes)
    ref, ref_valid = _oracle(sm, packed)
    seq = []
    with Scanner(sm) as sc, Block(sm.n, m) as blk:
        limbs, _ = sc.score_layout()
        assert (int(limbs.sum()) + 1 + 15) // 16 + 1 > 4, "the model must be wide enough for the two-plane form"
        rows, bpv = _dev_rows(sc, packed)
        o, vd = _dev_out(m)

        def call(v1, block=False):
            sc.set_option("score_v1", v1)
            if block:
                sc.scan_block(blk, o.data_ptr(), vd.data_ptr())
            else:
                sc.scan_2bit_dev(rows.data_ptr(), bpv, m, o.data_ptr(), vd.data_ptr())
            st = sc.stats()
            seq.append(("block" if block else "rows", v1, st["three_plane"], st["n_unlisted"]))
            assert_table_close(o.cpu().numpy(), vd.cpu().numpy(), ref, ref_valid, what=f"F call {len(seq)}")
            return st

        assert call(0)["three_plane"] == 0                  # 3 % missing: this step turns the next calls over
        assert call(0)["three_plane"] == 1
        st = call(1)
        assert st["three_plane"] == 0 and st["n_unlisted"] == 0, (seq, st)
        assert call(0)["three_plane"] == 1, seq             # the FP64 call left the choice alone
        sc.load_block(blk, packed)
        assert call(0, block=True)["three_plane"] == 1      # (the block's census: 3 % missing)
        st = call(1, block=True)
        assert st["three_plane"] == 0 and st["n_unlisted"] == 0, (seq, st)
        assert call(0)["three_plane"] == 1, seq
        assert call(0, block=True)["three_plane"] == 1, seq
    print("\nF: (input, score_v1, three_plane, n_unlisted) per call:", seq)
