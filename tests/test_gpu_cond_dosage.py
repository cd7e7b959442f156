"""sgx_ds_block_cond_set / sgx_ds_block_cond and the dosage route of seqAssocGLMM_SPA_cond on the device: the kernel
against the long-double reference of tests/cond_ds_ref.py, the identities that tie it to sgx_ds_block_skat, to the
hard-call kernel and to the pinned scan, determinism, the error paths, and the driver against its run with the numpy
stand-in.  Bounds: check() of tests/test_gpu_cond.py (REL_TOL and Z_FLOOR of conftest, derived in tests/test_gpu_skat.py).
Models as there: the golden models at N = 1000, synth_null_model otherwise.  Rows: the hard calls of
skat_ref.hard_calls (1 % missing, every 7th row alt-major) -- as uint8 with 0xFF, or as float64 with 30 % of the
genotypes blurred and NaN --, flip and mean as the driver forms them; scanned row ALL_MISS holds no value at all.  The
first NC rows of a case are the conditioning set, loaded into a block of their own that is freed before the scan."""
import os

import numpy as np
import pytest

import cond_ds_ref as CD
import skat_ds_ref as D
import skat_ref as R
from test_gpu_cond import check
from test_gpu_skat import _flat, _model

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NC = 8
WG_ROWS = 256             # COND_WG_ROWS of kern_cond.h: the rows one workgroup owns
ALL_MISS = 5
_cache = {}


def make_rows(n, kind, m, seed):
    codes = R.hard_calls(n, m, seed)
    if kind == "u8":
        return np.where(codes == 3, 0xFF, codes).astype(np.uint8), codes
    rng = np.random.default_rng(seed)
    x = np.where(codes == 3, np.nan, codes.astype(np.float64))
    return np.clip(x + rng.normal(0, 0.08, x.shape) * (rng.random(x.shape) < 0.3), 0, 2), codes


def _case(n, kind, m=WG_ROWS + 1):
    """Per (N, row type), made once: model, set rows, scanned rows with their flip / mean, the long-double reference."""
    if (n, kind) not in _cache:
        sm = _model(n)
        rows, codes = make_rows(n, kind, NC + m, 17 + n)
        rows[NC + ALL_MISS] = 0xFF if kind == "u8" else np.nan
        flip, mean = D.flip_mean(rows)
        assert np.isnan(mean[NC + ALL_MISS]) and np.isfinite(np.delete(mean, NC + ALL_MISS)).all()
        c = dict(sm=sm, rows_c=rows[:NC], fc=flip[:NC], mc=mean[:NC], rows=rows[NC:], fl=flip[NC:], mn=mean[NC:], codes=codes)
        # a row whose values are all the same has Phi_jj = 0 in exact arithmetic (the intercept explains it): no relative
        # bound applies to it, so it is not compared (N = 63 has a few; picked from the input, not from any result)
        ok = [D.ok_mask(r) for r in c["rows"]]
        c["skip"] = np.array([j for j, (r, k) in enumerate(zip(c["rows"], ok)) if not k.any() or np.ptp(r[k].astype(np.float64)) == 0])
        assert ALL_MISS in c["skip"] and c["skip"].size <= (40 if n < 100 else 1), c["skip"]
        c["ref"] = CD.cond_ds_ref(sm, c["rows"], c["fl"], c["mn"], c["rows_c"], c["fc"], c["mc"])
        _cache[(n, kind)] = c
    return _cache[(n, kind)]


def _block(sc, rows):
    blk = sc.dosage_block(rows.dtype, rows.shape[0])
    blk.load(rows)
    return blk


def install(sc, c):
    with _block(sc, c["rows_c"]) as b:
        return b.cond_set(np.arange(len(c["rows_c"])), c["fc"], c["mc"])


def run(sc, c, a, b):
    """Rows [a, b) of the case through a block of their own."""
    with _block(sc, c["rows"][a:b]) as blk:
        return blk.cond(c["fl"][a:b], c["mn"][a:b])


def check_rows(got, c, a, b, what):
    keep = np.setdiff1d(np.arange(a, b), c["skip"])
    if keep.size:
        check(got[0][keep - a], got[1][keep - a], got[2][keep - a], c["ref"], keep, what)


@pytest.mark.parametrize("n", [63, 1000, 1001, 70001])
@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_1_kernel_against_the_reference(kind, n):
    """N = 63: below one iteration (u8); 1000 / 1001: even / odd, so that rows start misaligned; 70001: two slab cuts
    and a tail.  M = 1, 15, 17, 257."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    c = _case(n, kind)
    with Scanner(c["sm"]) as sc:
        s_c, phi_cc = install(sc, c)
        for m in (1, 15, 17, WG_ROWS + 1):
            check_rows(run(sc, c, 0, m), c, 0, m, f"{kind} N={n} m={m}")
    R_cc = np.asarray(c["ref"]["Phi_CC"], dtype=np.float64)
    assert np.all(np.abs(phi_cc - R_cc) <= 1e-10 * np.sqrt(np.outer(np.diag(R_cc), np.diag(R_cc))))
    assert np.array_equal(phi_cc, phi_cc.T)


@pytest.mark.parametrize("k,nc", [(3, 1), (3, 9), (3, 10), (8, 16), (16, 16)])
@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_2_column_tiles(kind, k, nc):
    """2K + 1 + C = 8, 16, 17, 33, 49 columns of B."""
    import torch  # noqa: F401
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    n, m = 1000, 17
    sm = _flat(synth.synth_null_model(n, "binary" if k != 8 else "quantitative", 0.2, n_cov=k, seed=20260 + k))
    assert sm.k == k
    rows, _ = make_rows(n, kind, nc + m, 5 + k + nc)
    flip, mean = D.flip_mean(rows)
    c = dict(sm=sm, rows_c=rows[:nc], fc=flip[:nc], mc=mean[:nc], rows=rows[nc:], fl=flip[nc:], mn=mean[nc:])
    ref = CD.cond_ds_ref(sm, c["rows"], c["fl"], c["mn"], c["rows_c"], c["fc"], c["mc"])
    with Scanner(sm) as sc:
        install(sc, c)
        score, var, cov = run(sc, c, 0, m)
    check(score, var, cov, ref, slice(0, m), f"{kind} K={k} C={nc}")


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_3_cond_set_equals_block_skat(kind):
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    for n in (1000, 70001):
        c = _case(n, kind)
        with Scanner(c["sm"]) as sc, _block(sc, c["rows"][:20]) as blk:
            idx = np.array([3, 0, 19, 7, 11], dtype=np.int32)                      # not in block order
            s, covs = blk.skat([0, idx.size], idx, c["fl"][idx], c["mn"][idx])
            s_c, phi_cc = blk.cond_set(idx, c["fl"][idx], c["mn"][idx])
        assert s_c.tobytes() == s.tobytes() and phi_cc.tobytes() == covs[0].tobytes(), n


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_4_ties_to_the_per_unit_route(kind):
    """cov[j], var[j] and score[j] against DosageBlock.skat on the units {j} + C, within the bound of test 1."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    c = _case(70001, kind)
    m = 40
    use = np.setdiff1d(np.arange(m), [ALL_MISS])
    allr = np.concatenate([c["rows_c"], c["rows"][:m]])
    allf, allm = np.concatenate([c["fc"], c["fl"][:m]]), np.concatenate([c["mc"], c["mn"][:m]])
    idx = np.concatenate([np.concatenate([[NC + j], np.arange(NC)]) for j in use])
    ptr = np.arange(0, (use.size + 1) * (NC + 1), NC + 1)
    with Scanner(c["sm"]) as sc:
        install(sc, c)
        score, var, cov = run(sc, c, 0, m)
        with _block(sc, allr) as blk:
            s2, covs = blk.skat(ptr, idx, allf[idx], allm[idx])
    worst = 0.0
    for k, j in enumerate(use):
        phi = covs[k]
        sd = np.sqrt(np.diag(phi))
        e = np.abs(np.concatenate([[var[j]], cov[j]]) - phi[0]) / (1e-10 * sd[0] * sd)
        worst = max(worst, float(e.max()))
        assert abs(score[j] - s2[ptr[k]]) <= 1e-10 * abs(s2[ptr[k]]) + 1e-12 * sd[0]
    print(kind, "largest difference to the per-unit route, in units of the tolerance:", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("n", [1000, 70001])
def test_5_ties_to_the_hard_call_kernel(n):
    """Hard-call u8 rows through the new entries and, packed, through Scanner.cond_set / cond_2bit: both within the
    bound of the same reference."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    c = _case(n, "u8")
    m = 40
    codes = c["codes"][:NC + m].copy()
    codes[NC + ALL_MISS] = 3
    packed, lut = pack_dosage_2bit(codes), R.tables(codes)
    with Scanner(c["sm"]) as sc:
        install(sc, c)
        ds = run(sc, c, 0, m)
        sc.cond_set(packed[:NC], lut[:NC])
        hc = sc.cond_2bit(packed[NC:], lut[NC:])
    check_rows(ds, c, 0, m, f"dosage rows N={n}")
    check_rows(hc, c, 0, m, f"2-bit rows N={n}")


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_6_ties_to_the_pinned_scan(kind, trait):
    """chdtrc(1, score^2 / var) = the pval_noadj of the block's own scan(), as test 5 of tests/test_gpu_cond.py."""
    import torch  # noqa: F401
    from scipy.special import chdtrc
    from saigegds_amd._lib import Scanner
    c = _case(1000, kind)
    sm = _model(1000, trait)
    use = np.setdiff1d(np.arange(64), [ALL_MISS])
    with Scanner(sm) as sc:
        install(sc, c)
        with _block(sc, c["rows"][:64]) as blk:
            out, valid = blk.scan()
            score, var, _ = blk.cond(c["fl"][:64], c["mn"][:64])
    assert valid[use].all()
    p = chdtrc(1.0, score[use] ** 2 / var[use])
    ref = out[use, 5 if sm.quant else 6]
    err = np.abs(p - ref) / ref
    print(kind, trait, "largest relative difference to the scan's pval_noadj", err.max())
    assert np.all(err <= 1e-10)


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_7_determinism(kind):
    """The same bytes twice, for a row wherever it sits and whatever M is, and on either side of COND_WG_ROWS (one and
    two row groups; the cut by COND_PART_BYTES takes over 10^5 rows at this N and goes through the same offsets)."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    c = _case(70001, kind)
    with Scanner(c["sm"]) as sc:
        install(sc, c)
        big = run(sc, c, 0, WG_ROWS + 1)
        again = run(sc, c, 0, WG_ROWS + 1)
        one_group = run(sc, c, 0, WG_ROWS)
        mid = run(sc, c, 37, 60)
        last = run(sc, c, WG_ROWS, WG_ROWS + 1)
        install(sc, c)                                        # the set installed again: the same B
        again2 = run(sc, c, 37, 60)
    for k in range(3):
        assert big[k].tobytes() == again[k].tobytes(), "twice"
        assert big[k][:WG_ROWS].tobytes() == one_group[k].tobytes(), "M = COND_WG_ROWS and COND_WG_ROWS + 1"
        assert big[k][37:60].tobytes() == mid[k].tobytes(), "rows [37, 60) alone"
        assert big[k][WG_ROWS:].tobytes() == last[k].tobytes(), "the last row alone"
        assert mid[k].tobytes() == again2[k].tobytes(), "after a second cond_set"


def test_8_errors_leave_the_handle_usable():
    """Every refusal that can be reached from one process on one device (a twin handle and a second device cannot)."""
    import torch  # noqa: F401
    from saigegds_amd import _lib
    from saigegds_amd._lib import COND_MAX, Scanner
    L = _lib.load()
    c = _case(1000, "f64")
    m = 4
    rows = np.ascontiguousarray(c["rows"][:m])
    fl, mn = np.ascontiguousarray(c["fl"][:m]), np.ascontiguousarray(c["mn"][:m])
    s, v, cv = np.zeros(m), np.zeros(m), np.zeros(m * NC)
    idx = np.arange(NC, dtype=np.int32)
    fc, mc = np.ascontiguousarray(c["fc"]), np.ascontiguousarray(c["mc"])
    sC, cC = np.zeros(COND_MAX + 1), np.zeros((COND_MAX + 1) ** 2)
    p = lambda a: a.ctypes.data     # noqa: E731
    with Scanner(c["sm"]) as sc, Scanner(_model(63)) as other:
        h = sc._h
        with _block(sc, rows) as blk, sc.dosage_block(np.float64, 4) as empty, _block(sc, c["rows_c"]) as cblk, \
                other.dosage_block(np.float64, 4) as alien:
            def good():
                score, var, cov = blk.cond(fl, mn)
                check(score, var, cov, c["ref"], slice(0, m), "after an error")
            ok = (p(fl), p(mn), p(s), p(v), p(cv))
            # no set installed
            assert L.sgx_ds_block_cond(h, blk._b, *ok) == -1 and b"no conditioning set" in L.sgx_last_error()
            cblk.cond_set(idx, fc, mc)
            good()
            # sgx_ds_block_cond
            for i in range(5):
                args = list(ok)
                args[i] = None
                assert L.sgx_ds_block_cond(h, blk._b, *args) == -1 and b"NULL buffer" in L.sgx_last_error()
                good()
            assert L.sgx_ds_block_cond(None, blk._b, *ok) == -1 and L.sgx_ds_block_cond(h, None, *ok) == -1
            assert L.sgx_ds_block_cond(h, empty._b, *ok) == -1 and b"nothing loaded" in L.sgx_last_error()
            assert L.sgx_ds_block_cond(h, alien._b, *ok) == -1 and b"Invalid length of dosages" in L.sgx_last_error()
            good()
            # sgx_ds_block_cond_set: none of these replaces the installed set
            okc = (NC, p(idx), p(fc), p(mc), p(sC), p(cC))
            for i in range(1, 6):
                args = list(okc)
                args[i] = None
                assert L.sgx_ds_block_cond_set(h, cblk._b, *args) == -1 and b"NULL buffer" in L.sgx_last_error()
                good()
            big = np.zeros(COND_MAX + 1, dtype=np.int32)
            assert L.sgx_ds_block_cond_set(h, cblk._b, COND_MAX + 1, p(big), p(np.zeros(COND_MAX + 1, dtype=np.uint8)),
                                           p(np.zeros(COND_MAX + 1)), p(sC), p(cC)) == -1 and b"at most" in L.sgx_last_error()
            for bad in (NC, -1):
                out = idx.copy()
                out[3] = bad
                assert L.sgx_ds_block_cond_set(h, cblk._b, NC, p(out), p(fc), p(mc), p(sC), p(cC)) == -1
                assert b"outside the block" in L.sgx_last_error()
            assert L.sgx_ds_block_cond_set(h, empty._b, *okc) == -1 and b"nothing loaded" in L.sgx_last_error()
            assert L.sgx_ds_block_cond_set(h, alien._b, *okc) == -1 and b"Invalid length of dosages" in L.sgx_last_error()
            assert L.sgx_ds_block_cond_set(None, cblk._b, *okc) == -1 and L.sgx_ds_block_cond_set(h, None, *okc) == -1
            good()
            # clearing the set
            cblk.cond_set(idx[:0], fc[:0], mc[:0])
            assert L.sgx_ds_block_cond(h, blk._b, *ok) == -1 and b"no conditioning set" in L.sgx_last_error()
            cblk.cond_set(idx, fc, mc)
            good()


def _driver_pair(src, mod, cond, **kw):
    """The driver with the stand-in (first: the skip rule is settled on the CPU) and on the device."""
    from saigegds_amd import seqAssocGLMM_SPA_cond
    from saigegds_amd.cond import cond_tests
    ref = seqAssocGLMM_SPA_cond(src, mod, cond, verbose=False, scanner_factory=CD.NumpyCondDsScanner, **kw)
    st = CD.NumpyCondDsScanner.last
    S, var, cov = (np.concatenate([r[k] for r in st.cond_log]) for k in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        _, se, _ = cond_tests(S, var, cov, st.cond_S, st.cond_Phi)
        share = 1 - 1 / (se * se * var)                   # of Phi_jj that the set explains; NaN: the row gets NaN anyway
    near = np.flatnonzero(share > 0.9)
    assert near.size <= 4, near                           # the cap of test 6 of tests/test_gpu_cond.py
    got = seqAssocGLMM_SPA_cond(src, mod, cond, verbose=False, **kw)
    return got, ref, near


def _driver_check(got, ref, vid, near, cond):
    from conftest import assert_table_close
    assert list(got.keys()) == list(ref.keys())
    for c in ("id", "pos", "num"):
        assert np.array_equal(got[c], ref[c]), c
    cols = [c for c in ("AF.alt", "mac", "num", "beta", "SE", "pval", "p.norm", "converged") if c in got]
    tab = lambda a: np.stack([np.asarray(a[c], dtype=np.float64) for c in cols], axis=1)      # noqa: E731
    ones = np.ones(len(got["id"]), dtype=np.uint8)
    assert_table_close(tab(got), ones, tab(ref), ones, what="scan columns against the stand-in's")
    k = np.isin(got["id"], cond)
    assert k.sum() == len(cond)
    for c in ("beta.cond", "SE.cond", "pval.cond"):
        assert np.isnan(got[c][k]).all() and np.isnan(ref[c][k]).all(), c
        assert np.array_equal(np.isnan(got[c]), np.isnan(ref[c])), c
    f = np.isfinite(ref["pval.cond"]) & ~np.isin(got["id"], np.asarray(vid)[near])
    assert f.sum() >= 0.8 * f.size
    e_s = np.abs(got["SE.cond"][f] - ref["SE.cond"][f]) / (1e-8 * ref["SE.cond"][f])
    e_b = np.abs(got["beta.cond"][f] - ref["beta.cond"][f]) / (1e-8 * np.abs(ref["beta.cond"][f]) + 1e-10 * ref["SE.cond"][f])
    e_p = np.abs(got["pval.cond"][f] - ref["pval.cond"][f]) / (1e-8 * ref["pval.cond"][f])
    print("driver: SE.cond / beta.cond / pval.cond off by", e_s.max(), e_b.max(), e_p.max(), "x tolerance; rows skipped", near.size)
    assert e_s.max() <= 1 and e_b.max() <= 1 and e_p.max() <= 1


def test_9_driver_fractional_dosages():
    import torch  # noqa: F401
    from test_cond_dosage import fractional_case
    src, mod = fractional_case()
    got, ref, near = _driver_pair(src, mod, [30, 77], mac=2)
    _driver_check(got, ref, src.variant_id, near, [30, 77])


def test_9_driver_file_of_dosages():
    import torch  # noqa: F401
    from test_cond_dosage import file_case
    path, mem, mod = file_case()
    cond = [mem.variant_id[25], mem.variant_id[63]]
    got, ref, near = _driver_pair(path, mod, cond, mac=1)
    _driver_check(got, ref, mem.variant_id, near, cond)


def test_3_an_odd_count_of_entries_at_odd_n():
    """A set of 7 rows, not in block order, of a u8 block at N = 1001: the means, the index list and the flips each end
    off a 16-byte boundary, and each table still starts on one.  Phi_CC against the reference of test 1 (the set's
    rows there, of which these are 7), S_C and Phi_CC against skat on the set as one unit, bit for bit."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    c = _case(1001, "u8")
    idx = np.array([6, 0, 3, 7, 1, 5, 2], dtype=np.int32)
    with Scanner(c["sm"]) as sc, _block(sc, c["rows_c"]) as blk:
        s, covs = blk.skat([0, idx.size], idx, c["fc"][idx], c["mc"][idx])
        s_c, phi_cc = blk.cond_set(idx, c["fc"][idx], c["mc"][idx])
    assert s_c.tobytes() == s.tobytes() and phi_cc.tobytes() == covs[0].tobytes()
    R_cc = np.asarray(c["ref"]["Phi_CC"], dtype=np.float64)[np.ix_(idx, idx)]
    assert np.all(np.abs(phi_cc - R_cc) <= 1e-10 * np.sqrt(np.outer(np.diag(R_cc), np.diag(R_cc))))
