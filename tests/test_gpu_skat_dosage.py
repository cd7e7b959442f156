"""sgx_ds_block_skat and seqAssocGLMM_spaSKAT on dosage input on the device: the kernel against the long-double
reference of tests/skat_ds_ref.py, the identities that tie S and Phi to the pinned scan and burden paths of the same
resident rows and to sgx_skat_2bit, determinism, the error paths, and the driver against its run with the numpy
stand-in.  Models as in tests/test_gpu_skat.py: the golden models at N = 1000, synth_null_model otherwise.  N = 70001
is odd (u8 rows start at odd addresses, f64 rows off the 16-byte lines) and spans 18 sample slabs of 4096."""

import numpy as np
import pytest

import skat_ds_ref as D
import skat_ref as R
from test_gpu_skat import _flat, _model, check

pytestmark = pytest.mark.gpu
NA_INT = np.iinfo(np.int32).min
_cache = {}


def _rows(n, kind, m=40):
    """(rows, flip, mean).  f64: the hard calls of skat_ref.hard_calls (1 % missing, every 7th row alt-major), 30 % of
    the genotypes blurred, flip and mean as the driver forms them (the alt-major rows are the flipped ones).  u8 / i32:
    values 0..200, 1 % missing; every 7th entry flipped, the mean flipped with it."""
    rng = np.random.default_rng(17 + n)
    if kind == "f64":
        codes = R.hard_calls(n, m, 11 + n)
        x = np.where(codes == 3, np.nan, codes.astype(np.float64))
        rows = np.clip(x + rng.normal(0, 0.08, x.shape) * (rng.random(x.shape) < 0.3), 0, 2)
        flip, mean = D.flip_mean(rows)
        assert flip[::7].all() and not flip[1:7].any()
        return rows, flip, mean
    v = rng.integers(0, 201, (m, n))
    miss = rng.random((m, n)) < 0.01
    rows = np.where(miss, 0xFF, v).astype(np.uint8) if kind == "u8" else np.where(miss, NA_INT, v).astype(np.int32)
    mu = np.where(miss, 0, v).sum(axis=1) / (~miss).sum(axis=1)
    flip = (np.arange(m) % 7 == 0).astype(np.uint8)
    return rows, flip, np.where(flip != 0, 2 - mu, mu)


def _case(n, kind):
    """Per (N, row type), made once: model, 40 rows, flip, mean, the long-double reference of the 40 as one unit."""
    if (n, kind) not in _cache:
        sm = _model(n)
        rows, flip, mean = _rows(n, kind)
        S, cov = D.skat_ds_ref(sm, rows, [0, 40], np.arange(40), flip, mean)
        _cache[(n, kind)] = (sm, rows, flip, mean, S, cov[0])
    return _cache[(n, kind)]


def _block(sc, rows):
    blk = sc.dosage_block(rows.dtype, rows.shape[0])
    blk.load(rows)
    return blk


@pytest.mark.parametrize("m", [1, 15, 16, 17, 40])
@pytest.mark.parametrize("n", [1000, 70001])
@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_1_kernel_against_the_reference(kind, n, m):
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    sm, rows, flip, mean, S, cov = _case(n, kind)
    with Scanner(sm) as sc, _block(sc, rows) as blk:
        score, covs = blk.skat([0, m], np.arange(m), flip[:m], mean[:m])
    assert len(covs) == 1
    check(score, covs[0], S[:m], cov[:m, :m], f"{kind} N={n} m={m}")


def test_1_i32_block():
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    sm, rows, flip, mean, S, cov = _case(1000, "i32")
    with Scanner(sm) as sc, _block(sc, rows) as blk:
        score, covs = blk.skat([0, 17], np.arange(17), flip[:17], mean[:17])
    check(score, covs[0], S[:17], cov[:17, :17], "i32 N=1000 m=17")


@pytest.mark.parametrize("k", [3, 8, 16])
@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_2_dense_column_tiles(trait, k):
    """2K + 1 dense columns = 7 / 17 / 33: below one tile, one over one tile, one over two."""
    import torch  # noqa: F401
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    n, m = 1000, 17
    sm = _flat(synth.synth_null_model(n, trait, 0.2, n_cov=k, seed=20260 + k))
    assert sm.k == k
    with Scanner(sm) as sc:
        for kind in ("f64", "u8"):
            rows, flip, mean = _rows(n, kind, m)
            S, cov = D.skat_ds_ref(sm, rows, [0, m], np.arange(m), flip, mean)
            with _block(sc, rows) as blk:
                score, covs = blk.skat([0, m], np.arange(m), flip, mean)
            check(score, covs[0], S, cov[0], f"{trait} K={k} {kind}")


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_3_ties_to_the_block_scan(trait):
    """chdtrc(1, S_j^2 / Phi_jj) = the pval_noadj of blk.scan() on the same resident rows (binary: column 6,
    quantitative: column 5): the first 64 fractional rows of the golden set with mac > 0."""
    import torch  # noqa: F401
    from scipy.special import chdtrc
    from saigegds_amd._lib import Scanner
    from test_skat_dosage import fractional_case
    ds, _, _ = fractional_case()
    ok = np.isfinite(ds)
    s, nn = np.where(ok, ds, 0.0).sum(axis=1), ok.sum(axis=1)
    pick = np.flatnonzero(np.minimum(s, 2 * nn - s) > 0)[:64]
    assert pick.size == 64
    rows = np.ascontiguousarray(ds[pick])
    assert np.any(rows[ok[pick]] % 1 != 0)
    flip, mean = D.flip_mean(rows)
    sm = _model(1000, trait)
    with Scanner(sm) as sc, _block(sc, rows) as blk:
        out, valid = blk.scan()
        score, covs = blk.skat([0, 64], np.arange(64), flip, mean)
    assert valid.all()
    p = chdtrc(1.0, score ** 2 / np.diag(covs[0]))
    ref = out[:, 5 if sm.quant else 6]
    err = np.abs(p - ref) / ref
    print(trait, "largest relative difference to the scan's pval_noadj", err.max())
    assert np.all(err <= 1e-10)


def test_4_ties_to_the_burden_path():
    """(sum w_j S_j)^2 / (w' Phi w) = qchisq(p.norm) of the row blk.burden makes with the same flip and mw = mean w;
    units of 8 variants, those whose collapsed row the scan does not flip."""
    import torch  # noqa: F401
    from scipy.special import chdtri
    from saigegds_amd._lib import Scanner
    sm, rows, flip, mean, _, _ = _case(1000, "f64")
    rng = np.random.default_rng(4)
    w = rng.random(40) / 8
    ptr = np.arange(0, 41, 8)
    with Scanner(sm) as sc, _block(sc, rows) as blk:
        score, covs = blk.skat(ptr, np.arange(40), flip, mean)
        out, valid = blk.burden(ptr, np.arange(40, dtype=np.int32), flip, w[:, None], (mean * w)[:, None])
    good = 0
    for u in range(5):
        r = slice(8 * u, 8 * u + 8)
        if not valid[u] or not out[u, 0] <= 0.5:
            continue
        good += 1
        chi = float(np.sum(w[r] * score[r])) ** 2 / float(w[r] @ covs[u] @ w[r])
        ref = chdtri(1.0, out[u, 6])
        print("unit", u, chi, ref, abs(chi - ref) / ref)
        assert abs(chi - ref) <= 1e-9 * ref
    assert good >= 4


@pytest.mark.parametrize("n", [1000, 70001])
def test_5_ties_to_skat_2bit(n):
    """Hard calls in a u8 block and in an f64 block against sgx_skat_2bit on the packed codes, tolerance of test 1."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    sm = _model(n)
    codes = R.hard_calls(n, 40, 11 + n)
    lut = R.tables(codes)
    u8 = np.where(codes == 3, 0xFF, codes).astype(np.uint8)
    f64 = np.where(codes == 3, np.nan, codes.astype(np.float64))
    flip, mean = D.flip_mean(u8)
    assert flip.any() and not flip.all()
    with Scanner(sm) as sc:
        S2, c2 = sc.skat_2bit(pack_dosage_2bit(codes), [0, 40], np.arange(40), lut)
        for rows in (u8, f64):
            with _block(sc, rows) as blk:
                score, covs = blk.skat([0, 40], np.arange(40), flip, mean)
            check(score, covs[0], S2, c2[0], f"N={n} {rows.dtype} block against the 2-bit call")


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_6_determinism(kind):
    import torch  # noqa: F401
    from conftest import REL_TOL
    from saigegds_amd._lib import Scanner
    sm, rows, flip, mean, _, _ = _case(70001, kind)
    rng = np.random.default_rng(9)
    units = [rng.permutation(40)[:k] for k in (3, 16, 17, 40, 9)]

    def call(blk, order, mean=mean):
        idx = np.concatenate([units[u] for u in order])
        ptr = np.concatenate([[0], np.cumsum([units[u].size for u in order])])
        score, covs = blk.skat(ptr, idx, flip[idx], mean[idx])
        return {u: (score[ptr[k]:ptr[k + 1]].copy(), covs[k].copy()) for k, u in enumerate(order)}
    with Scanner(sm) as sc, _block(sc, rows) as blk:
        together = call(blk, [0, 1, 2, 3, 4])
        again = call(blk, [0, 1, 2, 3, 4])
        rev = call(blk, [4, 3, 2, 1, 0])
        alone = {u: call(blk, [u])[u] for u in range(5)}
        # a unit that repeats a variant
        rep = np.array([5, 11, 5])
        s2, c2 = blk.skat([0, 3], rep, flip[rep], mean[rep])
        # an entry with a NaN mean (its row has missing values): non-finite for itself only
        bad = int(units[2][4])
        assert (rows[bad] == 0xFF).any() if kind == "u8" else np.isnan(rows[bad]).any()
        nan_mean = mean.copy()
        nan_mean[bad] = np.nan
        poisoned = call(blk, [2, 1], nan_mean)
    for u in range(5):
        for other, what in ((again, "twice"), (rev, "reverse order"), (alone, "alone")):
            assert together[u][0].tobytes() == other[u][0].tobytes(), (u, what)
            assert together[u][1].tobytes() == other[u][1].tobytes(), (u, what)
            assert np.array_equal(other[u][1], other[u][1].T), (u, what)
    # the repeated entry: the same operands give the same bits.  Phi[0, 1] and Phi[2, 1] (the mirror of [1, 2]) are the
    # same sum with the weight mu2 on the other factor, (g_a mu2) g_b against (g_b mu2) g_a: products of real-valued
    # dosages round differently, so these two agree within the tolerance of test 1, not bit for bit
    c = c2[0]
    assert c[0, 2] == c[0, 0] == c[2, 2] and s2[0] == s2[2] and np.array_equal(c, c.T)
    assert abs(c[0, 1] - c[2, 1]) <= REL_TOL * np.sqrt(c[0, 0] * c[1, 1])
    assert np.isfinite(c).all() and c[0, 0] > 0
    for u in (2, 1):
        hit = units[u] == bad
        assert hit.sum() == 1 or u == 1
        s, cv = poisoned[u]
        touched = hit[:, None] | hit[None, :]
        assert not np.isfinite(s[hit]).any() and not np.isfinite(cv[touched]).any(), u
        assert s[~hit].tobytes() == together[u][0][~hit].tobytes(), u
        assert cv[~touched].tobytes() == together[u][1][~touched].tobytes(), u


def test_7_errors_leave_the_handle_usable():
    import torch  # noqa: F401
    from saigegds_amd import _lib
    from saigegds_amd._lib import SKAT_MAX_VARIANTS, Scanner, SgxError
    L = _lib.load()
    sm, rows, flip, mean, S, cov = _case(1000, "f64")
    with Scanner(sm) as sc, _block(sc, rows) as blk:
        idx = np.arange(4, dtype=np.int32)
        fl, mn = np.ascontiguousarray(flip[:4]), np.ascontiguousarray(mean[:4])
        score, cv = np.zeros(4), np.zeros(16)
        big = np.array([0, SKAT_MAX_VARIANTS + 1], dtype=np.int64)         # only unit_ptr is large: nothing is read through it
        ptr = np.array([0, 4], dtype=np.int64)
        good = [ptr.ctypes.data, idx.ctypes.data, fl.ctypes.data, mn.ctypes.data, score.ctypes.data, cv.ctypes.data]
        assert L.sgx_ds_block_skat(sc._h, blk._b, 1, big.ctypes.data, *good[1:]) == -1
        assert b"at most" in L.sgx_last_error()
        for k in range(6):
            args = list(good)
            args[k] = None
            assert L.sgx_ds_block_skat(sc._h, blk._b, 1, *args) == -1, k
            assert b"NULL" in L.sgx_last_error()
        assert L.sgx_ds_block_skat(None, blk._b, 1, *good) == -1 and L.sgx_ds_block_skat(sc._h, None, 1, *good) == -1
        with pytest.raises(SgxError, match="out of range") as ei:
            blk.skat([0, 4], np.array([0, 1, 40, 2]), flip[:4], mean[:4])          # index >= M
        assert ei.value.code == -1
        with pytest.raises(SgxError, match="out of range"):
            blk.skat([0, 4], np.array([0, -1, 3, 2]), flip[:4], mean[:4])
        with _block(sc, rows[:8]) as small:                                        # M below the block's other rows
            with pytest.raises(SgxError, match="out of range"):
                small.skat([0, 2], [0, 8], flip[:2], mean[:2])
        assert not score.any() and not cv.any()
        # a unit of 0 entries writes nothing
        s0, c0 = blk.skat([0, 0, 2, 2], [3, 4], flip[3:5], mean[3:5])
        assert s0.shape == (2,) and [c.shape for c in c0] == [(0, 0), (2, 2), (0, 0)]
        # the handle still works
        s1, c1 = blk.skat([0, 1], [0], flip[:1], mean[:1])
    check(s1, c1[0], S[:1], cov[:1, :1], "after the errors: N=1000 m=1")
    check(s0, c0[1], S[3:5], cov[3:5, 3:5], "a unit between two empty ones")


def test_8_driver_fractional_f64_in_batches(monkeypatch):
    """The fractional float64 case of tests/test_skat_dosage.py in batches of at most 60 resident rows against the
    driver's run with the numpy stand-in."""
    import torch  # noqa: F401
    from saigegds_amd import _lib, seqAssocGLMM_spaSKAT
    from saigegds_amd.assoc import GenotypeSource
    from test_skat_dosage import _model as host_model, close, fractional_case
    ds, sid, units = fractional_case()
    mod = host_model("binary")
    src = GenotypeSource(sid, dosage=ds)
    loads, load = [], _lib.DosageBlock.load
    monkeypatch.setattr(_lib.DosageBlock, "load", lambda self, rows: (loads.append(rows.shape[0]), load(self, rows))[1])
    got = seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, ds_budget=60 * 8000)
    assert len(loads) >= 3 and max(loads) <= 82
    ref = seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, scanner_factory=D.NumpySkatDsScanner)
    assert list(got.keys()) == list(ref.keys())
    for c in ("numvar", "n.var"):
        assert np.array_equal(got[c], ref[c]), c
    assert list(got["n.var"][[2, 3]]) == [0, 0] and (got["n.var"][[0, 1, 4, 5]] > 20).all()
    for c in ("Q.b1_1", "pval.b1_1", "Q.b1_25", "pval.b1_25", "maf.avg", "mac.avg"):
        close(got[c], ref[c], 1e-9, c)
    assert np.isfinite(got["pval.b1_25"][[0, 1, 4, 5]]).all()


def test_8_driver_on_a_packed_real_file(tmp_path):
    """seqAssocGLMM_spaSKAT on a written file with a dPackedReal16U node and no genotype node (1103 samples, the model's
    1000 among them in another order; rows decoded on the device by load_packed) equals the call on
    GenotypeSource(dosage = decoded rows) exactly, in one batch and in batches of 30 rows."""
    import torch  # noqa: F401
    import aggregate_ds_ref as A
    import packed_ds_cases as P
    from saigegds_amd import seqAssocGLMM_spaSKAT
    from saigegds_amd.assoc import GenotypeSource
    cls = "dPackedReal16U"
    _, _, scale, offset = P.CLASSES[cls]
    mod = A.golden_model()
    m = 96
    codes, _ = P.golden_codes(m)
    raw = P.stored_rows(cls, P.dosages(m, 1000, 21, codes))
    wide, sel = P.widen(raw, 1103, 4)
    sid = [f"x{i}" for i in range(1103)]
    for k, s in enumerate(sel):
        sid[s] = str(mod.sample_id[k])
    path = P.write_ds_file(tmp_path / "ds16.gds", wide, cls, scale, offset, sid)
    units = [np.arange(s, s + 12) + 1 for s in range(0, m, 12)]
    src = GenotypeSource(sid, dosage=P.decode(wide, cls, scale, offset))
    for budget in (None, 30 * 8000):
        a = seqAssocGLMM_spaSKAT(path, mod, units, verbose=False, ds_budget=budget)
        b = seqAssocGLMM_spaSKAT(src, mod, units, verbose=False, ds_budget=budget)
        A.same_dicts(a, b, f"budget {budget}")
        assert np.isfinite(a["pval.b1_25"]).sum() >= len(units) // 2 and (a["n.var"] > 0).sum() >= len(units) // 2


def test_9_an_odd_count_of_entries_at_odd_n():
    """15 entries, not in block order, of a u8 block at N = 1001: the index list, the means and the flips each end off
    a 16-byte boundary, and each table still starts on one.  Against the reference of test 1."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    sm, rows, flip, mean, S, cov = _case(1001, "u8")
    idx = np.random.default_rng(15).permutation(40)[:15].astype(np.int32)
    with Scanner(sm) as sc, _block(sc, rows) as blk:
        score, covs = blk.skat([0, 15], idx, flip[idx], mean[idx])
    check(score, covs[0], S[idx], cov[np.ix_(idx, idx)], "u8 N=1001, 15 entries")
