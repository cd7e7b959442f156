"""sgx_skat_2bit and seqAssocGLMM_spaSKAT on the device: the kernel against the long-double reference of
tests/skat_ref.py, the identities that tie S and Phi to the pinned scan and burden paths, determinism, the error
paths, and the driver against its run with the reference scanner (tests/test_skat.py).  Models and genotypes as in
tests/test_gpu_aggregate_dosage.py: the golden models at N = 1000, synth_null_model otherwise; hard calls with 1 %
missing, every 7th row alt-major."""
import ctypes as C
import os

import numpy as np
import pytest

import skat_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
_cache = {}


def _flat(mod):
    from saigegds_amd.nullmod import init_nullmod
    return init_nullmod(mod, np.arange(len(mod.sample_id)), 0.0, 0.0, 1.0, 0.05, float(np.nanmean(mod.var_ratio)))


def _model(n, trait="binary"):
    from conftest import load_null_model
    from saigegds_amd import synth
    if n == 1000:
        return _flat(load_null_model("saige_model.npz" if trait == "binary" else "saige_model_quant.npz"))
    return _flat(synth.synth_null_model(n, trait, 0.05, n_cov=3, seed=20260))


def _case(n):
    """Per N, made once: model, 40 rows of hard calls, their tables, the long-double reference of the 40 as one unit."""
    if n not in _cache:
        from saigegds_amd.gds import pack_dosage_2bit
        sm = _model(n)
        codes = R.hard_calls(n, 40, 11 + n)
        packed, lut = pack_dosage_2bit(codes), R.tables(codes)
        S, cov = R.skat_ref(sm, packed, [0, 40], np.arange(40), lut)
        _cache[n] = (sm, packed, lut, S, cov[0])
    return _cache[n]


def check(score, cov, S_ref, cov_ref, what):
    """|dPhi_jl| <= 1e-10 sqrt(Phi_jj Phi_ll), |dS_j| <= 1e-10 |S_j| + 1e-12 sqrt(Phi_jj): REL_TOL / Z_FLOOR of conftest.
    The Phi bound is derived, not measured: a double sum of N non-negative terms is off by at most N 2^-53 of itself
    and W_jj / var2_jj <= 3: 2.3e-11 at N = 70 001."""
    from conftest import REL_TOL, Z_FLOOR
    S_ref, cov_ref = np.asarray(S_ref, dtype=np.longdouble), np.asarray(cov_ref, dtype=np.longdouble)
    assert score.shape == S_ref.shape and cov.shape == cov_ref.shape, what
    assert np.array_equal(cov, cov.T), f"{what}: cov is not exactly symmetric"
    sd = np.sqrt(np.diag(cov_ref))
    e_phi = np.abs(cov - cov_ref) / (REL_TOL * sd[:, None] * sd[None, :])
    e_s = np.abs(score - S_ref) / (REL_TOL * np.abs(S_ref) + Z_FLOOR * sd)
    print(f"{what}: Phi off by {float(e_phi.max()):.3g} x tolerance, S by {float(e_s.max()):.3g} x")
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(score)), what
    assert float(e_phi.max()) <= 1.0 and float(e_s.max()) <= 1.0, what


@pytest.mark.parametrize("m", [1, 15, 16, 17, 40])
@pytest.mark.parametrize("n", [1000, 70001])
def test_1_kernel_against_the_reference(n, m):
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    sm, packed, lut, S, cov = _case(n)
    with Scanner(sm) as sc:
        score, covs = sc.skat_2bit(packed, [0, m], np.arange(m), lut[:m])
    assert len(covs) == 1
    check(score, covs[0], S[:m], cov[:m, :m], f"N={n} m={m}")


@pytest.mark.parametrize("k", [3, 8, 16])
@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_2_dense_column_tiles(trait, k):
    """2K + 1 dense columns = 7 / 17 / 33: below one tile, one over one tile, one over two."""
    import torch  # noqa: F401
    from saigegds_amd import synth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    n, m = 1000, 17
    sm = _flat(synth.synth_null_model(n, trait, 0.2, n_cov=k, seed=20260 + k))
    assert sm.k == k
    codes = R.hard_calls(n, m, 5 + k)
    packed, lut = pack_dosage_2bit(codes), R.tables(codes)
    S, cov = R.skat_ref(sm, packed, [0, m], np.arange(m), lut)
    with Scanner(sm) as sc:
        score, covs = sc.skat_2bit(packed, [0, m], np.arange(m), lut)
    check(score, covs[0], S, cov[0], f"{trait} K={k}")


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_3_ties_to_the_pinned_scan(trait):
    """chdtrc(1, S_j^2 / Phi_jj) = the pval_noadj of Scanner.scan_2bit on the same rows (binary: column 6,
    quantitative: column 5), first 64 variants of grm1k_10k_snp.npz with mac > 0."""
    import torch  # noqa: F401
    from scipy.special import chdtrc
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    codes = unpack_dosage_2bit(g["packed"][:200], 1000)
    ok = codes != 3
    s, nn = np.where(ok, codes, 0).sum(axis=1), ok.sum(axis=1)
    pick = np.flatnonzero(np.minimum(s, 2 * nn - s) > 0)[:64]
    assert pick.size == 64
    packed = np.ascontiguousarray(g["packed"][pick])
    lut = R.tables(codes[pick])
    sm = _model(1000, trait)
    with Scanner(sm) as sc:
        out, valid = sc.scan_2bit(packed)
        score, covs = sc.skat_2bit(packed, [0, 64], np.arange(64), lut)
    assert valid.all()
    p = chdtrc(1.0, score ** 2 / np.diag(covs[0]))
    ref = out[:, 5 if sm.quant else 6]
    err = np.abs(p - ref) / ref
    print(trait, "largest relative difference to the scan's pval_noadj", err.max())
    assert np.all(err <= 1e-10)


def test_4_ties_to_the_burden_path():
    """(sum w_j S_j)^2 / (w' Phi w) = qchisq(p.norm) of the row burden_2bit makes from lut * w; units of 8 variants,
    those whose collapsed row the scan does not flip."""
    import torch  # noqa: F401
    from scipy.special import chdtri
    from saigegds_amd._lib import Scanner
    sm, packed, lut, _, _ = _case(1000)
    rng = np.random.default_rng(4)
    w = rng.random(40) / 8
    ptr = np.arange(0, 41, 8)
    with Scanner(sm) as sc:
        score, covs = sc.skat_2bit(packed, ptr, np.arange(40), lut)
        out, valid = sc.burden_2bit(packed, ptr, np.arange(40, dtype=np.int32), lut * w[:, None])
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


def test_5_determinism():
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    sm, packed, lut, _, _ = _case(70001)
    rng = np.random.default_rng(9)
    units = [rng.permutation(40)[:k] for k in (3, 16, 17, 40, 9)]

    def call(sc, order):
        idx = np.concatenate([units[u] for u in order])
        ptr = np.concatenate([[0], np.cumsum([units[u].size for u in order])])
        score, covs = sc.skat_2bit(packed, ptr, idx, lut[idx])
        return {u: (score[ptr[k]:ptr[k + 1]].copy(), covs[k].copy()) for k, u in enumerate(order)}
    with Scanner(sm) as sc:
        together = call(sc, [0, 1, 2, 3, 4])
        again = call(sc, [0, 1, 2, 3, 4])
        rev = call(sc, [4, 3, 2, 1, 0])
        alone = {u: call(sc, [u])[u] for u in range(5)}
        # a unit that repeats a variant
        rep = np.array([5, 11, 5])
        s2, c2 = sc.skat_2bit(packed, [0, 3], rep, lut[rep])
    for u in range(5):
        for other, what in ((again, "twice"), (rev, "reverse order"), (alone, "alone")):
            assert together[u][0].tobytes() == other[u][0].tobytes(), (u, what)
            assert together[u][1].tobytes() == other[u][1].tobytes(), (u, what)
    c = c2[0]
    assert c[0, 2] == c[0, 0] == c[2, 2] and c[0, 1] == c[2, 1] and s2[0] == s2[2]
    assert np.isfinite(c).all() and c[0, 0] > 0


def test_6_errors_leave_the_handle_usable():
    import torch  # noqa: F401
    from saigegds_amd import _lib
    from saigegds_amd._lib import SKAT_MAX_VARIANTS, Scanner, SgxError
    L = _lib.load()
    sm, packed, lut, S, cov = _case(1000)
    with Scanner(sm) as sc:
        idx = np.arange(4, dtype=np.int32)
        score, cv = np.zeros(4), np.zeros(16)
        big = np.array([0, SKAT_MAX_VARIANTS + 1], dtype=np.int64)         # only unit_ptr is large: nothing is read through it
        args = (sc._h, packed.ctypes.data, packed.shape[1], packed.shape[0], 1)
        assert L.sgx_skat_2bit(*args, big.ctypes.data, idx.ctypes.data, lut.ctypes.data, score.ctypes.data, cv.ctypes.data) == -1
        assert b"at most" in L.sgx_last_error()
        with pytest.raises(SgxError, match="out of range") as ei:
            sc.skat_2bit(packed, [0, 4], np.array([0, 1, 40, 2]), lut[:4])
        assert ei.value.code == -1
        ptr = np.array([0, 4], dtype=np.int64)
        assert L.sgx_skat_2bit(*args, ptr.ctypes.data, idx.ctypes.data, lut.ctypes.data, None, cv.ctypes.data) == -1
        assert b"NULL" in L.sgx_last_error()
        assert L.sgx_skat_2bit(*args, ptr.ctypes.data, idx.ctypes.data, lut.ctypes.data, score.ctypes.data, None) == -1
        # a unit of 0 entries writes nothing
        s0, c0 = sc.skat_2bit(packed, [0, 0, 2, 2], [3, 4], lut[3:5])
        assert s0.shape == (2,) and [c.shape for c in c0] == [(0, 0), (2, 2), (0, 0)]
        # the handle still works
        s1, c1 = sc.skat_2bit(packed, [0, 1], [0], lut[:1])
    check(s1, c1[0], S[:1], cov[:1, :1], "after the errors: N=1000 m=1")


def test_7_driver_end_to_end():
    """grm1k_10k_snp.gds, 20 units of 5-40 consecutive variants, against the driver with the reference scanner."""
    import torch  # noqa: F401
    from conftest import load_null_model
    from saigegds_amd import seqAssocGLMM_spaSKAT
    from test_skat import close, ref_scanner_factory
    path = os.path.join(GOLD, "grm1k_10k_snp.gds")
    mod = load_null_model("saige_model.npz")
    rng = np.random.default_rng(7)
    sizes = rng.integers(5, 41, 20)
    sizes[0], sizes[1] = 5, 40
    starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    units = [np.arange(a, a + k) + 1 for a, k in zip(starts, sizes)]
    got = seqAssocGLMM_spaSKAT(path, mod, units, verbose=False)
    ref = seqAssocGLMM_spaSKAT(path, mod, units, verbose=False, scanner_factory=ref_scanner_factory())
    assert list(got.keys()) == list(ref.keys())
    for c in ("numvar", "n.var"):
        assert np.array_equal(got[c], ref[c]), c
    assert (got["n.var"] > 0).all()
    for c in ("Q.b1_1", "pval.b1_1", "Q.b1_25", "pval.b1_25", "maf.avg", "mac.avg"):
        close(got[c], ref[c], 1e-9, c)
    assert np.isfinite(got["pval.b1_25"]).all()


def test_8_rows_uploaded_in_chunks():
    """sgx_skat_2bit sends its rows up in chunks of pipe_mb MiB at the device stride 4 ceil(N / 16): 17 504 bytes at
    N = 70 001, so pipe_mb = 1 is 59 rows a chunk.  60 rows (a chunk and one row) and 125 (two chunks and a tail of 7,
    not a multiple of 16), two units whose entries point across the chunks, give the bits of the one-chunk call."""
    import torch  # noqa: F401
    from saigegds_amd._lib import Scanner
    from saigegds_amd.gds import pack_dosage_2bit
    n = 70001
    sm = _case(n)[0]
    codes = R.hard_calls(n, 125, 31 + n)
    packed, lut = pack_dosage_2bit(codes), R.tables(codes)
    assert (1 << 20) // (4 * ((n + 15) // 16)) == 59
    with Scanner(sm) as sc:
        try:
            for rows, cut in ((60, 17), (125, 40)):
                idx = np.random.default_rng(rows).permutation(rows)
                got = {}
                for pipe_mb in (0, 1):
                    sc.set_option("pipe_mb", pipe_mb)
                    got[pipe_mb] = sc.skat_2bit(packed[:rows], [0, cut, rows], idx, lut[idx])
                assert np.isfinite(got[0][0]).all()
                assert got[0][0].tobytes() == got[1][0].tobytes(), rows
                for a, b in zip(got[0][1], got[1][1]):
                    assert a.tobytes() == b.tobytes(), rows
        finally:
            sc.set_option("pipe_mb", 0)
