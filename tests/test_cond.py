"""The conditional scan on the host: ``cond_tests`` against the long-double reference of tests/cond_ref.py, its
collinearity rules and SPA scaling, and the driver ``seqAssocGLMM_SPA_cond`` with a numpy stand-in scanner (scan: the
CPU oracle; cond_set / cond_2bit: tests/skat_ref.py and tests/cond_ref.py in double), as tests/test_skat.py runs the
SKAT driver without a GPU."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import cond_ref as CR
import skat_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def golden_rows(n_rows):
    """The first n_rows polymorphic variants of grm1k_10k_snp.npz -> (packed, codes, tables)."""
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    codes = unpack_dosage_2bit(g["packed"][:200], 1000)
    ok = codes != 3
    s, nn = np.where(ok, codes, 0).sum(axis=1), ok.sum(axis=1)
    pick = np.flatnonzero(np.minimum(s, 2 * nn - s) > 0)[:n_rows]
    assert pick.size == n_rows
    return np.ascontiguousarray(g["packed"][pick]), codes[pick], R.tables(codes[pick])


def flat_model(trait):
    from conftest import scan_model
    return scan_model("saige_model.npz" if trait == "binary" else "saige_model_quant.npz", mac=0.0, maf=0.0, missing=1.0)


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_cond_tests_against_the_residual_row(trait):
    from saigegds_amd.cond import cond_tests
    packed, codes, lut = golden_rows(43)
    sm = flat_model(trait)
    ref = CR.cond_ref(sm, packed[3:], lut[3:], packed[:3], lut[:3])
    f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    beta, se, p = cond_tests(f(ref["S"]), f(ref["var"]), f(ref["cov"]), f(ref["S_C"]), f(ref["Phi_CC"]))
    assert np.isfinite(beta).all()
    chi, chi_ref = (beta / se) ** 2, f(ref["T"] ** 2 / ref["V"])
    err = np.abs(chi - chi_ref) / chi_ref
    print(trait, "largest relative difference of T^2 / V", err.max(), "largest share explained", float((1 - ref["V"] / ref["var"]).max()))
    assert np.all(err <= 1e-10)
    assert np.all(np.abs(beta - f(ref["T"] / ref["V"])) <= 1e-10 * np.abs(f(ref["T"] / ref["V"])) + 1e-12 * se)
    assert np.all(np.abs(1 / se ** 2 - f(ref["V"])) <= 1e-10 * f(ref["V"]))
    # the rows test 6 of tests/test_gpu_cond.py may skip
    assert int(np.sum(1 - f(ref["V"] / ref["var"]) > 0.9)) <= 4


def test_collinear_rows_and_collinear_sets():
    from saigegds_amd.cond import cond_tests
    packed, codes, lut = golden_rows(10)
    sm = flat_model("binary")
    # scanned rows: 3 ordinary ones, conditioning variant 1 itself, and its alt-major twin (codes 2 - c: the same G)
    twin = np.where(codes[1] == 3, 3, 2 - codes[1]).astype(np.uint8)
    from saigegds_amd.gds import pack_dosage_2bit
    rows = np.concatenate([packed[3:6], packed[1:2], pack_dosage_2bit(twin[None, :])])
    tabs = np.concatenate([lut[3:6], lut[1:2], R.tables(twin[None, :])])
    ref = CR.cond_ref(sm, rows, tabs, packed[:3], lut[:3], dtype=np.float64)
    beta, se, p = cond_tests(ref["S"], ref["var"], ref["cov"], ref["S_C"], ref["Phi_CC"])
    assert np.isfinite(beta[:3]).all() and np.isfinite(se[:3]).all() and np.isfinite(p[:3]).all()
    for a in (beta, se, p):
        assert np.isnan(a[3]) and np.isnan(a[4])
    # a set that holds a variant twice
    dup = CR.cond_ref(sm, rows[:3], tabs[:3], packed[[0, 1, 0]], lut[[0, 1, 0]], dtype=np.float64)
    with pytest.raises(ValueError, match="collinear"):
        cond_tests(dup["S"], dup["var"], dup["cov"], dup["S_C"], dup["Phi_CC"])


def test_spa_scale_reproduces_the_rows_own_p_value():
    from scipy.special import chdtri
    from saigegds_amd.cond import cond_tests
    S, var, p_spa = np.array([2.5, -1.0]), np.array([1.3, 0.7]), 1e-3
    d = np.array([S[0] ** 2 / (var[0] * chdtri(1.0, p_spa)), 1.0])
    phi_cc = np.array([[2.0, 0.3], [0.3, 1.0]])
    beta, se, p = cond_tests(S, var, np.zeros((2, 2)), np.array([0.4, -3.0]), phi_cc, d, np.array([1.7, 1.0]))
    assert abs(p[0] - p_spa) <= 1e-12 * p_spa
    from scipy.special import chdtrc
    assert p[1] == chdtrc(1.0, S[1] ** 2 / var[1])


# ---- the driver, no GPU -----------------------------------------------------------------------------------------

def ref_cond_scanner_factory():
    """Scanner stand-in on host memory (``torch_device = "cpu"``: the driver's tensors and the pointers it hands over
    are the host's): the oracle's scan, cond_set = skat_ref and cond_2bit = cond_ref in double."""
    from oracle.oracle import Oracle, OracleScanner

    def arr(ptr, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return np.frombuffer((C.c_char * n).from_address(ptr), dtype=dtype).reshape(shape)

    class RefCondScanner(OracleScanner):
        torch_device = "cpu"

        def __init__(self, sm):
            OracleScanner.__init__(self, sm)
            self._sm, self._set = sm, None

        def set_thresholds(self, maf, mac, missing, spa_pval):
            sm = dataclasses.replace(self._sm, maf=maf, mac=mac, missing=missing, spa_pval=spa_pval)
            Oracle.close(self)
            Oracle.__init__(self, sm)
            self._sm = sm

        def row_stride(self):
            return (self.n + 511) // 512 * 128

        def sync(self):
            pass

        def scan_2bit_dev(self, ptr, bpv, m, out_ptr, valid_ptr):
            o, v = self.scan_2bit(arr(ptr, (m, bpv), np.uint8))
            arr(out_ptr, (m, 8), np.float64)[:], arr(valid_ptr, (m,), np.uint8)[:] = o, v

        def cond_set(self, packed_c, lut_c):
            c = packed_c.shape[0]
            self._set = (np.array(packed_c), np.array(lut_c))
            S, cov = R.skat_ref(self._sm, packed_c, [0, c], np.arange(c), lut_c, dtype=np.float64)
            return S, cov[0]

        def cond_2bit(self, packed, lut):
            with np.errstate(invalid="ignore"):
                r = CR.cond_ref(self._sm, packed, lut, *self._set, dtype=np.float64)
            return r["S"], r["var"], r["cov"]

        def cond_2bit_dev(self, ptr, bpv, m, lut_ptr, score_ptr, var_ptr, cov_ptr):
            c = self._set[0].shape[0]
            s, v, cv = self.cond_2bit(arr(ptr, (m, bpv), np.uint8), arr(lut_ptr, (m, 4), np.float64))
            arr(score_ptr, (m,), np.float64)[:], arr(var_ptr, (m,), np.float64)[:], arr(cov_ptr, (m, c), np.float64)[:] = s, v, cv
    return RefCondScanner


def driver_case(trait="binary"):
    """200 golden variants, the alt-major twins of the first 20 (codes 2 - c), a monomorphic row and one without a
    genotype."""
    from conftest import load_null_model
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    codes = unpack_dosage_2bit(g["packed"][:200], 1000)
    twins = np.where(codes[:20] == 3, 3, 2 - codes[:20]).astype(np.uint8)
    extra = np.zeros((2, 1000), dtype=np.uint8)
    extra[1] = 3
    codes = np.concatenate([codes, twins, extra])
    mod = load_null_model("saige_model.npz" if trait == "binary" else "saige_model_quant.npz")
    return GenotypeSource([str(s) for s in g["sample_id"]], packed=pack_dosage_2bit(codes)), mod


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_driver_with_reference_scanner(trait, tmp_path):
    from saigegds_amd import seqAssocGLMM_SPA_cond
    from saigegds_amd.rds import read_rdata
    src, mod = driver_case(trait)
    fac = ref_cond_scanner_factory()
    ans = seqAssocGLMM_SPA_cond(src, mod, [30, 77], mac=4, verbose=False, scanner_factory=fac)
    base = ["id", "chr", "pos", "ref", "alt", "AF.alt", "mac", "num", "beta", "SE", "pval"] + (["p.norm", "converged"] if trait == "binary" else [])
    assert list(ans.keys()) == base + ["beta.cond", "SE.cond", "pval.cond"]
    ids = list(ans["id"])
    assert 221 not in ids and 222 not in ids and 30 in ids and 77 in ids
    for c in ("beta.cond", "SE.cond", "pval.cond"):
        a = ans[c]
        assert np.isnan(a[ids.index(30)]) and np.isnan(a[ids.index(77)])
        assert np.isfinite(np.delete(a, [ids.index(30), ids.index(77)])).all()
    assert np.all((ans["pval.cond"][np.isfinite(ans["pval.cond"])] > 0))
    # the alt-major twin of a variant: the same test, beta.cond of the other allele
    n_twin = 0
    for v in range(1, 21):
        if v in ids and 200 + v in ids:
            a, b = ids.index(v), ids.index(200 + v)
            n_twin += 1
            assert (ans["AF.alt"][a] > 0.5) != (ans["AF.alt"][b] > 0.5)
            assert abs(ans["beta.cond"][a] + ans["beta.cond"][b]) <= 1e-9 * abs(ans["beta.cond"][a]) + 1e-11 * ans["SE.cond"][a]
            assert abs(ans["SE.cond"][a] - ans["SE.cond"][b]) <= 1e-9 * ans["SE.cond"][a]
            assert abs(ans["pval.cond"][a] - ans["pval.cond"][b]) <= 1e-8 * ans["pval.cond"][a]
            assert np.sign(ans["beta"][a]) == -np.sign(ans["beta"][b])
    assert n_twin >= 5
    # round trip through the result file
    fn = str(tmp_path / "cond.RData")
    assert seqAssocGLMM_SPA_cond(src, mod, [30, 77], mac=4, verbose=False, scanner_factory=fac, res_savefn=fn) is None
    back = next(iter(read_rdata(fn).values()))
    for c in ("pval", "beta.cond", "pval.cond"):
        assert np.array_equal(np.asarray(back[c], dtype=np.float64), ans[c], equal_nan=True), c


def test_driver_argument_errors():
    from saigegds_amd import seqAssocGLMM_SPA_cond
    from saigegds_amd.assoc import GenotypeSource
    src, mod = driver_case()
    fac = ref_cond_scanner_factory()
    run = lambda cond, **kw: seqAssocGLMM_SPA_cond(src, mod, cond, verbose=False, scanner_factory=fac, **kw)      # noqa: E731
    for bad in ([], list(range(1, 18)), [5, 9, 5], [5, 100000]):
        with pytest.raises(ValueError, match="condition"):
            run(bad)
    with pytest.raises(ValueError, match="221"):                       # monomorphic
        run([5, 221])
    with pytest.raises(ValueError, match="222"):                       # no genotype at all
        run([222])
    with pytest.raises(ValueError, match="gds"):
        run([5], res_savefn="x.gds")
    with pytest.raises(NotImplementedError, match="Conditional analysis on dosage input is not implemented."):
        run([5], dsnode="annotation/format/DS")
    ds = GenotypeSource(src.sample_id(), dosage=np.zeros((4, 1000)))
    with pytest.raises(NotImplementedError, match="Conditional analysis on dosage input is not implemented."):
        seqAssocGLMM_SPA_cond(ds, mod, [1], verbose=False, scanner_factory=fac)
    with pytest.raises(TypeError):
        run([5], mac="4")


def test_file_driver_equals_in_memory_driver():
    from conftest import load_null_model
    from saigegds_amd import GenotypeSource, seqAssocGLMM_SPA_cond
    from saigegds_amd.gds import GdsFile
    path = os.path.join(GOLD, "grm1k_10k_snp.gds")
    f = GdsFile(path)
    vid = np.asarray(f.read("variant.id"))
    mod = load_null_model("saige_model.npz")
    fac = ref_cond_scanner_factory()
    cond = [vid[11], vid[402]]
    a = seqAssocGLMM_SPA_cond(path, mod, cond, verbose=False, scanner_factory=fac)
    src = GenotypeSource(f.sample_id(), packed=f.dosage_alt_packed_range(0, vid.size), variant_id=vid,
                         chromosome=list(f.read("chromosome")), position=f.read("position"))
    b = seqAssocGLMM_SPA_cond(src, mod, cond, verbose=False, scanner_factory=fac)
    for c in ("id", "AF.alt", "mac", "num", "beta", "SE", "pval", "p.norm", "converged", "beta.cond", "SE.cond", "pval.cond"):
        assert np.array_equal(np.asarray(a[c]), np.asarray(b[c]), equal_nan=True), c
    assert np.isfinite(a["pval.cond"]).sum() > 0.9 * a["pval.cond"].size
