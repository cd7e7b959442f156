"""Collapsing of ultra-rare variants without a GPU: the numpy reference tests/collapse_ref.py against a
plain loop, the drivers ``seqAssocGLMM_spaSKAT`` / ``seqAssocGLMM_spaSKATO`` with ``collapse_mac`` through a stand-in
scanner (scan: the CPU oracle; skat_2bit: tests/skat_ref.py; collapse_2bit: the reference), their refusals, the default,
and the checks of the C entry's groups as a stand-alone program under -fsanitize=address,undefined."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import collapse_ref as CR
import skat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("n.var", "Q", "pval", "pval.SKAT", "pval.burden", "rho.min", "n.iter")     # columns compared bit for bit


def loop_ref(codes, grp_ptr, var_idx, flip):
    """The definition, one sample at a time."""
    n = codes.shape[1]
    rows, counts = [], []
    for g in range(len(grp_ptr) - 1):
        top = [0] * n
        for e in range(grp_ptr[g], grp_ptr[g + 1]):
            for i in range(n):
                c = int(codes[var_idx[e], i])
                d = 0 if c == 3 else (2 - c if flip[e] else c)
                top[i] = max(top[i], d)
        rows.append(top)
        counts.append([top.count(1), top.count(2)])
    return np.array(rows, dtype=np.uint8).reshape(len(grp_ptr) - 1, n), np.array(counts, dtype=np.int32).reshape(-1, 2)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_reference_against_a_plain_loop(n):
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 4, (7, n)).astype(np.uint8)
    codes[5] = 3                                                # a row that is all missing
    grp_ptr, var_idx = [0, 0, 1, 3, 8, 9], np.array([2, 0, 1, 6, 5, 4, 3, 2, 5])
    flip = np.array([0, 1, 0, 1, 1, 0, 0, 1, 1], dtype=np.uint8)
    packed = np.concatenate([pack_dosage_2bit(codes), np.full((7, 2), 0xFF, dtype=np.uint8)], axis=1)   # two more bytes a row
    if n % 4:
        packed[:, (n + 3) // 4 - 1] |= np.uint8((0xFF << (2 * (n % 4))) & 0xFF)      # garbage beyond sample n - 1
    rows, counts = CR.collapse_ref(packed, n, grp_ptr, var_idx, flip)
    want, want_counts = loop_ref(codes, grp_ptr, var_idx, flip)
    assert rows.shape == (5, packed.shape[1]) and rows.dtype == np.uint8 and counts.dtype == np.int32
    assert np.array_equal(unpack_dosage_2bit(rows, n), want) and np.array_equal(counts, want_counts)
    assert np.array_equal(rows[:, :(n + 3) // 4], pack_dosage_2bit(want)) and not rows[:, (n + 3) // 4:].any()   # zero padding
    assert not rows[0].any() and not counts[0].any()            # a group of no entries
    assert not rows[4].any() and not counts[4].any()            # the all-missing row, flipped: still nothing
    assert want.max() <= 2


def ref_scanner_factory(collapse=True):
    """Scanner stand-in: the oracle's scan, skat_2bit = skat_ref in double and (``collapse``) collapse_2bit = collapse_ref;
    counts the collapse_2bit calls and the scanners closed."""
    from oracle.oracle import OracleScanner

    class RefScanner(OracleScanner):
        calls = closed = 0

        def __init__(self, sm):
            OracleScanner.__init__(self, sm)
            self._sm, self._open = sm, 1

        def skat_2bit(self, packed, unit_ptr, var_idx, lut):
            return R.skat_ref(self._sm, packed, unit_ptr, var_idx, lut, dtype=np.float64)

        def close(self):
            RefScanner.closed += self._open                     # (the oracle closes itself once more when it is deleted)
            self._open = 0
            OracleScanner.close(self)

    def collapse_2bit(self, packed, grp_ptr, var_idx, flip):
        RefScanner.calls += 1
        return CR.collapse_ref(packed, self.n, grp_ptr, var_idx, flip)
    if collapse:
        RefScanner.collapse_2bit = collapse_2bit
    return RefScanner


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_against_stored(driver, trait, scanner_factory, **kw):
    """``driver(collapse_mac=10)`` against the same driver without it on ``stored_case``'s source: bit for bit on the
    columns of EXACT; ``n.collapsed`` and ``mac.collapsed`` against the reference; the summary columns those of the
    original units."""
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import pack_dosage_2bit
    codes, mod, units, ids = CR.driver_case(trait)
    codes2, units2, n_coll, pseudo = CR.stored_case(codes, units, 10)
    got = driver(GenotypeSource(ids, packed=pack_dosage_2bit(codes)), mod, units, verbose=False, collapse_mac=10,
                 scanner_factory=scanner_factory, **kw)
    want = driver(GenotypeSource(ids, packed=pack_dosage_2bit(codes2)), mod, units2, verbose=False,
                  scanner_factory=scanner_factory, **kw)
    plain = driver(GenotypeSource(ids, packed=pack_dosage_2bit(codes)), mod, units, verbose=False,
                   scanner_factory=scanner_factory, **kw)
    assert [k for k in got if k not in ("n.collapsed", "mac.collapsed")] == list(want) == list(plain)
    cols = [c for c in want if c.split(".b")[0] in EXACT]
    assert {"n.var"} < set(cols) and any(c.startswith("pval") for c in cols) and any(c.startswith("Q") for c in cols)
    for c in cols:
        assert same_bits(got[c], want[c]), (c, got[c], want[c])
    assert list(got["n.collapsed"]) == list(n_coll) and got["n.collapsed"].dtype == np.int64
    mac = [math.nan if p is None else float(CR.counts_of(p[None, :])[2][0]) for p in pseudo]
    assert np.array_equal(got["mac.collapsed"], mac, equal_nan=True)
    # every unit shape occurs, and collapsing changed the test where it had something to collapse
    assert n_coll[5] == 0 and n_coll[4] == 1 and n_coll[1] >= 1 and n_coll[3] == 18 and n_coll[2] >= 11
    assert list(got["n.var"][[3, 4, 5]]) == [1, 1, 0] and got["n.var"][3] < plain["n.var"][3] == 18
    assert np.all(got["n.var"] == plain["n.var"] - np.maximum(n_coll - 1, 0))
    pcol = next(c for c in cols if c.startswith("pval"))
    assert np.isfinite(got[pcol][[0, 1, 2, 3, 4, 6]]).all() and np.isnan(got[pcol][5])
    assert not same_bits(got[pcol][[2, 3, 6]], plain[pcol][[2, 3, 6]])
    for c in plain:                                             # the summary keeps describing the original variants
        if c not in cols:
            assert same_bits(got[c], plain[c]), c
    return got


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
@pytest.mark.parametrize("test", ["SKAT", "SKATO"])
def test_driver_with_reference_scanner(test, trait):
    import saigegds_amd
    fac = ref_scanner_factory()
    check_against_stored(getattr(saigegds_amd, "seqAssocGLMM_spa" + test), trait, fac)
    assert fac.calls == 1 and fac.closed == 3                   # one collapse_2bit call for all units


def test_nan_is_the_call_without_the_argument():
    from saigegds_amd import seqAssocGLMM_spaSKAT, seqAssocGLMM_spaSKATO
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import pack_dosage_2bit
    codes, mod, units, ids = CR.driver_case("binary")
    src = GenotypeSource(ids, packed=pack_dosage_2bit(codes))
    for driver in (seqAssocGLMM_spaSKAT, seqAssocGLMM_spaSKATO):
        fac = ref_scanner_factory()
        a = driver(src, mod, units, verbose=False, scanner_factory=fac)
        for nan in (float("nan"), np.float64("nan"), np.float32("nan")):
            b = driver(src, mod, units, verbose=False, scanner_factory=fac, collapse_mac=nan)
            assert list(a) == list(b) and "n.collapsed" not in b
            for c in a:
                assert same_bits(a[c], b[c]), c
        assert fac.calls == 0


def test_refusals_and_argument_errors():
    from saigegds_amd import seqAssocGLMM_spaSKAT, seqAssocGLMM_spaSKATO
    from saigegds_amd.assoc import GenotypeSource
    from saigegds_amd.gds import pack_dosage_2bit
    codes, mod, units, ids = CR.driver_case("binary")
    src = GenotypeSource(ids, packed=pack_dosage_2bit(codes))
    frac = GenotypeSource(ids, dosage=np.where(codes == 3, np.nan, codes * 0.5))
    made = []

    def no_scanner(sm):
        made.append(sm)
        raise AssertionError("a scanner was made")
    for driver in (seqAssocGLMM_spaSKAT, seqAssocGLMM_spaSKATO):
        for bad in ("10", None, True, [10], np.array([10.0])):
            with pytest.raises(TypeError, match="collapse"):
                driver(src, mod, units, verbose=False, scanner_factory=no_scanner, collapse_mac=bad)
        for bad in (0, 0.5, -1, 0.999, float("-inf")):
            with pytest.raises(ValueError, match="collapse_mac"):
                driver(src, mod, units, verbose=False, scanner_factory=no_scanner, collapse_mac=bad)
        # dosage input: refused before a scanner exists, so before any row is read
        with pytest.raises(NotImplementedError, match="'collapse_mac' on dosage input is not implemented."):
            driver(frac, mod, units[:2], verbose=False, scanner_factory=no_scanner, collapse_mac=10)
        # an integer matrix of hard calls is the 2-bit input
        ints = GenotypeSource(ids, dosage=np.where(codes == 3, 0xFF, codes).astype(np.uint8))
        fac = ref_scanner_factory()
        a = driver(ints, mod, units, verbose=False, scanner_factory=fac, collapse_mac=10)
        b = driver(src, mod, units, verbose=False, scanner_factory=fac, collapse_mac=10)
        assert list(a) == list(b) and all(same_bits(a[c], b[c]) for c in a)
        # a scanner without collapse_2bit: refused, and closed
        fac = ref_scanner_factory(collapse=False)
        with pytest.raises(NotImplementedError, match="collapse_2bit"):
            driver(src, mod, units, verbose=False, scanner_factory=fac, collapse_mac=10)
        assert fac.closed == 1
        with pytest.raises(ValueError, match="parallel"):          # refused as without the argument
            driver(src, mod, units, verbose=False, scanner_factory=no_scanner, collapse_mac=10, parallel=2,
                   grm_mat=(ids, np.eye(len(ids))))
    assert not made


def test_group_checks_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "collapse_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "saigegds_amd", "csrc"),
                    os.path.join(ROOT, "tests", "collapse_check.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "14 group lists OK" in res.stdout
