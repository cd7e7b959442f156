"""Collapsing of ultra-rare variants on dosage input without a GPU: the numpy reference
tests/collapse_ds_ref.py against a one-sample-at-a-time loop and, on hard calls, against the 2-bit reference; the drivers
``seqAssocGLMM_spaSKAT`` / ``seqAssocGLMM_spaSKATO`` with ``collapse_mac`` through the numpy stand-in of a scanner with
dosage blocks (tests/skat_ds_ref.py) whose block has ``collapse`` = the reference, in one batch and in several; the
refusal of a block without ``collapse``; and NaN as the call without the argument."""
import math

import numpy as np
import pytest

import collapse_ds_ref as DR
import collapse_ref as CR
from aggregate_ds_ref import _NumpyDosageBlock
from skat_ds_ref import NumpySkatDsScanner, _NumpySkatDosageBlock
from test_collapse_ref import EXACT, same_bits


def loop_ref(rows, grp_ptr, var_idx, flip):
    """The definition, one sample at a time, in Python's own numbers."""
    rows = DR.resident(rows)
    u8 = rows.dtype == np.uint8
    out = np.zeros((len(grp_ptr) - 1, rows.shape[1]), dtype=rows.dtype)
    for g in range(len(grp_ptr) - 1):
        for i in range(rows.shape[1]):
            top = 0 if u8 else 0.0
            for e in range(grp_ptr[g], grp_ptr[g + 1]):
                x = int(rows[var_idx[e], i]) if u8 else float(rows[var_idx[e], i])
                if u8:
                    v = 0 if x == 0xFF else (2 - x if flip[e] else x)
                else:
                    v = 0.0 if not math.isfinite(x) else (2.0 - x if flip[e] else x)
                if v > top:
                    top = v
            out[g, i] = top
    return out


GRP_PTR, VAR_IDX = [0, 0, 1, 3, 8, 9, 11], np.array([2, 0, 1, 6, 5, 4, 3, 2, 5, 7, 7])
FLIP = np.array([0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1], dtype=np.uint8)


@pytest.mark.parametrize("kind", ["u8", "i32", "f64"])
@pytest.mark.parametrize("n", [1, 5, 33])
def test_reference_against_a_plain_loop(n, kind):
    rng = np.random.default_rng(n)
    if kind == "f64":
        rows = np.rint(rng.uniform(0, 2, (8, n)) * 64) / 64
        rows[rng.random((8, n)) < 0.2] = np.nan
        rows[5] = np.nan                                        # a row that is all missing
        rows[7, ::5] = [np.inf, -np.inf, -0.0, -0.5, 2.5, 3.0, 1e-300][:len(rows[7, ::5])]
    else:
        rows = rng.integers(0, 4 if kind == "i32" else 7, (8, n))
        miss = rng.random((8, n)) < 0.2
        miss[5] = True
        if kind == "u8":
            rows = np.where(miss, 0xFF, rows).astype(np.uint8)
            rows[7, 0] = 254
        else:
            rows = np.where(miss, DR.NA_INT, rows).astype(np.int32)
            rows[7, 0] = -1
    got, want = DR.collapse_ds_ref(rows, GRP_PTR, VAR_IDX, FLIP), loop_ref(rows, GRP_PTR, VAR_IDX, FLIP)
    assert got.dtype == (np.uint8 if kind == "u8" else np.float64) and same_bits(got, want)
    assert not got[0].any() and not got[4].any()                # no entry; the all-missing row, flipped: nothing
    assert not np.signbit(got.astype(np.float64)).any() and (got >= 0).all()      # no -0.0, no NaN, nothing negative
    if kind == "u8":
        assert got[5, 0] == 254 and got.max() < 0xFF            # row 7 unflipped and flipped: 254 enters, 2 - 254 does not
    # the order of the entries and repeats change nothing
    e = np.arange(3, 8)
    for order in (e[::-1], np.concatenate([e, e[:2]]), rng.permutation(e)):
        assert same_bits(DR.collapse_ds_ref(rows, [0, order.size], VAR_IDX[order], FLIP[order])[0], got[3])


@pytest.mark.parametrize("kind", ["u8", "i32", "f64"])
def test_hard_calls_give_the_two_bit_reference(kind):
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    n = 37
    codes = np.random.default_rng(2).integers(0, 4, (8, n)).astype(np.uint8)
    codes[5] = 3
    rows = {"u8": np.where(codes == 3, 0xFF, codes).astype(np.uint8),
            "i32": np.where(codes == 3, DR.NA_INT, codes.astype(np.int64)).astype(np.int32),
            "f64": np.where(codes == 3, np.nan, codes.astype(np.float64))}[kind]
    ref2, counts = CR.collapse_ref(pack_dosage_2bit(codes), n, GRP_PTR, VAR_IDX, FLIP)
    got = DR.collapse_ds_ref(rows, GRP_PTR, VAR_IDX, FLIP)
    assert np.array_equal(got, unpack_dosage_2bit(ref2, n))
    assert np.array_equal(got.astype(np.float64).sum(axis=1), counts[:, 0] + 2 * counts[:, 1])


# ---- the drivers through the numpy stand-in -------------------------------------------------------------------------

class _CollapseBlock(_NumpySkatDosageBlock):
    def collapse(self, grp_ptr, var_idx, flip, return_rows=False):
        """``DosageBlock.collapse``: the reference's rows appended; counts and table by the stand-in's own load and scan."""
        self.sc.collapse_calls += 1
        new = DR.collapse_ds_ref(self.rows, grp_ptr, var_idx, flip).astype(self.dtype)
        assert len(self.rows) + len(new) <= self.cap, "more rows than the block was made for"
        tmp = _NumpyDosageBlock(self.sc, self.dtype, len(new))
        n, s, st = tmp.load(new)
        self.sc.uploads -= 1
        out, valid = tmp.scan()
        self.rows = np.concatenate([self.rows, new])
        return (n, s, st, out, valid, new) if return_rows else (n, s, st, out, valid)


def ds_scanner_factory(collapse=True):
    """A scanner class that declares ``ds_collapse``; its block has ``collapse`` (or, ``collapse=False``, has not).
    Counts the scanners made and closed, the loads and the collapse calls of the last one."""
    class Fac(NumpySkatDsScanner):
        ds_collapse = True
        made = closed = 0
        caps = []

        def __init__(self, sm):
            super().__init__(sm)
            self.collapse_calls, self._open = 0, 1
            Fac.made += 1

        def dosage_block(self, dtype, max_variants):
            Fac.caps.append(max_variants)
            return (_CollapseBlock if collapse else _NumpySkatDosageBlock)(self, dtype, max_variants)

        def close(self):
            Fac.closed += self._open
            self._open = 0
            NumpySkatDsScanner.close(self)
    Fac.caps = []
    return Fac


def check_against_stored(driver, trait, kind, scanner_factory, mac_ulps=0, **kw):
    """``driver(collapse_mac=10)`` on the dosage rows against the same driver without it on ``stored_case``'s source: bit
    for bit on the columns of EXACT; ``n.collapsed`` and ``mac.collapsed`` against the reference; the summary columns those
    of the plain call -> (the result, the plain call's).  ``mac_ulps``: 0 where the scanner sums a row in numpy's order,
    as the reference does; else the bound, in units of the last place, on ``mac.collapsed`` against the correctly rounded
    sum of the pseudo-row -- a sum of fractions depends on its order, the pseudo-row itself does not."""
    from saigegds_amd.assoc import GenotypeSource
    rows, mod, units, ids = DR.driver_case(trait, kind)
    rows2, units2, n_coll, pseudo = DR.stored_case(rows, units, 10)
    got = driver(GenotypeSource(ids, dosage=rows), mod, units, verbose=False, collapse_mac=10,
                 scanner_factory=scanner_factory, **kw)
    want = driver(GenotypeSource(ids, dosage=rows2), mod, units2, verbose=False, scanner_factory=scanner_factory, **kw)
    plain = driver(GenotypeSource(ids, dosage=rows), mod, units, verbose=False, scanner_factory=scanner_factory, **kw)
    assert [k for k in got if k not in ("n.collapsed", "mac.collapsed")] == list(want) == list(plain)
    cols = [c for c in want if c.split(".b")[0] in EXACT]
    assert {"n.var"} < set(cols) and any(c.startswith("pval") for c in cols) and any(c.startswith("Q") for c in cols)
    for c in cols:
        assert same_bits(got[c], want[c]), (c, got[c], want[c])
    assert list(got["n.collapsed"]) == list(n_coll) and got["n.collapsed"].dtype == np.int64
    if mac_ulps == 0:                                           # the stand-in sums a row as the reference does
        mac = [math.nan if p is None else float(DR.counts_of(p[None, :])[2][0]) for p in pseudo]
        assert np.array_equal(got["mac.collapsed"], mac, equal_nan=True)
    else:                                                       # against the correctly rounded sum of the (bit-equal) row
        for g, p in zip(got["mac.collapsed"], pseudo):
            s = math.nan if p is None else math.fsum(p.tolist())
            mac = min(s, 2 * rows.shape[1] - s)
            assert (math.isnan(g) and p is None) or abs(g - mac) <= mac_ulps * np.spacing(mac), (g, mac)
    # the data: real mac on both sides of the cut-off among the constructed rows, alt-major and missing values among the rare
    n, s, rmac, alt = DR.counts_of(rows)
    built = rmac[CR.N_GOLD:]
    assert (built <= 10).sum() >= 20 and ((built > 10) | (kind == "u8")).any() and (built > 0).all()
    rare = (rmac > 0) & (rmac <= 10)
    assert (rare & alt).any() and (rare & (n < rows.shape[1])).any()
    if kind == "f64":
        assert (rows[rare] % 1 != 0).any() and not np.isin(rows2[len(rows):], [0.0, 1.0, 2.0]).all()
    # every unit shape occurs, and collapsing changed the test where it had something to collapse
    assert n_coll[5] == 0 and n_coll[4] == 1 and n_coll[1] >= 1 and n_coll[3] >= 10 and n_coll[2] >= 8
    assert list(got["n.var"][[4, 5]]) == [1, 0] and got["n.var"][3] < plain["n.var"][3] == 18
    assert np.all(got["n.var"] == plain["n.var"] - np.maximum(n_coll - 1, 0))
    pcol = next(c for c in cols if c.startswith("pval"))
    assert np.isfinite(got[pcol][[0, 1, 2, 3, 4, 6]]).all() and np.isnan(got[pcol][5])
    assert not same_bits(got[pcol][[2, 3, 6]], plain[pcol][[2, 3, 6]])
    for c in plain:                                             # the summary keeps describing the original variants
        if c not in cols:
            assert same_bits(got[c], plain[c]), c
    return got, plain


def _driver(test):
    import saigegds_amd
    return getattr(saigegds_amd, "seqAssocGLMM_spa" + test)


@pytest.mark.parametrize("kind", ["f64", "u8"])
@pytest.mark.parametrize("trait", ["binary", "quantitative"])
@pytest.mark.parametrize("test", ["SKAT", "SKATO"])
def test_driver_with_reference_block(test, trait, kind):
    fac = ds_scanner_factory()
    check_against_stored(_driver(test), trait, kind, fac)
    assert fac.made == fac.closed == 3
    # the collapsed call's block: room for every distinct variant and one pseudo-row a unit
    units = DR.driver_case(trait, kind)[2]
    assert fac.caps[0] == np.unique(np.concatenate(units)).size + len(units)


BUDGET_ROWS = 60        # resident rows of the several-batch calls: units 0-1, 2-5 and 6 (78 rows: a batch of its own) are a batch each


@pytest.mark.parametrize("test", ["SKAT", "SKATO"])
def test_several_batches_equal_one(test):
    from saigegds_amd.aggregate import ds_row_bytes
    from saigegds_amd.assoc import GenotypeSource
    rows, mod, units, ids = DR.driver_case("binary", "f64")
    src = GenotypeSource(ids, dosage=rows)
    fac = ds_scanner_factory()
    one = _driver(test)(src, mod, units, verbose=False, collapse_mac=10, scanner_factory=fac)
    assert fac.last.uploads == 1 and fac.last.collapse_calls == 1
    cut = _driver(test)(src, mod, units, verbose=False, collapse_mac=10, scanner_factory=fac,
                        ds_budget=BUDGET_ROWS * ds_row_bytes(np.float64, 1000))
    assert fac.last.uploads == 3 and fac.last.collapse_calls == 3 and fac.caps[1] == 78 + 4 < fac.caps[0]      # the largest batch's rows + the most units
    assert set(units[6]) & set(units[2]) and set(units[6]) & set(units[3])      # batches share rare rows
    assert list(one) == list(cut)
    for c in one:
        assert same_bits(one[c], cut[c]), c
    # without collapsing the same budget takes no row for pseudo-variants: the accounting differs only where asked
    _driver(test)(src, mod, units, verbose=False, scanner_factory=fac, ds_budget=BUDGET_ROWS * ds_row_bytes(np.float64, 1000))
    assert fac.caps[2] == 78 and fac.last.collapse_calls == 0


def test_a_block_without_collapse_is_refused_and_closed():
    from saigegds_amd.assoc import GenotypeSource
    rows, mod, units, ids = DR.driver_case("binary", "f64")
    for test in ("SKAT", "SKATO"):
        fac = ds_scanner_factory(collapse=False)
        with pytest.raises(NotImplementedError, match="collapse"):
            _driver(test)(GenotypeSource(ids, dosage=rows), mod, units, verbose=False, collapse_mac=10, scanner_factory=fac)
        assert fac.made == fac.closed == 1 and fac.last.uploads == 0      # refused before any row went up
        # a scanner class that does not declare the capability: the message of a plain function, no scanner made
        with pytest.raises(NotImplementedError, match="'collapse_mac' on dosage input is not implemented."):
            _driver(test)(GenotypeSource(ids, dosage=rows), mod, units, verbose=False, collapse_mac=10,
                          scanner_factory=NumpySkatDsScanner)


def test_nan_is_the_call_without_the_argument():
    from saigegds_amd.assoc import GenotypeSource
    rows, mod, units, ids = DR.driver_case("binary", "f64")
    src = GenotypeSource(ids, dosage=rows)
    for test in ("SKAT", "SKATO"):
        fac = ds_scanner_factory()
        a = _driver(test)(src, mod, units, verbose=False, scanner_factory=fac)
        for nan in (float("nan"), np.float64("nan"), np.float32("nan")):
            b = _driver(test)(src, mod, units, verbose=False, scanner_factory=fac, collapse_mac=nan)
            assert list(a) == list(b) and "n.collapsed" not in b
            for c in a:
                assert same_bits(a[c], b[c]), c
            assert fac.last.collapse_calls == 0
        assert len(set(fac.caps)) == 1                          # and no room for pseudo-rows is asked for
