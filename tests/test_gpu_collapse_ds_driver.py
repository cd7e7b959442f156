"""``seqAssocGLMM_spaSKAT`` / ``seqAssocGLMM_spaSKATO`` with ``collapse_mac`` on dosage input, on the device (DESIGN.md
8m): the rows of tests/collapse_ds_ref.py (120 golden variants as imputed-like dosages plus constructed ultra-rare rows
with fractional carriers, some alt-major, some with missing values; N = 1000) in units of every shape.  The call with
``collapse_mac=10`` must equal, bit for bit on ``n.var``, ``Q``, every p-value column, ``rho.min`` and ``n.iter``, the same
driver without the argument on a source that stores the reference's pseudo-rows as real variants after all original
rows; ``n.collapsed`` and ``mac.collapsed`` are the reference's.  At N = 1000 the dosage score kernel takes every row in
one sample split whatever the number of rows in the call, so the table of a row does not depend on the
call it is scanned in and the comparison is exact."""
import numpy as np
import pytest

import collapse_ds_ref as DR
from test_collapse_ds_ref import BUDGET_ROWS, check_against_stored, same_bits

pytestmark = pytest.mark.gpu
# mac.collapsed of a row of fractions: ds_stats_kernel's compensated sum is the exact sum rounded once or, at worst, off
# by one more unit of the last place; min(s, 2 n - s) rounds once more.  uint8 rows: integers, exact.
MAC_ULPS = {"f64": 2, "u8": 0}


def _driver(test):
    import saigegds_amd
    return getattr(saigegds_amd, "seqAssocGLMM_spa" + test)


@pytest.mark.parametrize("kind", ["f64", "u8"])
@pytest.mark.parametrize("trait", ["binary", "quantitative"])
@pytest.mark.parametrize("test", ["SKAT", "SKATO"])
def test_collapsed_call_equals_the_stored_pseudo_rows(test, trait, kind):
    got, _ = check_against_stored(_driver(test), trait, kind, None, mac_ulps=MAC_ULPS[kind])
    print(test, trait, kind, "n.var", got["n.var"].tolist(), "n.collapsed", got["n.collapsed"].tolist(),
          "mac.collapsed", got["mac.collapsed"].tolist())


@pytest.mark.parametrize("kind", ["f64", "u8"])
@pytest.mark.parametrize("test", ["SKAT", "SKATO"])
def test_collapsed_call_with_grm_mat(test, kind):
    from test_kmat_ds_ref import family
    ids = DR.driver_case("binary", kind)[3]
    got, _ = check_against_stored(_driver(test), "binary", kind, None, mac_ulps=MAC_ULPS[kind], grm_mat=(ids, family()[0]))
    assert "n.iter" in got and got["n.iter"][[0, 1, 2, 3, 4, 6]].min() > 0 and got["n.iter"][5] == 0


@pytest.mark.parametrize("test", ["SKAT", "SKATO"])
def test_several_batches_equal_one(test):
    """Units 0-1, 2-5 and 6 are a batch each under the small budget, and unit 6 shares rare rows with units 2 and 3."""
    from saigegds_amd._lib import Scanner
    from saigegds_amd.aggregate import ds_row_bytes
    from saigegds_amd.assoc import GenotypeSource
    caps = []

    class Recording(Scanner):
        def dosage_block(self, dtype, max_variants):
            caps.append(max_variants)
            return Scanner.dosage_block(self, dtype, max_variants)
    rows, mod, units, ids = DR.driver_case("binary", "f64")
    src = GenotypeSource(ids, dosage=rows)
    one = _driver(test)(src, mod, units, verbose=False, collapse_mac=10, scanner_factory=Recording)
    cut = _driver(test)(src, mod, units, verbose=False, collapse_mac=10, scanner_factory=Recording,
                        ds_budget=BUDGET_ROWS * ds_row_bytes(np.float64, 1000))
    assert caps[1] == 78 + 4 < caps[0] == np.unique(np.concatenate(units)).size + len(units)
    assert list(one) == list(cut)
    for c in one:
        assert same_bits(one[c], cut[c]), c


def test_a_dosage_only_file(tmp_path):
    """The same rows from a file whose only genotype data is a float64 annotation/format/DS node."""
    from saigegds_amd import seqAssocGLMM_spaSKATO
    from saigegds_amd.assoc import GenotypeSource
    from test_gpu_firth_dosage_driver import _write_f64
    rows, mod, units, ids = DR.driver_case("binary", "f64")
    path = _write_f64(tmp_path / "ds.gds", rows, ids)
    got = seqAssocGLMM_spaSKATO(path, mod, units, verbose=False, collapse_mac=10)
    want = seqAssocGLMM_spaSKATO(GenotypeSource(ids, dosage=rows), mod, units, verbose=False, collapse_mac=10)
    assert list(got) == list(want) and got["n.collapsed"].sum() > 30
    for c in want:
        assert same_bits(got[c], want[c]), c
