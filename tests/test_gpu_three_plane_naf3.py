"""The three-plane contraction kernel at four B fragments (K = 3 binary, the headline's form): three row pieces per
consumer wave, one set of plane registers, variant tiles of 24 fragments = 384 variants.  Variant counts around one
tile, below it, and with leftover tiles cut into pieces; ragged N up to 430 000; two missing rates.  Every case scans
the same rows with the three-plane form and with the two-plane form (lists of the missing genotypes), and holds both
against the oracle: the score stage's integers are the same, so AF, mac, num and validity agree to the bit and the
other columns to rounding (the SPA lists are filled in another order)."""
import numpy as np
import pytest

from conftest import assert_table_close

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600, method="thread")]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """Import torch before the first HIP call of this process (libsaigehip.so binds to the torch wheel's runtime)."""
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    yield


def _case(n, m, miss, seed):
    from saigegds_amd import synth
    from saigegds_amd.nullmod import init_nullmod
    mod = synth.synth_null_model(n, "binary", 0.05, n_cov=3, seed=seed)
    sm = init_nullmod(mod, np.arange(n), float("nan"), 10, 0.1, 0.05, float(mod.var_ratio[0]))
    thr = synth.variant_thresholds(0, m, seed, log10_maf=(-2.5, -0.3), flip_frac=0.3, miss_rate=miss)
    return sm, synth.synth_packed(n, 0, m, seed, thr)


def _both_forms(n, m, miss, seed):
    from oracle import Oracle
    from saigegds_amd._lib import Scanner
    sm, packed = _case(n, m, miss, seed)
    ref, ref_valid = Oracle(sm).scan_2bit(packed)
    res = {}
    with Scanner(sm, device=0) as sc:
        limbs, _ = sc.score_layout()
        assert (int(limbs.sum()) + 1 + 15) // 16 + 1 == 4, "not the four-fragment form"
        for form in (1, 0):
            sc.set_option("three_plane", form)
            out, valid = sc.scan_2bit(packed)
            st = sc.stats()
            assert st["three_plane"] == form, st
            assert_table_close(out, valid, ref, ref_valid, what=f"three_plane={form} N={n} M={m} miss={miss}")
            res[form] = (out, valid)
    assert np.array_equal(res[0][1], res[1][1])
    v = ref_valid.astype(bool)
    assert np.array_equal(res[0][0][v][:, :3], res[1][0][v][:, :3])
    np.testing.assert_allclose(res[0][0][v][:, 3:7], res[1][0][v][:, 3:7], rtol=1e-11)


@pytest.mark.parametrize("miss", [1e-3, 0.04])
@pytest.mark.parametrize("m", [383, 384, 385, 100, 3 * 384 + 131])
def test_variant_counts_around_a_tile(m, miss):
    """N = 16 411 (not a multiple of 512; below 16 384 samples every column gets one limb more and K = 3 needs five
    B fragments): one tile less one, one tile, one tile and one variant, less than a tile, and leftover tiles that the
    work plan cuts into sample pieces."""
    _both_forms(16_411, m, miss, seed=71 + m)


@pytest.mark.parametrize("n,m", [(70_001, 1000), (430_000, 385)])
@pytest.mark.parametrize("miss", [1e-3, 0.04])
def test_long_rows(n, m, miss):
    """Long rows: N = 70 001 (not a multiple of 512) and the headline's N = 430 000."""
    _both_forms(n, m, miss, seed=83)
