"""seqAssocGLMM_SPA(exact_mac=) on the device: a small synthetic source with rows of MAC 1..10 (the golden genotypes
thinned as in tests/test_exact_driver.py) and the golden model at mac = 1, exact_mac = 10 -- pval.exact against
Scanner.exact_2bit on the same rows bit for bit, against the rational reference of tests/exact_ref.py within the bound of
DESIGN.md 9, and every other column against the run without the argument bit for bit."""
import numpy as np
import pytest

import exact_ref as R
from conftest import REL_TOL, load_null_model
from test_exact_driver import M, _codes, _source

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()
    yield


def test_exact_columns_of_a_run():
    from saigegds_amd import firth
    from saigegds_amd._lib import Scanner
    from saigegds_amd.assoc import seqAssocGLMM_SPA
    from saigegds_amd.gds import pack_dosage_2bit
    from saigegds_amd.nullmod import init_nullmod
    mod = load_null_model("saige_model.npz")
    plain = seqAssocGLMM_SPA(_source(), mod, mac=1, verbose=False)
    got = seqAssocGLMM_SPA(_source(), mod, mac=1, verbose=False, exact_mac=10)
    assert list(got) == list(plain) + ["pval.exact", "pval.exact.full"]
    for k in plain:                                          # every scan column bit for bit
        a, b = np.asarray(plain[k]), np.asarray(got[k])
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
    rare = got["mac"] <= 10
    assert 50 < rare.sum() < rare.size and set(range(1, 11)) <= set(got["mac"][rare].astype(int))
    assert np.isnan(got["pval.exact"][~rare]).all() and np.isnan(got["pval.exact.full"][~rare]).all()

    g, codes = _codes()
    rows = np.flatnonzero(np.isin(g["variant_id"][:M], np.asarray(got["id"])[rare]))
    packed = pack_dosage_2bit(codes[rows])
    lut, flip = firth.firth_tables(got["AF.alt"][rare])
    assert flip.any() and (codes[rows] == 3).any()
    sm = init_nullmod(mod, np.arange(len(mod.sample_id)), float("nan"), 1, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
    with Scanner(sm) as sc:
        o4 = sc.exact_2bit(packed, lut, 10)
    assert np.all(o4[:, 3] == 1) and np.array_equal(o4[:, 2], got["mac"][rare])
    assert got["pval.exact"][rare].tobytes() == o4[:, 0].tobytes()
    assert got["pval.exact.full"][rare].tobytes() == o4[:, 1].tobytes()
    ref = R.exact_ref(sm.mu, sm.y, packed, lut, 10)
    for c, name in ((0, "pval.exact"), (1, "pval.exact.full")):
        err = np.abs(o4[:, c] - ref[:, c]) / ref[:, c]
        print(f"{name}: off by {float(err.max()):.3g} relative at worst over {int(rare.sum())} rows")
        assert np.all(err <= REL_TOL), name
