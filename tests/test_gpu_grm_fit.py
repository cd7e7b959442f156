"""GPU: seqFitDenseGRM / seqFitSparseGRM on the reference's golden file through the HIP operator, against the numpy
stand-in of grm_dense_ref.py on the same markers."""
import os

import numpy as np
import pytest

import grm_dense_ref as D
import grm_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

GDS = os.path.join(os.path.dirname(__file__), "golden", "grm1k_10k_snp.gds")
ARGS = dict(maf=0.005, missing_rate=0.01, max_num_snp=2000, seed=200, verbose=False)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()
    yield


def test_fit_matches_the_stand_in():
    from saigegds_amd import seqFitDenseGRM, seqFitSparseGRM
    from saigegds_amd.gds import unpack_dosage_2bit
    keep = {}

    def spy(packed, n):
        keep["op"] = D.NumpyGrm(packed, n)
        return keep["op"]

    ids_ref, K_ref = seqFitDenseGRM(GDS, operator_factory=spy, **ARGS)
    ids, K = seqFitDenseGRM(GDS, **ARGS)
    assert ids == ids_ref and K.shape == (1000, 1000) and np.array_equal(K, K.T)
    ref = D.reference(unpack_dosage_2bit(keep["op"].packed, 1000))
    e, e_ref = D.scaled_error(K, ref), D.scaled_error(K_ref, ref)
    e_both = D.scaled_error(K, D.Ref(K_ref.astype(R.LD), ref.scale))
    print("\nscaled error: HIP %.4g, stand-in %.4g, HIP against the stand-in %.4g" % (e, e_ref, e_both))
    assert e <= 4 * D.E_DENSE and e_both <= 4 * D.E_DENSE
    sp = seqFitSparseGRM(GDS, rel_cutoff=0.125, **ARGS)
    sp_ref = seqFitSparseGRM(GDS, rel_cutoff=0.125, operator_factory=D.NumpyGrm, **ARGS)
    assert float(np.min(np.abs(ref.K - R.LD(0.125)))) > 1e-9           # no entry near the cutoff: the sets are equal
    assert np.array_equal(sp.i, sp_ref.i) and np.array_equal(sp.j, sp_ref.j) and sp.sample_id == ids
    wi, wj, wx = D.threshold(K, 0.125)
    assert np.array_equal(sp.i, wi) and np.array_equal(sp.x, wx)
    assert np.array_equal(sp.to_dense()[sp.i, sp.j], K[sp.i, sp.j])
