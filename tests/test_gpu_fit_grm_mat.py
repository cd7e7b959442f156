"""``seqFitNullGLMM_SPA(grm_mat=)`` through the HIP operators (``ExplicitGrmOperator``): the golden models in dense and
CSR storage, and a fit on ``seqFitSparseGRM``'s own output against the numpy stand-in, followed by a scan."""
import functools
import os

import numpy as np
import pytest

import kmat_ref as KR
from saigegds_amd import (SparseGRM, seqAssocGLMM_SPA, seqFitDenseGRM, seqFitNullGLMM_SPA, seqFitSparseGRM)
from test_fit_grm_mat import GDS, GOLD, TRAITS, pheno
from test_fitnull import TOL, _check_model, _mean_rel

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_grm():
    ids, K = seqFitDenseGRM(GDS, verbose=False)
    i, j = np.triu_indices(len(ids))
    sp = SparseGRM(sample_id=list(ids), n=len(ids), n_markers=0, rel_cutoff=-1e300, i=i.astype(np.int32),
                   j=j.astype(np.int32), x=K[i, j])
    return (list(ids), K), sp


@pytest.mark.parametrize("storage", ["dense", "csr"])
@pytest.mark.parametrize("trait", list(TRAITS))
def test_grm_mat_on_the_device_reproduces_golden_model(trait, storage):
    grm = device_grm()[0 if storage == "dense" else 1]
    m = seqFitNullGLMM_SPA(TRAITS[trait][0], pheno(), GDS, trait_type=trait, verbose=False, grm_mat=grm)
    _check_model(m, np.load(os.path.join(GOLD, TRAITS[trait][1])))


def test_fit_on_thresholded_grm_matches_stand_in_then_scans():
    sp = seqFitSparseGRM(GDS, rel_cutoff=0.125, verbose=False)
    assert sp.n == 1000 and (sp.i == sp.j).sum() == 1000
    kw = dict(trait_type="binary", verbose=False, grm_mat=sp)
    m = seqFitNullGLMM_SPA(TRAITS["binary"][0], pheno(), GDS, **kw)
    r = seqFitNullGLMM_SPA(TRAITS["binary"][0], pheno(), GDS, operator_factory=KR.KmatRef, **kw)
    assert list(m.sample_id) == list(r.sample_id) and bool(m.converged) == bool(r.converged)
    assert np.array_equal(np.asarray(m.var_ratio_table["id"]), np.asarray(r.var_ratio_table["id"]))
    for k in ("tau", "coefficients", "fitted_values", "linear_predictors", "residuals", "cov", "var_ratio"):
        assert _mean_rel(getattr(m, k), getattr(r, k)) < TOL, k
    res = seqAssocGLMM_SPA(GDS, m, mac=4, verbose=False)
    assert len(res["pval"]) > 0 and np.isfinite(np.asarray(res["pval"], dtype=np.float64)).all()
