"""``seqFitNullGLMM_SPA(grm_mat=)``: the null model on an explicit GRM, with the numpy stand-in injected.

The reference has no explicit GRM, so this path is tied to the pinned implicit operator: the dense K = G'G/M of the
markers the fit picks, passed as ``grm_mat``, must reproduce the reference's golden models under the rule of
tests/test_fitnull.py (mean relative difference per field below 1e-4, the same variance-ratio markers)."""
import functools
import os
import re

import numpy as np
import pytest

import grm_dense_ref as D
import kmat_ref as KR
from saigegds_amd import SparseGRM, seqFitDenseGRM, seqFitNullGLMM_SPA
from test_fitnull import _check_model

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GDS = os.path.join(GOLD, "grm1k_10k_snp.gds")
TRAITS = {"binary": ("y ~ x1 + x2", "saige_model.npz"), "quantitative": ("yy ~ x1 + x2", "saige_model_quant.npz")}
FIELDS = ("tau", "coefficients", "fitted_values", "linear_predictors", "residuals", "cov", "var_ratio")


def pheno():
    ph = np.load(os.path.join(GOLD, "pheno.npz"))
    return {"sample.id": ph["sample_id"], "y": ph["y"], "yy": ph["yy"], "x1": ph["x1"], "x2": ph["x2"]}


@functools.lru_cache(maxsize=None)
def dense_grm():
    """(sample_id, K) of the markers the fit picks by default, K read-only."""
    ids, K = seqFitDenseGRM(GDS, verbose=False, operator_factory=D.NumpyGrm)
    K.setflags(write=False)
    return list(ids), K


@functools.lru_cache(maxsize=None)
def all_pairs_grm():
    """The same matrix as a SparseGRM that holds every pair."""
    ids, K = dense_grm()
    i, j, x = D.threshold(K, D.EVERYTHING)
    return SparseGRM(sample_id=ids, n=len(ids), n_markers=0, rel_cutoff=D.EVERYTHING, i=i, j=j, x=x)


def fit(trait, grm_mat, factory=KR.KmatRef, **kw):
    return seqFitNullGLMM_SPA(TRAITS[trait][0], pheno(), GDS, trait_type=trait, verbose=False, grm_mat=grm_mat,
                              operator_factory=factory, **kw)


@functools.lru_cache(maxsize=None)
def dense_fit(trait):
    return fit(trait, dense_grm())


@functools.lru_cache(maxsize=None)
def sparse_fit(trait):
    return fit(trait, all_pairs_grm())


def same_model(a, b):
    for k in FIELDS:
        assert np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), k
    assert list(a.sample_id) == list(b.sample_id)
    assert np.array_equal(np.asarray(a.var_ratio_table["id"]), np.asarray(b.var_ratio_table["id"]))


@pytest.mark.parametrize("trait", list(TRAITS))
def test_dense_grm_mat_reproduces_golden_model(trait):
    _check_model(dense_fit(trait), np.load(os.path.join(GOLD, TRAITS[trait][1])))


@pytest.mark.parametrize("trait", list(TRAITS))
def test_sparse_grm_mat_with_every_pair_reproduces_golden_model(trait):
    _check_model(sparse_fit(trait), np.load(os.path.join(GOLD, TRAITS[trait][1])))


def test_shuffled_superset_gives_the_same_bits():
    ids, K = dense_grm()
    rng = np.random.default_rng(4)
    n = len(ids)
    big = np.zeros((n + 3, n + 3))
    big[:n, :n] = K
    big[n:, n:] = np.eye(3)
    big[n, 0] = big[0, n] = 0.3
    bids = ids + ["extra1", "extra2", "extra3"]
    p = rng.permutation(n + 3)
    shuffled = ([bids[k] for k in p], big[np.ix_(p, p)])
    same_model(fit("binary", shuffled), dense_fit("binary"))
    i, j, x = D.threshold(shuffled[1], D.EVERYTHING)
    sp = SparseGRM(sample_id=shuffled[0], n=n + 3, n_markers=0, rel_cutoff=D.EVERYTHING, i=i, j=j, x=x)
    same_model(fit("binary", sp), sparse_fit("binary"))


def test_operator_factory_gets_the_aligned_matrix():
    ids, K = dense_grm()
    seen = []

    class Stop(Exception):
        pass

    def factory(grm, n):
        seen.append((grm, n))
        raise Stop

    with pytest.raises(Stop):
        fit("binary", (ids[::-1], np.ascontiguousarray(K[::-1, ::-1])), factory)
    assert seen[0][1] == len(ids) and np.array_equal(seen[0][0], K)
    with pytest.raises(Stop):
        fit("binary", all_pairs_grm().subset(ids[::-1]), factory)
    assert isinstance(seen[1][0], SparseGRM) and seen[1][0].sample_id == ids
    assert np.array_equal(seen[1][0].to_dense(), K)


def test_argument_errors():
    ids, K = dense_grm()
    with pytest.raises(ValueError, match=rf"not in 'grm_mat': \['{re.escape(ids[0])}'\]"):
        fit("binary", (ids[1:], K[1:, 1:]))
    with pytest.raises(ValueError, match=r"not in 'grm_mat'"):
        fit("binary", all_pairs_grm().subset(ids[5:]))
    with pytest.raises(ValueError, match="loco"):
        fit("binary", dense_grm(), loco=True)
    with pytest.raises(ValueError, match="square"):
        fit("binary", (ids, K[:, :-1]))
    with pytest.raises(ValueError, match="SparseGRM"):
        fit("binary", 3.5)


@pytest.mark.parametrize("ext", ["npz", "rds"])
def test_file_name_equals_object(ext, tmp_path):
    fn = str(tmp_path / f"grm.{ext}")
    ids, K = seqFitDenseGRM(GDS, verbose=False, operator_factory=D.NumpyGrm, out_fn=fn)
    assert np.array_equal(K, dense_grm()[1])
    same_model(fit("quantitative", fn), dense_fit("quantitative"))
