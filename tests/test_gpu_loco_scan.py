"""GPU: the leave-one-chromosome-out fit on the HIP operator (all chromosomes in lockstep through pcg_loco)
against the per-chromosome subset-operator fit of test_fit_loco.py, and seqAssocGLMM_SPA with a LOCO model
against plain scans of each chromosome's variants."""
import os
from dataclasses import replace

import numpy as np
import pytest

from saigegds_amd.assoc import GenotypeSource, match_samples, seqAssocGLMM_SPA
from saigegds_amd.fitnull import seqFitNullGLMM_SPA
from saigegds_amd.nullmod import NullModel, init_nullmod
from test_fit_loco import _data, three_chromosome_source

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()
    yield


@pytest.mark.parametrize("trait", ["binary", "quantitative"])
def test_lockstep_fit_matches_the_subset_operator_fit(trait):
    from oracle.oracle import GrmOracle
    src = three_chromosome_source(step=16)
    kw = dict(trait_type=trait, verbose=False, loco=True)
    formula = "y ~ x1 + x2" if trait == "binary" else "yy ~ x1 + x2"
    gpu = seqFitNullGLMM_SPA(formula, _data(), src, **kw)
    cpu = seqFitNullGLMM_SPA(formula, _data(), src, operator_factory=GrmOracle, **kw)
    assert list(gpu.loco) == list(cpu.loco) == ["1", "2", "X"]
    print(trait, "tau", gpu.tau, cpu.tau, "steps", gpu.loco_steps)
    for ch in cpu.loco:
        assert gpu.loco_steps[ch] == cpu.loco_steps[ch], (ch, gpu.loco_steps[ch], cpu.loco_steps[ch])
        want = cpu.loco[ch]["fitted_values"]
        np.testing.assert_allclose(gpu.loco[ch]["fitted_values"], want, rtol=1e-8, atol=1e-10 * np.max(np.abs(want)), err_msg=ch)
        assert not np.array_equal(gpu.loco[ch]["fitted_values"], gpu.fitted_values)


def _scan_inputs():
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    z = np.load(os.path.join(GOLD, "saige_model.npz"))
    mod = NullModel(trait_type="binary", tau=z["tau"], fitted_values=z["fitted_values"], sample_id=list(z["sample_id"]),
                    var_ratio=z["var_ratio"], y=z["y"], V=z["V"], X1=z["X1"], XV=z["XV"], XXVX_inv=z["XXVX_inv"])
    # chromosome runs shorter than a block; 1 comes twice; X has no LOCO entry
    chrom = ["1"] * 100 + ["2"] * 120 + ["X"] * 50 + ["1"] * 30
    m = len(chrom)

    def source(rows):
        return GenotypeSource(list(g["sample_id"]), packed=np.ascontiguousarray(g["packed"][:m][rows]),
                              variant_id=g["variant_id"][:m][rows], chromosome=list(np.asarray(chrom)[rows]),
                              position=g["position"][:m][rows])

    rng = np.random.default_rng(3)
    mu = mod.fitted_values
    loco = {ch: {"fitted_values": np.clip(mu * rng.uniform(0.8, 1.2, mu.size), 1e-3, 1 - 1e-3)} for ch in ("1", "2")}
    return mod, loco, chrom, source


def _ndev():
    from saigegds_amd._lib import load
    return load().sgx_device_count()


@pytest.mark.parametrize("parallel", [1, 2])
def test_scan_uses_each_chromosomes_model(parallel, capsys):
    if parallel > _ndev():
        pytest.skip("one device visible")
    mod, loco, chrom, source = _scan_inputs()
    every = np.arange(len(chrom))
    got = seqAssocGLMM_SPA(source(every), replace(mod, loco=loco), mac=4, parallel=parallel, verbose=True)
    assert capsys.readouterr().out.count("chromosome 'X' has no leave-one-chromosome-out model") == 1
    parts = []
    for r0, r1 in ((0, 100), (100, 220), (220, 270), (270, 300)):
        ch = chrom[r0]
        m_run = replace(mod, fitted_values=loco[ch]["fitted_values"]) if ch in loco else mod
        parts.append(seqAssocGLMM_SPA(source(every[r0:r1]), m_run, mac=4, verbose=False))
    assert list(got) == list(parts[0])
    for k in got:
        want = np.concatenate([np.asarray(p[k]) for p in parts])
        assert np.array_equal(np.asarray(got[k]), want, equal_nan=(want.dtype.kind == "f")), k
    # the models differ where it matters: the full model gives another table
    full = seqAssocGLMM_SPA(source(every), mod, mac=4, verbose=False)
    assert not np.array_equal(full["pval"], got["pval"])
    x = np.asarray(got["chr"]) == "X"
    assert x.any() and np.array_equal(np.asarray(full["pval"])[np.asarray(full["chr"]) == "X"], np.asarray(got["pval"])[x])


def test_model_without_loco_takes_the_plain_path():
    from saigegds_amd._lib import Scanner
    mod, _, chrom, source = _scan_inputs()
    src = source(np.arange(len(chrom)))
    got = seqAssocGLMM_SPA(src, mod, mac=4, verbose=False)
    ii = match_samples(src, mod)[2]
    sm = init_nullmod(mod, ii, float("nan"), 4, 0.1, 0.05, float(np.nanmean(mod.var_ratio)))
    with Scanner(sm, device=0) as sc:
        out, valid = sc.scan_2bit(src.packed)
    keep = valid.astype(bool)
    assert np.array_equal(np.asarray(got["id"]), src.variant_id[keep])
    for k, col in (("AF.alt", 0), ("mac", 1), ("beta", 3), ("SE", 4), ("pval", 5), ("p.norm", 6)):
        assert np.array_equal(got[k], out[keep, col], equal_nan=True), k
    assert np.array_equal(got["num"], out[keep, 2].astype(np.int32)) and np.array_equal(got["converged"], out[keep, 7] == 1)
