"""saigegds_amd -- MI355X-native single-variant association scan of SAIGEgds.

Public surface (mirrors the reference's R API for this path):
    seqAssocGLMM_SPA   host driver of the scan        (R/assoc_single.r:92-334)
    load_modobj        .check_modobj                  (R/saige_main.r:93-111)
    init_nullmod       .init_nullmod                  (R/assoc_single.r:17-67)
    seqGLMM_GxG_spa    SNP x SNP interaction test     (R/saige_interaction.r:44-641)
    seqAssocGLMM_spaSKAT  variance-component set test (not in the reference)
    seqAssocGLMM_spaSKATO SKAT-O: burden and SKAT combined over a grid of rho (not in the reference)
    seqAssocGLMM_SPA_cond scan given a set of conditioning variants (not in the reference)
    seqFitDenseGRM, seqFitSparseGRM  the explicit GRM, dense and thresholded (not in the reference)
    load_grm, ExplicitGrmOperator    read it back; the operator seqFitNullGLMM_SPA(grm_mat=) fits on
    exact_pass, EXACT_MAX_MAC  exact p-values of ultra-rare rows, seqAssocGLMM_SPA(exact_mac=) (not in the reference)
    seqFitLDpruning    LD pruning of the GRM markers, the vignette's first step (upstream 2.x)
    ld_counts_2bit, ld_corr  the pairwise LD sums of 2-bit rows on the device, and r from them
    seqFitPCA, pca_project, load_pca  top principal components of the GRM on its operator, projection of left-out
                       samples on the SNP loadings (the reference leaves PCA to SNPRelate)
    seqFitKING, KingResult, load_king, unrelated_set  KING-robust kinship pairs without allele frequencies, and a maximal
                       unrelated set from them (the reference leaves this to SNPRelate)
    seqSAIGE_LoadPval  load saved association results     (R/saige_main.r:164-215)
The compute lives in libsaigehip.so (include/saigehip.h); there is no CPU path.
"""
from .nullmod import NullModel, ScanModel, init_nullmod, load_modobj  # noqa: F401
from .assoc import GenotypeSource, seqAssocGLMM_SPA  # noqa: F401
from .fitnull import FittedNullModel, glmmHeritability, seqFitNullGLMM_SPA  # noqa: F401
from .gxg import DosageMatrix, GxGTable, saddle_prob, seqGLMM_GxG_spa  # noqa: F401
from .aggregate import (AggrParamBeta, pACAT, pACAT2, seqAssocGLMM_spaACAT_O, seqAssocGLMM_spaACAT_V,  # noqa: F401
                        seqAssocGLMM_spaBurden)
from .skat import pchisq_mix, seqAssocGLMM_spaSKAT  # noqa: F401
from .skato import pchisq_mix_vec, seqAssocGLMM_spaSKATO, skato_pvalue  # noqa: F401
from .cond import cond_tests, seqAssocGLMM_SPA_cond  # noqa: F401
from .grm import SparseGRM, load_grm, seqFitDenseGRM, seqFitSparseGRM  # noqa: F401
from ._lib import ExplicitGrmOperator, ld_corr, ld_counts_2bit  # noqa: F401
from .ldprune import seqFitLDpruning  # noqa: F401
from .pca import load_pca, pca_project, seqFitPCA  # noqa: F401
from .king import KingResult, load_king, seqFitKING, unrelated_set  # noqa: F401
from .results import seqSAIGE_LoadPval  # noqa: F401
from .exact import EXACT_MAX_MAC, exact_pass  # noqa: F401

__version__ = "0.1.0"
