"""Firth bias-reduced effect sizes for the rows a binary-trait scan flags (``seqAssocGLMM_SPA(firth_pval=)``).

The scan's ``beta`` is the one-step score estimate ``S / var``: biased for rare variants at an unbalanced case/control
ratio, and without a meaning where every carrier is a case.  The reference has nothing in its place (SAIGE proper has
``--is_Firth_beta`` / ``--pCutoffforFirth``), so nothing here mirrors reference code and no reference vector pins it;
the definition is DESIGN.md 8j.  With the null model's fitted mean ``mu`` as offset the penalised fit of a row has one
parameter,

    logit p_i = logit mu_i + beta g_i,    w_i = p_i (1 - p_i),
    I = sum w g^2,   A = sum w (1 - 2p) g^3,   U*(beta) = sum g (y - p) + A / 2I,

``beta.firth`` is the root of ``U*`` (the score of ``loglik + 1/2 log I``) and ``SE.firth = 1 / sqrt(I)`` there.  ``g`` is
the scan's own dosage -- mean imputation and the flip to the minor allele, ``aggregate.dosage_tables`` -- so only the
samples with ``g != 0`` enter, and the sign is turned back to the alt allele like ``beta`` and ``beta.cond``.

``firth_pass`` is the host side: it takes the flagged rows in batches of bounded bytes, reads their 2-bit rows
(``ScanInput.packed_rows_at``: in-memory sources, host-decoded and device-decoded files alike), forms the tables from
the ``AF.alt`` column and talks to the device through ``Scanner.firth_2bit`` alone (``sgx_firth_2bit``, kern_firth.h).
Out of scope: dosage rows, the set-test and conditional drivers, more than one GPU.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Tuple

import numpy as np

from . import aggregate

FIRTH_BATCH_BYTES = 1 << 30     # host bytes of 2-bit rows per firth_2bit call
NO_DOSAGE = "Firth effect sizes on dosage input are not implemented."


def firth_tables(af: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``AF.alt`` of rows -> (their dosage tables [m, 4], flip): the scan's own imputation (2 AF for a missing
    genotype) and flip (AF > 0.5), by ``aggregate.dosage_tables``.  A non-finite AF gives a non-finite table."""
    af = np.asarray(af, dtype=np.float64)
    flip = af > 0.5
    mean = np.where(flip, 2 - 2 * af, 2 * af)
    return aggregate.dosage_tables(flip.astype(np.uint8), mean), flip


def hard_call_input(inp):
    """The opened input of a driver call as 2-bit rows: hard calls as they are, an in-memory uint8 / int32 matrix that
    holds 0, 1, 2 and the missing code only as the rows it means (``aggregate.reduce_hard_calls``); any other input --
    a dosage node, a file of dosages only, a matrix of other values -- is refused."""
    if inp.kind == "dosage" and inp.in_mem:
        ds = np.asarray(inp.ds_all)
        if ds.ndim == 2 and ds.dtype in (np.uint8, np.int32):
            inp = aggregate.reduce_hard_calls(dataclasses.replace(inp, ds_all=ds, ds_dtype=ds.dtype))
    if inp.kind != "packed":
        raise NotImplementedError(NO_DOSAGE)
    return inp


def firth_pass(inp, out: np.ndarray, valid: np.ndarray, rows, make_scanner: Callable, maxit: int = 50):
    """Firth fits of the variants ``rows`` (0-based indices into the input's variants) of a finished scan: ``out``
    [n_var, 8] and ``valid`` [n_var] are the scan's table and flags.  ``make_scanner()`` gives an object with
    ``firth_2bit(packed, lut, maxit)`` and ``close()`` for the model of these rows.  -> (beta, SE, converged), each
    [n_var]: NaN / NaN / False off ``rows``; beta refers to the alt allele."""
    n_var = out.shape[0]
    beta, se = np.full(n_var, np.nan), np.full(n_var, np.nan)
    cvg = np.zeros(n_var, dtype=bool)
    rows = np.unique(np.asarray(rows, dtype=np.int64))
    rows = rows[np.asarray(valid)[rows] != 0]
    if rows.size == 0:
        return beta, se, cvg
    if inp.kind != "packed":
        raise NotImplementedError(NO_DOSAGE)
    per = max(1, FIRTH_BATCH_BYTES // max(1, (inp.n_samp + 3) // 4))
    sc = make_scanner()
    try:
        for a in range(0, rows.size, per):
            idx = rows[a:a + per]
            lut, flip = firth_tables(out[idx, 0])
            o4 = np.asarray(sc.firth_2bit(inp.packed_rows_at(idx), lut, int(maxit)))
            beta[idx] = np.where(flip, -o4[:, 0], o4[:, 0])
            se[idx] = o4[:, 1]
            cvg[idx] = o4[:, 3] == 1
    finally:
        sc.close()
    return beta, se, cvg
